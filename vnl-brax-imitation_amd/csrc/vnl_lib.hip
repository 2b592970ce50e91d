// C-ABI (include/vnl.h) + kernels of the rodent rollout for gfx950.
// Build: hipcc --offload-arch=gfx950 -O3 -shared -fPIC (see csrc/build.py).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <map>
#include <string>
#include <vector>

#include "../../include/vnl.h"
#include "vnl_body.h"
#include "vnl_inertial.h"

// ----------------------------------------------------------------------------- errors
static thread_local char g_err[512] = "";
static int fail(int code, const char* fmt, const char* a = "", const char* b = "") {
  snprintf(g_err, sizeof(g_err), fmt, a, b);
  return code;
}
#define HIPCHK(call)                                                              \
  do {                                                                            \
    hipError_t e_ = (call);                                                       \
    if (e_ != hipSuccess) return fail(VNL_ERR_HIP, "%s: %s", #call, hipGetErrorString(e_)); \
  } while (0)

extern "C" const char* vnl_last_error(void) { return g_err; }
void vnl_set_error_(const char* msg) { snprintf(g_err, sizeof(g_err), "%s", msg); }  // used by vnl_policy.hip
extern "C" int vnl_version(void) { return 1; }

// ----------------------------------------------------------------------------- blob
struct BlobEntry {
  char name[24];
  uint32_t dtype, count;
  uint64_t offset;
};

struct vnl_model {
  std::map<std::string, std::vector<double>> f;
  std::map<std::string, std::vector<int>> i;
  double scalar(const char* k) const {
    auto it = f.find(k);
    return (it == f.end() || it->second.size() != 1) ? NAN : it->second[0];
  }
  bool has_f(const char* k, size_t n) const {
    auto it = f.find(k);
    return it != f.end() && it->second.size() == n;
  }
  bool has_i(const char* k, size_t n) const {
    auto it = i.find(k);
    return it != i.end() && it->second.size() == n;
  }
};

extern "C" int vnl_model_create(const void* blob, size_t nbytes, vnl_model** out) {
  if (!blob || !out) return fail(VNL_ERR_ARG, "vnl_model_create: null argument");
  const uint8_t* b = (const uint8_t*)blob;
  if (nbytes < 16 || memcmp(b, "VNLMDL01", 8) != 0) return fail(VNL_ERR_BLOB, "bad blob magic");
  uint32_t ns;
  memcpy(&ns, b + 8, 4);
  if (16 + (size_t)ns * sizeof(BlobEntry) > nbytes) return fail(VNL_ERR_BLOB, "truncated blob directory");
  vnl_model* m = new vnl_model();
  const BlobEntry* e = (const BlobEntry*)(b + 16);
  for (uint32_t k = 0; k < ns; k++) {
    size_t esz = e[k].dtype == 1 ? 8 : 4;
    if (e[k].offset + esz * e[k].count > nbytes) {
      delete m;
      return fail(VNL_ERR_BLOB, "truncated blob section %s", e[k].name);
    }
    std::string name(e[k].name, strnlen(e[k].name, 24));
    if (e[k].dtype == 1) {
      std::vector<double> v(e[k].count);
      memcpy(v.data(), b + e[k].offset, 8 * (size_t)e[k].count);
      m->f[name] = v;
    } else if (e[k].dtype == 2) {
      std::vector<int> v(e[k].count);
      memcpy(v.data(), b + e[k].offset, 4 * (size_t)e[k].count);
      m->i[name] = v;
    } else {
      delete m;
      return fail(VNL_ERR_BLOB, "unknown dtype in section %s", e[k].name);
    }
  }
  static const char* need[] = {"nq", "nv", "nu", "nbody", "njnt", "ncg", "ncon", "nlimit", "nefc", "timestep",
                               "tolerance", "ls_tolerance", "impratio", "meaninertia", "iterations",
                               "ls_iterations", "eulerdamp", "solver_newton"};
  for (const char* k : need)
    if (m->scalar(k) != m->scalar(k)) {
      delete m;
      return fail(VNL_ERR_BLOB, "blob lacks scalar %s", k);
    }
  *out = m;
  return VNL_OK;
}
extern "C" void vnl_model_destroy(vnl_model* m) { delete m; }

// ----------------------------------------------------------------------------- env
struct vnl_env {
  int device = 0, B = 0;
  DevModel dm{};
  DevEnv de{};
  WsLayout L{};
  KernelConsts* kc = nullptr;  // device copy of {dm, de, L}
  vreal* dump = nullptr;  // [B][L.total] image of the per-env LDS, written only when debug is on
  int* trace = nullptr;   // [B][n_frames][VNL_TRACE_INTS] solver decisions, written only when debug is on
  // vnl_env_reset_done: where the draws of a fresh reset go when the caller asks for no record ([B] | [B] | [B][nq])
  int *rd_start = nullptr, *rd_clip = nullptr;
  vreal* rd_noise = nullptr;
  int debug = 0;          // 0 off, 1 image at the end of reset / step, 2 image after the last forward pass of a step
  int spec = 0;           // 1: the kernels specialised for the rodent's dims and layout (VnlSpecRodent) run this env
  size_t lds_bytes = 0;
  int blocks_per_cu = 0;
  // domain randomisation (vnl_env_set_domain): the model's values of the randomisable fields and what the contact rows'
  // inverse weight is derived from, kept from the upload; the per-env tables [B][ncg | ncg | nu | nv | nv] once set
  std::vector<double> mu0, gain0, damp0, arm0, cg_t;
  double impratio = 1.0;
  vreal* dom = nullptr;  // the four-field tables, then the body tables [B][nd | 3 nd | 6 nd | 1] (nd dynamic bodies)
  int has_dom = 0;  // 1: vnl_env_reset / vnl_env_step launch the randomised instantiations (csrc/vnl_domain.hip)
  int has_dom4 = 0, has_body = 0;  // which part was set (vnl_env_set_domain / vnl_env_set_body_domain); the other reads as compiled
  // vnl_env_set_domain_ranges: the device copy of the bounds ([ncg] cg_t | impratio | lo, hi of every field given), float64
  double* rng_buf = nullptr;
  int has_ranges = 0;
  // vnl_env_set_body_domain: the inertial fields of the model AS GIVEN and the fold of its welded bodies, kept from the upload
  struct FuseMap* fmap = nullptr;
  std::vector<double> mass0, ipos0, ifull0, inertia0, iquat0;  // (inertia0 / iquat0 empty: the blob does not carry them)
  std::vector<double> R_iq0;                                   // [nbody as given][9] rotation matrix of iquat0 (qmat_d), once
  std::vector<int> dyn_dofnum;                                 // dofs of every dynamic body
  std::vector<int> dyn_parent;                                 // parent of every dynamic body (the fused tree)
  // vnl_env_set_body_domain_ranges: one device buffer (bounds, what the fold needs, per-env raw fields and staging; see
  // body_ranges_layout) and the host copy of the raw fields vnl_env_set_body_domain was given ([B][n] each, empty: compiled)
  char* brng_buf = nullptr;
  int has_body_ranges = 0;
  std::vector<double> body_raw[3];
  std::vector<void*> allocs;
  std::map<std::string, std::pair<int, int>> sections;  // name -> (offset, count)
};

// makes `device` current for the scope and restores the caller's device afterwards
struct DeviceGuard {
  int prev = -1;
  bool ok = false, switched = false;
  explicit DeviceGuard(int device) {
    if (hipGetDevice(&prev) != hipSuccess) return;
    if (prev != device) {
      if (hipSetDevice(device) != hipSuccess) return;
      switched = true;
    }
    ok = true;
  }
  ~DeviceGuard() {
    if (switched) (void)hipSetDevice(prev);
  }
};

template <class T, class S>
static int upload(vnl_env* env, const std::vector<S>& src, const T** dst) {
  std::vector<T> tmp(src.begin(), src.end());
  if (tmp.empty()) tmp.push_back(T(0));
  void* p = nullptr;
  HIPCHK(hipMalloc(&p, tmp.size() * sizeof(T)));
  env->allocs.push_back(p);
  HIPCHK(hipMemcpy(p, tmp.data(), tmp.size() * sizeof(T), hipMemcpyHostToDevice));
  *dst = (const T*)p;
  return VNL_OK;
}
template <class T>
static int upload_raw(vnl_env* env, const T* src, size_t n, const T** dst) {
  std::vector<T> tmp(src, src + n);
  return upload<T, T>(env, tmp, dst);
}

// ---- welded bodies -------------------------------------------------------------------------------------------------
// A body without joints moves rigidly with its parent: for the dynamics it IS part of the parent.  The rodent has 13 such
// bodies among its 66, which is what pushed every per-body loop of the step kernel over the 64 lanes of a wave.  The model
// handed to the kernels therefore has them folded into their parents -- mass, centre of mass and inertia merged exactly
// (parallel-axis theorem in the parent's frame), children and collision geoms re-attached with composed fixed transforms --
// while every body of the model AS GIVEN keeps its row of xpos / xquat (pose of its dynamic body composed with its fixed
// transform).  The oracle works on the model as given: the parity tests check this transformation with everything else.
struct FuseMap {
  int nb_out = 0;
  std::vector<int> out_dyn, body_out;
  std::vector<double> out_pos, out_quat;
  std::vector<int> mem_start, mem;  // the members of every dynamic body, ascending (CSR): what fuse_inertial gathers over
  std::vector<double> R_out;        // [nb_out][9] the rotation matrix of out_quat
};
static void qmul_d(const double* a, const double* b, double* o) {
  o[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
  o[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  o[2] = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
  o[3] = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
}
static void qmat_d(const double* q, double* R) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  R[0] = 1 - 2 * (y * y + z * z), R[1] = 2 * (x * y - w * z), R[2] = 2 * (x * z + w * y);
  R[3] = 2 * (x * y + w * z), R[4] = 1 - 2 * (x * x + z * z), R[5] = 2 * (y * z - w * x);
  R[6] = 2 * (x * z - w * y), R[7] = 2 * (y * z + w * x), R[8] = 1 - 2 * (x * x + y * y);
}
static void mulv_d(const double* R, const double* v, double* o) {
  for (int r = 0; r < 3; r++) o[r] = R[3 * r] * v[0] + R[3 * r + 1] * v[1] + R[3 * r + 2] * v[2];
}
// The inertial part of the fold, shared by the upload and by vnl_env_set_body_domain (per env): mass / centre of mass / full
// inertia of every dynamic body with what is welded to it, from the three arrays over the bodies as given.  Moments are
// accumulated about the dynamic body's origin in its axes, then shifted back to the fused centre of mass.  A model without
// welded bodies passes through unchanged.  float64 throughout; the callers cast to vreal last.
static void fuse_inertial(const FuseMap& fmr, int nd, const double* mass, const double* ipos, const double* ifull,
                          std::vector<double>* Mo, std::vector<double>* nipo, std::vector<double>* nIo) {
  const FuseMap* fm = &fmr;
  const int nb = fm->nb_out;
  std::vector<double>&M = *Mo, &nip = *nipo, &nI = *nIo;
  if (nd == nb) {
    M.assign(mass, mass + nb), nip.assign(ipos, ipos + 3 * (size_t)nb), nI.assign(ifull, ifull + 9 * (size_t)nb);
    return;
  }
  // (csrc/vnl_inertial.h: a record per body as given, then per dynamic body the sum over its members in ascending order)
  std::vector<double> recs((size_t)VNL_FOLD_REC * nb);
  for (int b = 0; b < nb; b++)
    vnl_fold_member(&fm->R_out[9 * (size_t)b], &fm->out_pos[3 * (size_t)b], mass[b], &ipos[3 * (size_t)b], &ifull[9 * (size_t)b],
                    &recs[(size_t)VNL_FOLD_REC * b]);
  M.assign(nd, 0.0), nip.assign(3 * (size_t)nd, 0.0), nI.assign(9 * (size_t)nd, 0.0);
  for (int dyn = 0; dyn < nd; dyn++) {
    double acc[VNL_FOLD_ACC];
    vnl_fold_gather(&fm->mem[fm->mem_start[dyn]], fm->mem_start[dyn + 1] - fm->mem_start[dyn], recs.data(), acc);
    M[dyn] = acc[0];
    vnl_fold_finish(acc, &ipos[3 * (size_t)fm->body_out[dyn]], &nip[3 * (size_t)dyn], &nI[9 * (size_t)dyn]);
  }
}
// body_inertia_full [nb][9] -> body_inertia6 [nb][6]: xx yy zz xy xz yz
static std::vector<double> pack_inertia6(const std::vector<double>& f9) {
  const size_t nb = f9.size() / 9;
  std::vector<double> i6(6 * nb);
  for (size_t b = 0; b < nb; b++) vnl_pack_inertia6(&f9[9 * b], &i6[6 * b]);
  return i6;
}
static double total_mass_inv_of(const std::vector<double>& mass) { return vnl_total_mass_inv(mass.data(), (int)mass.size()); }
static bool fuse_welded_bodies(const vnl_model& in, vnl_model* out, FuseMap* fm) {
  const int nb = (int)in.scalar("nbody");
  const auto& bp = in.i.at("body_parentid");
  const auto& jn = in.i.at("body_jntnum");
  std::vector<char> keep(nb, 1);
  int nd = 0;
  for (int b = 0; b < nb; b++) {
    keep[b] = (b < 2 || jn[b] > 0) ? 1 : 0;
    // (a jointless body hanging off the world -- directly or through other jointless bodies -- is NOT folded: such a model is
    // not a single tree rooted at body 1 and is rejected below, as it always was)
    if (!keep[b]) {
      int a = bp[b];
      while (a > 1 && !keep[a]) a = bp[a];
      if (a == 0) keep[b] = 1;
    }
    nd += keep[b];
  }
  fm->nb_out = nb;
  fm->out_dyn.assign(nb, 0), fm->out_pos.assign(3 * (size_t)nb, 0.0), fm->out_quat.assign(4 * (size_t)nb, 0.0);
  fm->body_out.clear();
  const auto& bpos = in.f.at("body_pos");
  const auto& bquat = in.f.at("body_quat");
  for (int b = 0, k = 0; b < nb; b++) {  // fixed transform of every body in the frame of the dynamic body it rides on
    double* fp = &fm->out_pos[3 * (size_t)b];
    double* fq = &fm->out_quat[4 * (size_t)b];
    if (keep[b]) {
      fm->out_dyn[b] = k++, fm->body_out.push_back(b);
      fq[0] = 1.0;
    } else {
      const int p = bp[b];
      fm->out_dyn[b] = fm->out_dyn[p];
      double R[9], t[3];
      qmat_d(&fm->out_quat[4 * (size_t)p], R), mulv_d(R, &bpos[3 * (size_t)b], t);
      for (int c = 0; c < 3; c++) fp[c] = fm->out_pos[3 * (size_t)p + c] + t[c];
      qmul_d(&fm->out_quat[4 * (size_t)p], &bquat[4 * (size_t)b], fq);
    }
  }
  fm->R_out.assign(9 * (size_t)nb, 0.0), fm->mem_start.assign((size_t)nd + 1, 0), fm->mem.assign(nb, 0);
  for (int b = 0; b < nb; b++) qmat_d(&fm->out_quat[4 * (size_t)b], &fm->R_out[9 * (size_t)b]), fm->mem_start[fm->out_dyn[b] + 1]++;
  for (int k = 0; k < nd; k++) fm->mem_start[k + 1] += fm->mem_start[k];
  {
    std::vector<int> at(fm->mem_start.begin(), fm->mem_start.end() - 1);
    for (int b = 0; b < nb; b++) fm->mem[at[fm->out_dyn[b]]++] = b;
  }
  if (nd == nb) return false;
  *out = in;
  out->f["nbody"] = {(double)nd};
  auto pick_i = [&](const char* k) {
    std::vector<int> v;
    for (int b = 0; b < nb; b++)
      if (keep[b]) v.push_back(in.i.at(k)[b]);
    out->i[k] = v;
  };
  auto pick_f = [&](const char* k, int w) {
    std::vector<double> v;
    for (int b = 0; b < nb; b++)
      if (keep[b]) v.insert(v.end(), in.f.at(k).begin() + (size_t)w * b, in.f.at(k).begin() + (size_t)w * (b + 1));
    out->f[k] = v;
  };
  pick_i("body_jntadr"), pick_i("body_jntnum"), pick_i("body_rootid"), pick_i("body_dofadr"), pick_i("body_dofnum");
  pick_f("body_invweight0", 2);
  std::vector<int> par;
  std::vector<double> pos, quat;
  for (int b = 0; b < nb; b++) {
    if (!keep[b]) continue;
    const int p = b > 0 ? bp[b] : 0;
    par.push_back(fm->out_dyn[p]);
    double R[9], t[3], q[4];
    qmat_d(&fm->out_quat[4 * (size_t)p], R), mulv_d(R, &bpos[3 * (size_t)b], t);
    for (int c = 0; c < 3; c++) pos.push_back(fm->out_pos[3 * (size_t)p + c] + t[c]);
    qmul_d(&fm->out_quat[4 * (size_t)p], &bquat[4 * (size_t)b], q);
    quat.insert(quat.end(), q, q + 4);
  }
  out->i["body_parentid"] = par, out->f["body_pos"] = pos, out->f["body_quat"] = quat;
  std::vector<double> M, nip, nI;
  fuse_inertial(*fm, nd, in.f.at("body_mass").data(), in.f.at("body_ipos").data(), in.f.at("body_inertia_full").data(), &M, &nip, &nI);
  out->f["body_mass"] = M, out->f["body_ipos"] = nip, out->f["body_inertia_full"] = nI;
  for (const char* k : {"jnt_bodyid", "dof_bodyid"}) {
    std::vector<int> v = in.i.at(k);
    for (int& x : v) x = fm->out_dyn[x];
    out->i[k] = v;
  }
  {  // collision geoms: onto the dynamic body, frames composed; the contact's inverse weight stays that of the body as given
    const auto& gb = in.i.at("cg_bodyid");
    const auto& gp = in.f.at("cg_pos");
    const auto& gq = in.f.at("cg_quat");
    const auto& iw0 = in.f.at("body_invweight0");
    std::vector<int> nb_(gb.size());
    std::vector<double> np = gp, nq = gq, giw(gb.size());
    for (size_t g = 0; g < gb.size(); g++) {
      const int ob = gb[g];
      nb_[g] = fm->out_dyn[ob], giw[g] = iw0[2 * (size_t)ob];
      double R[9], t[3];
      qmat_d(&fm->out_quat[4 * (size_t)ob], R), mulv_d(R, &gp[3 * g], t);
      for (int c = 0; c < 3; c++) np[3 * g + c] = fm->out_pos[3 * (size_t)ob + c] + t[c];
      qmul_d(&fm->out_quat[4 * (size_t)ob], &gq[4 * g], &nq[4 * g]);
    }
    out->i["cg_bodyid"] = nb_, out->f["cg_pos"] = np, out->f["cg_quat"] = nq, out->f["cg_body_invweight0"] = giw;
  }
  return true;
}

// inverse weight of a contact's rows (constraint._instantiate_contact): at upload and, per env, in vnl_env_set_domain
// (contact_invweight: vnl_types.h -- shared with the device redraw of the domain)

static VnlDims dims_of(const DevModel& d) {
  return VnlDims{d.nq, d.nv, d.nu, d.nbody, d.njnt, d.ncg, d.ncon, d.nlimit, d.nefc, d.nM, d.iterations, d.ls_iterations, d.eulerdamp,
                 d.root_free, d.max_depth, d.jump_rounds, d.fac_steps, d.fac_route, d.solver_newton, d.blk_cfg, d.path_runs, d.nbody_out};
}

// The factorisation routes of a model (vnl_types.h: VNL_ROUTE_*), chosen here once; the kernels' dispatchers only read them.
// The register-resident forms need their lane sets (nv <= 64, or <= 128 with the rows 64 .. of depth < 16: deep1), a bound on
// the depth and room for VNL_FAC_LINES scratch lines of MAXD + 4 floats; the articulated-body pair needs eulerdamp, its V
// store below cvel and its lines of 16 floats in the six dead vectors Mgrad .. tmp2.
static int choose_routes(const DevModel& d, int deep1) {
  const WsLayout L = vnl_make_layout(dims_of(d));  // (the layout does not depend on the routes)
  const int nv = d.nv, md = d.max_depth, set1 = VNL_ROWSETS_1 * VNL_LANES, set2 = VNL_ROWSETS_2 * VNL_LANES;
  auto rows = [&](int room) {  // room: floats for the scratch lines (-1: none needed, the inversion)
    auto fits = [&](int maxd) { return room < 0 || VNL_FAC_LINES * (maxd + 4) <= room; };
    if (nv <= set1 && md < 16 && fits(16)) return VNL_ROUTE_ROWS16;
    if (nv <= set1 && md < 36 && fits(36)) return VNL_ROUTE_ROWS36;
    if (nv <= set2 && md < 36 && deep1 < 16 && fits(36)) return VNL_ROUTE_ROWS36X2;
    return VNL_ROUTE_LDS;
  };
  const int factor = rows(4 * nv - 3);  // qM: the lines in Ma .. search, from the first 16-byte boundary
  const int inverse = rows(-1);
  const int hessian = d.solver_newton ? rows(L.smooth - ((L.P + 3 * d.nefc + 3) & ~3)) : 0;  // the lines in the pool
  const bool pair = d.eulerdamp && nv <= set2 && vnl_vstore(L.P) + 12 * nv <= vnl_cvel_at(L.P, L.smooth, d.nbody, nv) &&
                    VNL_FAC_LINES * 16 + 3 <= 6 * nv;
  return factor << VNL_ROUTE_QM_FACTOR | inverse << VNL_ROUTE_QM_INVERSE | hessian << VNL_ROUTE_HESSIAN |
         (pair ? (nv <= set1 ? 1 : 2) : 0) << VNL_ROUTE_PAIR;
}

static int build_dev_model(vnl_env* env, const vnl_model* hm) {
  DevModel& d = env->dm;
  vnl_model fused;
  FuseMap fmap;
  for (const char* k : {"body_parentid", "body_jntnum"})
    if (hm->i.find(k) == hm->i.end()) return fail(VNL_ERR_BLOB, "blob section %s missing", k);
  for (const char* k : {"body_pos", "body_quat", "body_ipos", "body_inertia_full", "body_mass", "body_invweight0", "cg_pos", "cg_quat"})
    if (hm->f.find(k) == hm->f.end()) return fail(VNL_ERR_BLOB, "blob section %s missing", k);
  for (const char* k : {"jnt_bodyid", "dof_bodyid", "cg_bodyid", "body_jntadr", "body_rootid", "body_dofadr", "body_dofnum"})
    if (hm->i.find(k) == hm->i.end()) return fail(VNL_ERR_BLOB, "blob section %s missing", k);
  {  // kept for vnl_env_set_body_domain: the inertial fields as given (the fold below replaces them in `fused`)
    env->mass0 = hm->f.at("body_mass"), env->ipos0 = hm->f.at("body_ipos"), env->ifull0 = hm->f.at("body_inertia_full");
    const size_t nbo = env->mass0.size();
    if (env->ipos0.size() != 3 * nbo || env->ifull0.size() != 9 * nbo || (double)nbo != hm->scalar("nbody"))
      return fail(VNL_ERR_BLOB, "blob section %s missing or of unexpected size", "body_ipos / body_inertia_full");
    if (hm->has_f("body_inertia", 3 * nbo) && hm->has_f("body_iquat", 4 * nbo))
      env->inertia0 = hm->f.at("body_inertia"), env->iquat0 = hm->f.at("body_iquat");
    env->R_iq0.assign(env->iquat0.empty() ? 0 : 9 * nbo, 0.0);
    for (size_t b = 0; b < env->R_iq0.size() / 9; b++) qmat_d(&env->iquat0[4 * b], &env->R_iq0[9 * b]);
  }
  if (fuse_welded_bodies(*hm, &fused, &fmap)) hm = &fused;
  d.nbody_out = fmap.nb_out;
  env->fmap = new FuseMap(fmap);
  env->dyn_dofnum = hm->i.at("body_dofnum");
  env->dyn_parent = hm->i.at("body_parentid");
  auto S = [&](const char* k) { return hm->scalar(k); };
  d.nq = (int)S("nq"), d.nv = (int)S("nv"), d.nu = (int)S("nu"), d.nbody = (int)S("nbody"), d.njnt = (int)S("njnt");
  d.ncg = (int)S("ncg"), d.ncon = (int)S("ncon"), d.nlimit = (int)S("nlimit"), d.nefc = (int)S("nefc");
  d.iterations = (int)S("iterations"), d.ls_iterations = (int)S("ls_iterations"), d.eulerdamp = (int)S("eulerdamp");
  d.dt = (vreal)S("timestep"), d.tolerance = (vreal)S("tolerance"), d.ls_tolerance = (vreal)S("ls_tolerance");
  // Newton (reference configs/env_config.yaml:16-21): the Hessian M + J' D J is formed and factorised in qM's tree-sparse layout
  // (the checks at the end of this function refuse a model that does not admit it)
  d.solver_newton = S("solver_newton") != 0;
  d.dbg_stage = 0, d.dbg_count = 0;
#ifdef VNL_STAGE_KNOBS  // diagnostic library only: the product library reads no environment variables
  if (const char* dbg = getenv("VNL_DBG_REPEAT")) sscanf(dbg, "%d:%d", &d.dbg_stage, &d.dbg_count);
#endif
  d.scale = (vreal)(S("meaninertia") * (d.nv > 1 ? d.nv : 1));
  const int nb = d.nbody, nj = d.njnt, nv = d.nv, nu = d.nu, ng = d.ncg;
  std::vector<int> nsub_host, limrow_host;  // kept for the per-dof contact ranges further down
  struct Need {
    const char* k;
    size_t n;
    bool isint;
  } needs[] = {{"body_parentid", (size_t)nb, true}, {"body_jntadr", (size_t)nb, true}, {"body_jntnum", (size_t)nb, true},
               {"body_rootid", (size_t)nb, true}, {"body_dofadr", (size_t)nb, true}, {"body_dofnum", (size_t)nb, true}, {"body_pos", 3u * nb, false}, {"body_quat", 4u * nb, false},
               {"body_ipos", 3u * nb, false}, {"body_inertia_full", 9u * nb, false}, {"body_mass", (size_t)nb, false},
               {"body_invweight0", 2u * nb, false}, {"jnt_type", (size_t)nj, true}, {"jnt_qposadr", (size_t)nj, true},
               {"jnt_dofadr", (size_t)nj, true}, {"jnt_bodyid", (size_t)nj, true}, {"jnt_limited", (size_t)nj, true}, {"jnt_pos", 3u * nj, false},
               {"jnt_axis", 3u * nj, false}, {"jnt_range", 2u * nj, false}, {"jnt_stiffness", (size_t)nj, false},
               {"jnt_margin", (size_t)nj, false}, {"jnt_solref", 2u * nj, false}, {"jnt_solimp", 5u * nj, false},
               {"qpos0", (size_t)d.nq, false}, {"qpos_spring", (size_t)d.nq, false}, {"dof_bodyid", (size_t)nv, true},
               {"dof_parentid", (size_t)nv, true}, {"dof_armature", (size_t)nv, false},
               {"dof_damping", (size_t)nv, false}, {"dof_invweight0", (size_t)nv, false}, {"act_dof", (size_t)nu, true},
               {"act_ctrllimited", (size_t)nu, true}, {"act_gain", (size_t)nu, false}, {"act_gear", (size_t)nu, false},
               {"act_tau", (size_t)nu, false}, {"act_ctrlrange", 2u * nu, false}, {"cg_type", (size_t)ng, true},
               {"cg_bodyid", (size_t)ng, true}, {"cg_ncon", (size_t)ng, true}, {"cg_conadr", (size_t)ng, true},
               {"cg_pos", 3u * ng, false}, {"cg_quat", 4u * ng, false}, {"cg_size", 3u * ng, false},
               {"cg_friction", 3u * ng, false}, {"cg_solref", 2u * ng, false}, {"cg_solimp", 5u * ng, false},
               {"cg_margin", (size_t)ng, false}, {"gravity", 3, false}, {"plane_pos", 3, false},
               {"plane_normal", 3, false}};
  for (auto& n : needs)
    if (!(n.isint ? hm->has_i(n.k, n.n) : hm->has_f(n.k, n.n)))
      return fail(VNL_ERR_BLOB, "blob section %s missing or of unexpected size", n.k);
  auto F = [&](const char* k) -> const std::vector<double>& { return hm->f.at(k); };
  auto I = [&](const char* k) -> const std::vector<int>& { return hm->i.at(k); };

  // single kinematic tree rooted at body 1 (the spatial reference point is its origin)
  for (int b = 1; b < nb; b++)
    if (I("body_rootid")[b] != 1) return fail(VNL_ERR_UNSUPPORTED, "model must be a single tree rooted at body 1");
  const auto& jt = I("jnt_type");
  for (int j = 0; j < nj; j++)
    if (jt[j] != VNL_JNT_FREE && jt[j] != VNL_JNT_HINGE)
      return fail(VNL_ERR_UNSUPPORTED, "only free and hinge joints are implemented");
  d.root_free = (I("body_jntnum")[1] > 0 && jt[I("body_jntadr")[1]] == VNL_JNT_FREE) ? 1 : 0;
  d.root_px = (vreal)F("body_pos")[3], d.root_py = (vreal)F("body_pos")[4], d.root_pz = (vreal)F("body_pos")[5];
  d.gx = (vreal)F("gravity")[0], d.gy = (vreal)F("gravity")[1], d.gz = (vreal)F("gravity")[2];
  const auto& pn = F("plane_normal");
  const auto& pp = F("plane_pos");
  d.pnx = (vreal)pn[0], d.pny = (vreal)pn[1], d.pnz = (vreal)pn[2];
  d.ppx = (vreal)pp[0], d.ppy = (vreal)pp[1], d.ppz = (vreal)pp[2];
  {  // math.make_frame(n)[1]
    double a[3] = {pn[0], pn[1], pn[2]}, bb[3] = {0, 0, 0};
    if (-0.5 < a[1] && a[1] < 0.5) bb[1] = 1; else bb[2] = 1;
    double ab = a[0] * bb[0] + a[1] * bb[1] + a[2] * bb[2];
    for (int k = 0; k < 3; k++) bb[k] -= a[k] * ab;
    double nn = sqrt(bb[0] * bb[0] + bb[1] * bb[1] + bb[2] * bb[2]);
    d.t1x = (vreal)(bb[0] / nn), d.t1y = (vreal)(bb[1] / nn), d.t1z = (vreal)(bb[2] / nn);
  }
  d.total_mass_inv = (vreal)total_mass_inv_of(F("body_mass"));

  int rc;
#define UPF(name, vec) if ((rc = upload<vreal, double>(env, vec, &d.name)) != VNL_OK) return rc;
#define UPI(name, vec) if ((rc = upload<int, int>(env, vec, &d.name)) != VNL_OK) return rc;
  UPI(body_parent, I("body_parentid")) UPI(body_jntadr, I("body_jntadr")) UPI(body_jntnum, I("body_jntnum"))
  UPI(out_dyn, fmap.out_dyn) UPI(body_out, fmap.body_out) UPF(out_pos, fmap.out_pos) UPF(out_quat, fmap.out_quat)
  {
    std::vector<int> da(nb, 0), dn(nb, 0);
    for (int b = 0; b < nb; b++) {
      dn[b] = I("body_dofnum")[b];
      da[b] = dn[b] > 0 ? I("body_dofadr")[b] : 0;
    }
    UPI(body_dofadr, da) UPI(body_dofnum, dn)
    // subtree sizes (bodies are numbered depth-first: subtree(b) = b .. b + nsub[b]) and the
    // pointer-jumping tables jump[r][b] = 2^r-th ancestor of b (0 when it would be the world body)
    const auto& bp = I("body_parentid");
    std::vector<int> nsub(nb, 0);
    for (int b = nb - 1; b > 0; b--) nsub[bp[b]] += nsub[b] + 1;
    for (int b = 1; b < nb; b++)
      for (int c = b + 1; c <= b + nsub[b]; c++) {
        bool in = false;
        for (int a = c; a > 0; a = bp[a]) in |= (a == b);
        if (!in) return fail(VNL_ERR_UNSUPPORTED, "body numbering is not depth-first");
      }
    UPI(body_nsub, nsub)
    nsub_host = nsub;
    std::vector<int> lastdof(nb, nv);  // last dof on the path from the root to (and including) body b; nv = none
    for (int b = 1; b < nb; b++) lastdof[b] = dn[b] > 0 ? da[b] + dn[b] - 1 : lastdof[bp[b]];
    UPI(body_lastdof, lastdof)
    // The dofs on the path root -> body b as (at most 4) runs of consecutive dof indices, begin | end << 8 each:
    // jac_mul sums a body twist as differences of ONE prefix-sum array over the dofs instead of walking the path.
    {
      const auto& dpar = I("dof_parentid");
      std::vector<int> seg(8 * (size_t)nb, 0);  // per body: 4 runs of dofs, then 4 runs of ancestor bodies (incl. itself)
      int most = 1;
      for (int b = 1; b < nb; b++) {
        {
          std::vector<int> anc;
          for (int a = b; a > 0; a = bp[a]) anc.push_back(a);
          std::sort(anc.begin(), anc.end());
          int nseg = 0;
          for (size_t i = 0; i < anc.size();) {
            size_t j = i;
            while (j + 1 < anc.size() && anc[j + 1] == anc[j] + 1) j++;
            if (nseg == 4) return fail(VNL_ERR_UNSUPPORTED, "a body has more than 4 runs of consecutive ancestor bodies");
            seg[8 * b + 4 + nseg++] = anc[i] | ((anc[j] + 1) << 8);
            i = j + 1;
          }
          most = nseg > most ? nseg : most;
        }
        std::vector<int> path;
        for (int dd = lastdof[b] < nv ? lastdof[b] : -1; dd >= 0; dd = dpar[dd]) path.push_back(dd);
        std::sort(path.begin(), path.end());
        int nseg = 0;
        for (size_t i = 0; i < path.size();) {
          size_t j = i;
          while (j + 1 < path.size() && path[j + 1] == path[j] + 1) j++;
          if (nseg == 4) return fail(VNL_ERR_UNSUPPORTED, "a body path has more than 4 runs of consecutive dofs");
          seg[8 * b + nseg++] = path[i] | ((path[j] + 1) << 8);
          i = j + 1;
        }
        most = nseg > most ? nseg : most;
      }
      d.path_runs = most;
      UPI(body_pathseg, seg)
    }
    int bdepth = 0;
    for (int b = 1; b < nb; b++) {
      int dd = 0;
      for (int a = b; a > 0; a = bp[a]) dd++;
      bdepth = dd > bdepth ? dd : bdepth;
    }
    int rounds = 0;
    while ((1 << rounds) < bdepth) rounds++;
    d.jump_rounds = rounds;
    std::vector<unsigned char> jump((size_t)(rounds > 0 ? rounds : 1) * nb, 0);
    for (int b = 0; b < nb; b++) jump[b] = (unsigned char)bp[b];
    for (int r = 1; r < rounds; r++)
      for (int b = 0; b < nb; b++) jump[(size_t)r * nb + b] = jump[(size_t)(r - 1) * nb + jump[(size_t)(r - 1) * nb + b]];
    {
      const unsigned char* dp = nullptr;
      if ((rc = upload<unsigned char, unsigned char>(env, jump, &dp)) != VNL_OK) return rc;
      d.jump = dp;
    }
  }
  UPF(body_pos, F("body_pos")) UPF(body_quat, F("body_quat")) UPF(body_ipos, F("body_ipos")) UPF(body_mass, F("body_mass"))
  UPF(body_inertia6, pack_inertia6(F("body_inertia_full")))
  UPI(jnt_type, jt) UPI(jnt_qposadr, I("jnt_qposadr")) UPI(jnt_dofadr, I("jnt_dofadr")) UPI(jnt_body, I("jnt_bodyid"))
  UPF(jnt_pos, F("jnt_pos")) UPF(jnt_axis, F("jnt_axis")) UPF(jnt_stiffness, F("jnt_stiffness"))
  {
    std::vector<double> q0(nj), qs(nj);
    for (int j = 0; j < nj; j++) q0[j] = F("qpos0")[I("jnt_qposadr")[j]], qs[j] = F("qpos_spring")[I("jnt_qposadr")[j]];
    UPF(jnt_qpos0, q0) UPF(jnt_springref, qs)
  }
  {  // limit rows
    std::vector<int> qa, dof;
    std::vector<double> lo, hi, mg, iw, sr, si;
    for (int j = 0; j < nj; j++) {
      if (!I("jnt_limited")[j] || jt[j] != VNL_JNT_HINGE) continue;
      qa.push_back(I("jnt_qposadr")[j]), dof.push_back(I("jnt_dofadr")[j]);
      lo.push_back(F("jnt_range")[2 * j]), hi.push_back(F("jnt_range")[2 * j + 1]), mg.push_back(F("jnt_margin")[j]);
      iw.push_back(F("dof_invweight0")[I("jnt_dofadr")[j]]);
      for (int k = 0; k < 2; k++) sr.push_back(F("jnt_solref")[2 * j + k]);
      for (int k = 0; k < 5; k++) si.push_back(F("jnt_solimp")[5 * j + k]);
    }
    if ((int)qa.size() != d.nlimit) return fail(VNL_ERR_BLOB, "nlimit does not match jnt_limited");
    UPI(lim_qadr, qa) UPI(lim_dof, dof) UPF(lim_lo, lo) UPF(lim_hi, hi) UPF(lim_margin, mg) UPF(lim_invweight, iw)
    UPF(lim_solref, sr) UPF(lim_solimp, si)
  }
  {  // tree-sparse layout of qM (MuJoCo dof_Madr order: self, parent, grandparent, ...)
    const auto& par = I("dof_parentid");
    std::vector<int> madr(nv), depth(nv), anc;
    for (int i = 0; i < nv; i++) {
      madr[i] = (int)anc.size();
      int dep = 0;
      for (int j = i; j >= 0; j = par[j]) anc.push_back(j), dep++;
      depth[i] = dep - 1;
    }
    d.nM = (int)anc.size();
    std::vector<int> row(anc.size());
    for (int i = 0; i < nv; i++)
      for (int a = 0; a <= depth[i]; a++) row[madr[i] + a] = i;
    // descendants of a dof are the next ndesc dofs (DFS numbering); checked here because col_apply relies on it
    std::vector<int> ndesc(nv, 0);
    for (int i = 0; i < nv; i++)
      for (int j = par[i]; j >= 0; j = par[j]) ndesc[j]++;
    for (int a = 0; a < nv; a++)
      for (int i = a + 1; i <= a + ndesc[a]; i++) {
        bool is_desc = false;
        for (int j = par[i]; j >= 0; j = par[j]) is_desc |= (j == a);
        if (!is_desc) return fail(VNL_ERR_UNSUPPORTED, "dof numbering is not depth-first");
      }
    int maxd = 0;
    for (int i = 0; i < nv; i++) maxd = depth[i] > maxd ? depth[i] : maxd;
    d.max_depth = maxd;
    if (nv > 255 || nb > 255 || maxd > 62) return fail(VNL_ERR_UNSUPPORTED, "model too large for 8-bit index tables");
    std::vector<unsigned char> lvl_tab;  // dofs sorted by depth, then the level start offsets
    std::vector<int> lvl_start(maxd + 2, 0);
    for (int lev = 0; lev <= maxd; lev++) {
      lvl_start[lev] = (int)lvl_tab.size();
      int cnt = 0;
      for (int i = 0; i < nv; i++)
        if (depth[i] == lev) lvl_tab.push_back((unsigned char)i), cnt++;
      if (cnt * lev > 2 * nv) return fail(VNL_ERR_UNSUPPORTED, "tree level too wide for the inversion staging buffer");
    }
    lvl_start[maxd + 1] = (int)lvl_tab.size();
    for (int v : lvl_start) lvl_tab.push_back((unsigned char)v);
    {
      const unsigned char* dp = nullptr;
      if ((rc = upload<unsigned char, unsigned char>(env, lvl_tab, &dp)) != VNL_OK) return rc;
      d.lvl_tab = dp;
    }
    std::vector<int> limrow(nv, -1);
    {
      int r = 0;
      for (int j = 0; j < nj; j++)
        if (I("jnt_limited")[j] && jt[j] == VNL_JNT_HINGE) limrow[I("jnt_dofadr")[j]] = r++;
    }
    UPI(dof_body, I("dof_bodyid")) UPI(dof_Madr, madr) UPI(dof_depth, depth) UPI(M_anc, anc) UPI(M_row, row)
    UPI(dof_ndesc, ndesc)
    limrow_host = limrow;
    // Factorisation schedule: row j can be the pivot once all its descendants have been; rows whose
    // subtrees are disjoint go in the same step (at most VNL_FAC_LINES of them, one scratch line each).
    std::vector<int> ftime(nv, 0), fslot(nv, 0), count;
    for (int j = nv - 1; j >= 0; j--) {  // children have larger indices: their times are final here
      int t = 0;
      for (int i = j + 1; i <= j + ndesc[j]; i++)
        if (par[i] == j) t = ftime[i] + 1 > t ? ftime[i] + 1 : t;
      while ((int)count.size() <= t) count.push_back(0);
      while (count[t] >= VNL_FAC_LINES) {
        t++;
        if ((int)count.size() <= t) count.push_back(0);
      }
      ftime[j] = t, fslot[j] = count[t]++;
    }
    // a parent must come strictly after each child even when the child was pushed to a later step
    for (int j = nv - 1; j >= 0; j--)
      if (par[j] >= 0 && ftime[par[j]] <= ftime[j]) return fail(VNL_ERR_UNSUPPORTED, "factorisation schedule is not causal");
    d.fac_steps = (int)count.size();
    UPI(dof_ftime, ftime) UPI(dof_fslot, fslot)
    {
      int deep1 = 0;  // the deepest of the rows 64 .. (the second lane set)
      for (int j = 64; j < nv; j++) deep1 = depth[j] > deep1 ? depth[j] : deep1;
      d.fac_route = choose_routes(d, deep1);
    }
    {  // guests of invert_aba: rows 64.. placed with lanes whose own row is shallow (deepest guests first), so that own + guest <= 36 entries
      d.fac_guest = nullptr;
      if (nv > 64 && nv <= 128) {
        std::vector<int> guest(64, -1), order;
        for (int j = 64; j < nv; j++) order.push_back(j);
        std::sort(order.begin(), order.end(), [&](int x, int y) { return depth[x] > depth[y]; });
        bool ok = true;
        for (int j : order) {
          int host = -1;
          for (int l = 0; l < 64 && host < 0; l++)
            if (guest[l] < 0 && depth[l] <= 12) host = l;
          if (host < 0 || depth[j] > 24) ok = false;
          else guest[host] = j;
        }
        if (ok) UPI(fac_guest, guest)
      }
    }
    {  // fac_match[a][t]: the scratch lines whose pivot of step t lies strictly below row a (factor_aba absorbs them)
      // (rows padded to whole 32-bit words, four steps each: the kernel loads a row's schedule by the word)
      const int nst = vnl_fac_stride(d.fac_steps);
      std::vector<unsigned char> match((size_t)nv * (nst > 0 ? nst : 4), 0);
      for (int j = 0; j < nv; j++)
        for (int a = par[j]; a >= 0; a = par[a]) match[(size_t)a * nst + ftime[j]] |= (unsigned char)(1u << fslot[j]);
      const unsigned char* dp = nullptr;
      if ((rc = upload<unsigned char, unsigned char>(env, match, &dp)) != VNL_OK) return rc;
      d.fac_match = dp;
    }
    {  // EnvWave::blk_apply: the sparse products with the factor / its inverse cut into blocks of <= 8 entries of ONE row (or
       // column), dealt out so that every lane has about the same number -- the rows of a tree are as long as the dofs are deep
       // (0 .. 35 for the rodent) and its columns as long as the subtrees are large (0 .. 72): a lane per row / column
       // makes the wave wait for the longest.  The blocks of a row sit in adjacent lanes of one 16-lane DPP row (their partial
       // sums are combined by shifts), `trips` x 64 descriptors per form:
       //   bits 0-15 payload (row form: index of the block's first entry; column form: first descendant | depth of the column << 7)
       //   16-19 entries in the block | 20-26 row / column | 27 first block of its row | 28-31 lane + 1, 2, 4, 8 continues the row
      d.blk_tab = nullptr, d.blk_cfg = 0;
      auto pack = [&](bool colform, std::vector<unsigned>& out, int& trips, int& steps) -> bool {
        struct Item { int r, nblk; };
        std::vector<Item> items;
        int total = 0, longest = 1;
        for (int r = 0; r < nv; r++) {
          const int len = colform ? ndesc[r] : depth[r], nb_ = len > 0 ? (len + VNL_BLK_W - 1) / VNL_BLK_W : 1;
          if (nb_ > 16) return false;
          items.push_back({r, nb_}), total += nb_, longest = nb_ > longest ? nb_ : longest;
        }
        std::stable_sort(items.begin(), items.end(), [](const Item& a, const Item& b) { return a.nblk > b.nblk; });
        steps = longest > 8 ? 4 : (longest > 4 ? 3 : (longest > 2 ? 2 : (longest > 1 ? 1 : 0)));
        for (trips = (total + 63) / 64; trips <= 8; trips++) {
          std::vector<int> fill(trips * 4, 0);
          std::vector<unsigned> tab((size_t)trips * 64, 0u);
          bool ok = true;
          for (const Item& it : items) {
            int bin = -1;
            for (int b = 0; b < trips * 4 && bin < 0; b++)
              if (fill[b] + it.nblk <= 16) bin = b;
            if (bin < 0) { ok = false; break; }
            const int len = colform ? ndesc[it.r] : depth[it.r];
            for (int k = 0; k < it.nblk; k++) {
              const int slot = bin * 16 + fill[bin] + k, left = it.nblk - 1 - k;  // blocks of the row after this one
              const int n = len - VNL_BLK_W * k > VNL_BLK_W ? VNL_BLK_W : (len - VNL_BLK_W * k > 0 ? len - VNL_BLK_W * k : 0);
              unsigned payload;
              if (colform) payload = (unsigned)(n > 0 ? it.r + 1 + VNL_BLK_W * k : it.r) | ((unsigned)depth[it.r] << 7);
              else payload = (unsigned)(madr[it.r] + (n > 0 ? 1 + VNL_BLK_W * k : 0));
              unsigned mask = 0;
              for (int b = 0; b < 4; b++)
                if ((1 << b) <= left) mask |= 1u << b;
              tab[slot] = payload | ((unsigned)n << 16) | ((unsigned)it.r << 20) | ((k == 0 ? 1u : 0u) << 27) | (mask << 28);
            }
            fill[bin] += it.nblk;
          }
          if (ok) {
            out = tab;
            return true;
          }
        }
        return false;
      };
      std::vector<unsigned> rowtab, coltab;
      int tr = 0, tc = 0, sr = 0, sc = 0;
      if (nv <= 127 && maxd <= 63 && d.nM < 65536 && pack(false, rowtab, tr, sr) && pack(true, coltab, tc, sc)) {
        rowtab.insert(rowtab.end(), coltab.begin(), coltab.end());
        const unsigned* dp = nullptr;
        if ((rc = upload<unsigned, unsigned>(env, rowtab, &dp)) != VNL_OK) return rc;
        d.blk_tab = dp;
        d.blk_cfg = tr | (tc << 4) | (sr << 8) | (sc << 12);
      }
    }
  }
  UPF(dof_armature, F("dof_armature")) UPF(dof_damping, F("dof_damping"))
  UPI(act_dof, I("act_dof")) UPI(act_limited, I("act_ctrllimited")) UPF(act_gain, F("act_gain"))
  {  // per dof: the actuators that drive it (smooth_forces gathers instead of walking all actuators per dof)
    std::vector<int> packed(nv, 0), cnt(nv, 0);
    bool ok = nu < 255;
    for (int a = 0; a < nu && ok; a++) {
      const int dd = I("act_dof")[a];
      if (dd < 0 || dd >= nv) continue;
      if (cnt[dd] == 4) ok = false;
      else packed[dd] |= (a + 1) << (8 * cnt[dd]++);
    }
    d.dof_act = nullptr;
    if (ok) UPI(dof_act, packed)
  }
  UPF(act_tau, F("act_tau")) UPF(act_gear, F("act_gear"))
  {
    std::vector<double> lo(nu), hi(nu);
    for (int k = 0; k < nu; k++) lo[k] = F("act_ctrlrange")[2 * k], hi[k] = F("act_ctrlrange")[2 * k + 1];
    UPF(act_lo, lo) UPF(act_hi, hi)
  }
  UPI(cg_type, I("cg_type")) UPI(cg_body, I("cg_bodyid")) UPI(cg_conadr, I("cg_conadr")) UPI(cg_ncon, I("cg_ncon"))
  {
    std::vector<int> cgeom(d.ncon, 0);
    for (int g = 0; g < ng; g++)
      for (int q = 0; q < I("cg_ncon")[g]; q++) cgeom[I("cg_conadr")[g] + q] = g;
    // The contacts under a dof (subtree of its body = contiguous body range) form ONE range [c0, c1) of the
    // contacts SORTED BY BODY: con_geom[k] carries the geom of contact k in its low byte and, in the next byte, the
    // k-th contact in body order; the range is packed next to the dof's limit row as
    // (limrow + 1) | c0 << 10 | c1 << 18 | valid << 26 (constraint_force sums wrenches by prefix differences).
    const auto& cgb = I("cg_bodyid");
    const bool ok_ = d.ncon <= 64 && d.nlimit < 1023 && ng < 256;
    if (!ok_) return fail(VNL_ERR_UNSUPPORTED, "more than 64 contacts / 255 collision geoms / 1022 limit rows (constraint_force scans the contact wrenches in one wave)");
    std::vector<int> order(d.ncon);
    for (int c = 0; c < d.ncon; c++) order[c] = c;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return cgb[cgeom[a]] < cgb[cgeom[b]]; });
    if (ok_)
      for (int k = 0; k < d.ncon; k++) cgeom[k] |= order[k] << 8;
    UPI(con_geom, cgeom)
    std::vector<int> packed(nv);
    for (int dd = 0; dd < nv; dd++) {
      int b0 = I("dof_bodyid")[dd], b1 = b0 + nsub_host[b0], c0 = 0, c1 = 0;
      while (c0 < d.ncon && cgb[cgeom[order[c0]] & 0xff] < b0) c0++;
      c1 = c0;
      while (c1 < d.ncon && cgb[cgeom[order[c1]] & 0xff] <= b1) c1++;
      packed[dd] = (limrow_host[dd] + 1) | (c0 << 10) | (c1 << 18) | ((ok_ ? 1 : 0) << 26);
    }
    UPI(dof_limrow, packed)
  }
  UPF(cg_pos, F("cg_pos")) UPF(cg_quat, F("cg_quat")) UPF(cg_size, F("cg_size")) UPF(cg_solref, F("cg_solref"))
  UPF(cg_solimp, F("cg_solimp")) UPF(cg_margin, F("cg_margin"))
  {
    std::vector<double> mu(ng), iw(ng);
    double impratio = S("impratio");
    env->cg_t.assign(ng, 0.0);
    for (int g = 0; g < ng; g++) {
      mu[g] = F("cg_friction")[3 * g];
      double t = F("body_invweight0")[0] + (hm->f.count("cg_body_invweight0") ? F("cg_body_invweight0")[g]
                                                                                : F("body_invweight0")[2 * (size_t)I("cg_bodyid")[g]]);
      iw[g] = contact_invweight(t, mu[g], impratio);
      env->cg_t[g] = t;
    }
    UPF(cg_mu, mu) UPF(cg_invweight, iw)
    env->impratio = impratio, env->mu0 = mu;
    env->gain0 = F("act_gain"), env->damp0 = F("dof_damping"), env->arm0 = F("dof_armature");
  }
#undef UPF
#undef UPI
  if (d.solver_newton) {
    // The Newton solver's tree-sparse Hessian (EnvWaveT::newton_hessian) relies on every constraint row's Jacobian living on ONE
    // body's path to the root: a limit row on the single dof of its hinge (one limit row per dof: dof_limrow holds one), a
    // contact's rows on the path of the one dynamic body whose geom touches the plane.  Its factor is inverted in registers
    // (EnvWaveT::invert_factor: the LDS form works on qM's place only).
    std::vector<int> nlim(nv, 0);
    for (int j = 0; j < nj; j++)
      if (I("jnt_limited")[j] && I("jnt_type")[j] == VNL_JNT_HINGE) {
        const int dd = I("jnt_dofadr")[j];
        if (dd < 0 || dd >= nv || ++nlim[dd] > 1)
          return fail(VNL_ERR_UNSUPPORTED, "Newton solver: a limit row does not act on exactly one dof of its own");
      }
    for (int g = 0; g < ng; g++) {
      const int b = I("cg_bodyid")[g];
      if (b < 0 || b >= nb) return fail(VNL_ERR_UNSUPPORTED, "Newton solver: a contact is not attached to one dynamic body");
    }
    if (((d.fac_route >> VNL_ROUTE_QM_INVERSE) & 0xf) == VNL_ROUTE_LDS)
      return fail(VNL_ERR_UNSUPPORTED, "Newton solver: dof tree too deep for the register-resident inversion of the "
                                       "Hessian's factor (max depth < 36; rows 64 .. of depth < 16; nv <= 128)");
  }
  return VNL_OK;
}

static void layout(vnl_env* env) {
  const DevModel& d = env->dm;
  const WsLayout L = vnl_make_layout(dims_of(d));  // (csrc/vnl_types.h: the same function gives a specialised kernel its constants)
  env->L = L;
  auto sec = [&](const char* name, int at, int n) { env->sections[name] = {at, n}; };
  sec("qpos", L.qpos, d.nq), sec("qvel", L.qvel, d.nv), sec("act", L.act, d.nu), sec("ctrl", L.ctrl, d.nu);
  sec("act_dot", L.actdot, d.nu), sec("subtree_com1", L.com, 4), sec("cdof", L.cdof, 6 * d.nv);
  sec("qLD", L.LD, L.dinv - L.LD), sec("qLDiagInv", L.dinv, d.nv), sec("pool", L.P, L.smooth - L.P);
  sec("efc_D", L.efc_D, d.nefc), sec("Jaref", L.Jaref, d.nefc), sec("jv", L.jv, d.nefc);
  sec("qfrc_smooth", L.smooth, d.nv), sec("qacc_smooth", L.qacc_smooth, d.nv), sec("qacc", L.qacc, d.nv);
  sec("Ma", L.Ma, d.nv), sec("grad", L.grad, d.nv), sec("Mgrad", L.Mgrad, d.nv), sec("search", L.search, d.nv);
  sec("mv", L.mv, d.nv), sec("qfrc_constraint", L.qfrc_c, d.nv), sec("tmp", L.tmp, d.nv), sec("tmp2", L.tmp2, d.nv);
  sec("con_r", L.con_r, 3 * d.ncon), sec("con_t1", L.con_t1, 3 * d.ncg);
  sec("tab_anc", L.tab_anc, L.tab_madr - L.tab_anc), sec("tab_madr", L.tab_madr, L.tab_body - L.tab_madr);
  sec("tab_body", L.tab_body, L.tab_jump - L.tab_body), sec("tab_jump", L.tab_jump, L.tab_lvl - L.tab_jump);
  sec("tab_lvl", L.tab_lvl, L.act_list - L.tab_lvl);
  sec("act_list", L.act_list, vnl_words(4 * (long)((d.ncon + 3) / 4) + 8 + 2 * VNL_LIVE_MAX));
  sec("tab_con", L.tab_con, L.tab_path - L.tab_con), sec("tab_path", L.tab_path, L.tab_lim - L.tab_path);
  sec("tab_lim", L.tab_lim, L.con_mu - L.tab_lim), sec("con_mu", L.con_mu, d.ncg);
  if (d.solver_newton) {  // qM, and the Hessian's inverted L'DL factor and pivots, in the qLD layout
    sec("newton_qM", L.newt_M, d.nM), sec("newton_LD", L.newt_H, d.nM), sec("newton_LDiagInv", L.newt_H + d.nM, d.nv);
  }
#ifdef VNL_PROFILE
  sec("prof", L.prof, 2 * (VNL_NPROF + 1));
#endif
}

static bool same_layout(const WsLayout& a, const WsLayout& b) { return memcmp(&a, &b, sizeof(WsLayout)) == 0; }
static bool same_dims(const VnlDims& a, const VnlDims& b) { return memcmp(&a, &b, sizeof(VnlDims)) == 0; }
// eight workgroups per CU on 160 KB of LDS: the float32 rodent's working set, the solver's staged tables included, stays within 20,480 B
// (the diagnostic build -DVNL_PROFILE adds 328 B of stage stamps and runs at seven: its shares are read, not its times)
#ifndef VNL_PROFILE
static_assert(sizeof(vreal) != 4 || (size_t)VnlSpecRodent::L.total * sizeof(vreal) <= 20480, "the rodent's LDS layout no longer allows 8 workgroups per CU");
#endif

#include "vnl_env_kernels.h"

extern "C" void vnl_env_destroy(vnl_env* env) {
  if (!env) return;
  for (void* p : env->allocs) (void)hipFree(p);
  delete env->fmap;
  delete env;
}

extern "C" int vnl_env_create(const vnl_model* hm, const vnl_envspec* es, int32_t num_envs, int32_t device,
                              vnl_env** out) {
  if (!hm || !es || !out || num_envs <= 0) return fail(VNL_ERR_ARG, "vnl_env_create: bad argument");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(VNL_ERR_NO_DEVICE, "no HIP device: the rollout has no CPU fallback");
  if (device < 0 || device >= ndev) return fail(VNL_ERR_ARG, "device ordinal out of range");
  DeviceGuard guard(device);  // the caller's current device is restored on every return path
  if (!guard.ok) return fail(VNL_ERR_HIP, "hipSetDevice failed");
  vnl_env* env = new vnl_env();
  env->device = device, env->B = num_envs;
  int rc = build_dev_model(env, hm);
  if (rc != VNL_OK) {
    vnl_env_destroy(env);
    return rc;
  }
  const DevModel& d = env->dm;
  DevEnv& e = env->de;
  e.T = es->clip_frames, e.C = es->num_clips, e.ref_len = es->ref_traj_length, e.sub_clip_length = es->sub_clip_length;
  e.n_frames = es->n_frames, e.nb = es->num_track_bodies, e.nee = es->num_end_eff, e.napp = es->num_appendages;
  e.njc = es->num_joint_cols, e.com_ref_col = es->com_ref_col;
  e.healthy_lo = es->healthy_z_lo, e.healthy_hi = es->healthy_z_hi;
  e.inv_term_threshold = vreal(1) / es->termination_threshold, e.body_err_mult = es->body_error_multiplier;
  e.flags = es->flags, e.done_threshold = es->done_threshold, e.center_of_mass = nullptr;
  {
    const double builtin[6] = {0.01, 0.01, 0.01, 0.01, 0.0001, 0.01};  // rodent.py:203-209
    for (int k = 0; k < 6; k++) e.w_reward[k] = (es->flags & VNL_ENV_WEIGHTS) ? (vreal)es->reward_weights[k] : (vreal)builtin[k];
  }
  e.obs_size = (e.flags & VNL_ENV_OBS_QPOS_QVEL) ? d.nq + d.nv : d.nq + 2 * d.nv + 3 * e.nee;
  e.traj_size = e.ref_len * (3 * e.napp + 6 * e.nb + 3 + e.njc);
  bool ok = e.T >= e.ref_len && e.C >= 1 && e.nb >= 1 && e.com_ref_col >= 0 && e.com_ref_col < e.nb && d.nq >= 7 &&
            d.root_free;
  for (int k = 0; ok && k < e.nb; k++) ok = es->body_idxs[k] >= 0 && es->body_idxs[k] < d.nbody_out;
  for (int k = 0; ok && k < e.nee; k++) ok = es->end_eff_idx[k] >= 0 && es->end_eff_idx[k] < d.nbody_out;
  for (int k = 0; ok && k < e.napp; k++)
    ok = es->app_body[k] >= 0 && es->app_body[k] < d.nbody_out && es->app_ref_col[k] >= 0 && es->app_ref_col[k] < e.nb;
  for (int k = 0; ok && k < e.njc; k++) ok = es->joint_cols[k] >= 0 && es->joint_cols[k] < d.nq - 7;
  if (!ok) {
    vnl_env_destroy(env);
    return fail(VNL_ERR_ARG, "vnl_envspec: index out of range or unsupported shape");
  }
  size_t CT = (size_t)e.C * e.T, nj = d.nq - 7;
#define UP(call)              \
  if ((rc = (call)) != VNL_OK) { \
    vnl_env_destroy(env);     \
    return rc;                \
  }
  UP(upload_raw<int>(env, es->body_idxs, e.nb, &e.body_idxs))
  UP(upload_raw<int>(env, es->end_eff_idx, e.nee, &e.end_eff_idx))
  UP(upload_raw<int>(env, es->app_body, e.napp, &e.app_body))
  UP(upload_raw<int>(env, es->app_ref_col, e.napp, &e.app_ref_col))
  UP(upload_raw<int>(env, es->joint_cols, e.njc, &e.joint_cols))
  UP(upload_raw<float>(env, es->position, CT * 3, &e.position))
  UP(upload_raw<float>(env, es->quaternion, CT * 4, &e.quaternion))
  UP(upload_raw<float>(env, es->joints, CT * nj, &e.joints))
  UP(upload_raw<float>(env, es->body_positions, CT * e.nb * 3, &e.body_positions))
  UP(upload_raw<float>(env, es->velocity, CT * 3, &e.velocity))
  UP(upload_raw<float>(env, es->angular_velocity, CT * 3, &e.angular_velocity))
  UP(upload_raw<float>(env, es->joints_velocity, CT * nj, &e.joints_velocity))
  if (es->center_of_mass) UP(upload_raw<float>(env, es->center_of_mass, CT * 3, &e.center_of_mass))
#undef UP
  {
    void* p = nullptr;
    const size_t n2 = (size_t)num_envs * vnl_fac2_stride(d.nM, d.nv) * sizeof(vreal);
    HIPCHK(hipMalloc(&p, n2));
    env->allocs.push_back(p);
    HIPCHK(hipMemset(p, 0, n2));  // (the padding of a row is read with it, never used)
    e.fac2 = (vreal*)p;
  }
  {
    void* p = nullptr;
    HIPCHK(hipMalloc(&p, (size_t)num_envs * (2 * sizeof(int) + d.nq * sizeof(vreal))));
    env->allocs.push_back(p);
    env->rd_noise = (vreal*)p;
    env->rd_start = (int*)(env->rd_noise + (size_t)num_envs * d.nq), env->rd_clip = env->rd_start + num_envs;
  }
  layout(env);
  // a model whose every dimension and LDS offset equals the compile-time constants of a specialised kernel, and whose body
  // tree is the one that kernel's subtree sums are unrolled over, runs that kernel
  env->spec = (same_dims(dims_of(env->dm), VnlSpecRodent::D) && same_layout(env->L, VnlSpecRodent::L) &&
               vnl_same_tree<VnlSpecRodent>(env->dyn_parent.data(), (int)env->dyn_parent.size())) ? 1 : 0;
#ifdef VNL_NO_SPEC
  env->spec = 0;
#endif
  env->lds_bytes = (size_t)env->L.total * sizeof(vreal);
#ifdef VNL_STAGE_KNOBS
  if (const char* padk = getenv("VNL_DBG_LDS_BYTES")) {  // occupancy experiments only: force a larger LDS request
    size_t want = (size_t)atol(padk);
    if (want > env->lds_bytes) env->lds_bytes = want;
  }
#endif
  if (6 * d.nbody > 512) {
    vnl_env_destroy(env);
    return fail(VNL_ERR_UNSUPPORTED, "more than 85 dynamic bodies (the per-body scans of bias_forces keep 8 elements per lane)");
  }
  if (d.nu > d.nv) {
    vnl_env_destroy(env);
    return fail(VNL_ERR_UNSUPPORTED, "more actuators than dofs (the actuator forces are staged in two dof vectors)");
  }
  if (d.nefc > 512) {
    vnl_env_destroy(env);
    return fail(VNL_ERR_UNSUPPORTED, "more than 512 constraint rows (line-search rows are register-resident)");
  }
  if (env->lds_bytes > 64 * 1024) {
    vnl_env_destroy(env);
    return fail(VNL_ERR_UNSUPPORTED, "model too large: per-env working set exceeds 64 KB of LDS");
  }
  {
    int nb_ = 0;  // (of the step kernel this env runs)
    hipError_t r = env->spec ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb_, vnl_step_kernel<VnlSpecRodent>, 64, env->lds_bytes)
                             : hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb_, vnl_step_kernel<VnlSpecGeneric>, 64, env->lds_bytes);
    if (r == hipSuccess) env->blocks_per_cu = nb_;
  }
  {
    KernelConsts host{env->dm, env->de, env->L};
    void* p = nullptr;
    HIPCHK(hipMalloc(&p, sizeof(KernelConsts)));
    env->allocs.push_back(p);
    HIPCHK(hipMemcpy(p, &host, sizeof(KernelConsts), hipMemcpyHostToDevice));
    env->kc = (KernelConsts*)p;
  }
  *out = env;
  return VNL_OK;
}

extern "C" int vnl_env_dims(const vnl_env* env, vnl_dims* o) {
  if (!env || !o) return fail(VNL_ERR_ARG, "vnl_env_dims: null argument");
  const DevModel& d = env->dm;
  o->nq = d.nq, o->nv = d.nv, o->nu = d.nu, o->nbody = d.nbody_out, o->njnt = d.njnt, o->ngeom_collide = d.ncg;
  o->ncon = d.ncon, o->nefc = d.nefc, o->obs_size = env->de.obs_size, o->traj_size = env->de.traj_size;
  o->workspace_floats_per_env = env->L.total;
  o->workgroups_per_cu = env->blocks_per_cu;
  o->nbody_dynamic = d.nbody, o->kernel_specialised = env->spec;
  o->factor_route = d.fac_route;
  return VNL_OK;
}

extern "C" int vnl_env_scratch(const vnl_env* env, const char* name, float** dev_ptr, int32_t* count) {
  if (!env || !name || !dev_ptr || !count) return fail(VNL_ERR_ARG, "vnl_env_scratch: null argument");
  if (strncmp(name, "dom_", 4) == 0) {  // per-env parameter tables of a randomised env, [num_envs][count] (no debug needed)
    if (!env->has_dom) return fail(VNL_ERR_ARG, "vnl_env_scratch: %s: the env has no domain (vnl_env_set_domain / vnl_env_set_body_domain)", name);
    const DevModel& d = env->dm;
    const size_t B = (size_t)env->B;
    const size_t n4 = B * (2 * d.ncg + d.nu + 2 * d.nv), nd = (size_t)d.nbody;  // (the layout of domain_tables below)
    const struct { const char* k; size_t off; int n; } tabs[] = {
        {"dom_mu", 0, d.ncg}, {"dom_invw", B * d.ncg, d.ncg}, {"dom_gain", 2 * B * d.ncg, d.nu},
        {"dom_damp", B * (2 * d.ncg + d.nu), d.nv}, {"dom_arm", B * (2 * d.ncg + d.nu + d.nv), d.nv},
        {"dom_mass", n4, d.nbody}, {"dom_ipos", n4 + B * nd, 3 * d.nbody}, {"dom_inertia6", n4 + 4 * B * nd, 6 * d.nbody},
        {"dom_tminv", n4 + 10 * B * nd, 1}};
    for (const auto& t : tabs)
      if (strcmp(name, t.k) == 0) {
        *dev_ptr = (float*)(env->dom + t.off);
        *count = t.n;
        return VNL_OK;
      }
    return fail(VNL_ERR_ARG, "unknown scratch section %s", name);
  }
  if (strcmp(name, "fac_match") == 0) {  // the factorisation schedule as the kernels load it: [nv][count] 32-bit words (no debug needed)
    *dev_ptr = (float*)env->dm.fac_match;
    *count = vnl_fac_stride(env->dm.fac_steps) / 4;
    return VNL_OK;
  }
  if (!env->dump) return fail(VNL_ERR_ARG, "scratch dump is off: call vnl_env_debug(env, 1) before reset/step");
  if (strcmp(name, "solver_trace") == 0) {  // int32 [num_envs][n_frames][VNL_TRACE_INTS], contiguous (not inside the image)
    *dev_ptr = (float*)env->trace;
    *count = (env->de.n_frames > 0 ? env->de.n_frames : 1) * VNL_TRACE_INTS;
    return VNL_OK;
  }
  auto it = env->sections.find(name);
  if (it == env->sections.end()) return fail(VNL_ERR_ARG, "unknown scratch section %s", name);
  *dev_ptr = (float*)(env->dump + it->second.first);
  *count = it->second.second;
  return VNL_OK;
}

extern "C" int vnl_env_debug(vnl_env* env, int32_t enable, int32_t* row_stride) {
  if (!env) return fail(VNL_ERR_ARG, "vnl_env_debug: null argument");
  if (enable < 0 || enable > 2) return fail(VNL_ERR_ARG, "vnl_env_debug: mode must be 0, 1 or 2");
  if (enable && !env->dump) {
    void* p = nullptr;
    HIPCHK(hipMalloc(&p, (size_t)env->L.total * env->B * sizeof(vreal)));
    env->allocs.push_back(p);
    env->dump = (vreal*)p;
    const size_t nt = (size_t)env->B * (env->de.n_frames > 0 ? env->de.n_frames : 1) * VNL_TRACE_INTS * sizeof(int);
    HIPCHK(hipMalloc(&p, nt));
    env->allocs.push_back(p);
    HIPCHK(hipMemset(p, 0, nt));
    env->trace = (int*)p;
  }
  env->debug = enable;
  if (row_stride) *row_stride = env->L.total;
  return VNL_OK;
}

// ----------------------------------------------------------------------------- kernels
// (vnl_step_kernel / vnl_reset_kernel / vnl_reset_done_kernel: vnl_env_kernels.h)
__global__ void __launch_bounds__(64) vnl_fk_kernel(const KernelConsts* kc, DevState st, const vreal* qpos) {
  VNL_LDS_DECL(lds);
  const VNL_CAS KernelConsts* k = VNL_TO_CAS(KernelConsts, kc);
  EnvWave w{k->m, k->ev, st, k->L, lds, blockIdx.x, threadIdx.x, k, nullptr};
  w.fk(qpos);
}

// launchers of the randomised instantiations (csrc/vnl_domain.hip: a translation unit of their own); return a hipError_t
int vnl_domain_reset_(const KernelConsts* kc, int spec, int B, size_t lds, void* stream, const DevState& ds, const int* start_frame,
                      const vreal* noise, vreal* dump, int* trace);
int vnl_domain_step_(const KernelConsts* kc, int spec, int B, size_t lds, void* stream, const DevState& ds, const vreal* action,
                     vreal* dump, vreal* dump_mid, int* trace, const vnl_post_desc& post);
// .. and of the scoring step kernels, shared model and randomised (csrc/vnl_eval.hip: a translation unit of their own)
int vnl_eval_step_(const KernelConsts* kc, int spec, int dom, int B, size_t lds, void* stream, const DevState& ds,
                   const vreal* action, vreal* dump, vreal* dump_mid, int* trace, const vnl_post_desc& post,
                   const vnl_eval_desc& ev);
int vnl_domain_reset_done_(const KernelConsts* kc, int spec, int B, size_t lds, void* stream, const DevState& ds,
                           const ResetDoneArgs& a, vreal* dump, int* trace);
int vnl_domain_redraw_(const KernelConsts* kc, int spec, int B, void* stream, const float* mask, const int64_t* step_base,
                       int64_t step_offset, uint32_t key0, uint32_t key1, uint32_t env0, int initial);

static int to_dev_state(const vnl_state* s, DevState* d) {
  const void* ptrs[] = {s->qpos, s->qvel, s->act, s->qacc_warmstart, s->xpos, s->xquat, s->subtree_com1,
                        s->qfrc_actuator, s->obs, s->reward, s->done, s->metrics, s->traj, s->termination_error,
                        s->cur_frame, s->sub_clip_frame, s->clip_id};
  for (const void* p : ptrs)
    if (!p) return fail(VNL_ERR_ARG, "vnl_state: null buffer");
  // (vreal is float in the product; the casts only matter for the float64 test build)
  d->qpos = (vreal*)s->qpos, d->qvel = (vreal*)s->qvel, d->act = (vreal*)s->act, d->warm = (vreal*)s->qacc_warmstart;
  d->xpos = (vreal*)s->xpos, d->xquat = (vreal*)s->xquat, d->com1 = (vreal*)s->subtree_com1;
  d->qfrc_actuator = (vreal*)s->qfrc_actuator, d->obs = (vreal*)s->obs, d->reward = (vreal*)s->reward;
  d->done = (vreal*)s->done, d->metrics = (vreal*)s->metrics, d->traj = (vreal*)s->traj;
  d->term_err = (vreal*)s->termination_error, d->cur_frame = s->cur_frame, d->sub_clip_frame = s->sub_clip_frame;
  d->clip_id = s->clip_id;
  return VNL_OK;
}

extern "C" int vnl_env_reset(vnl_env* env, const int32_t* start_frame, const float* noise, const vnl_state* state,
                             void* stream) {
  if (!env || !start_frame || !noise || !state) return fail(VNL_ERR_ARG, "vnl_env_reset: null argument");
  DevState ds;
  int rc = to_dev_state(state, &ds);
  if (rc != VNL_OK) return rc;
  DeviceGuard guard(env->device);  // the launch goes to the env's GPU whatever the caller's current device is
  if (!guard.ok) return fail(VNL_ERR_HIP, "hipSetDevice failed");
  if (env->has_dom) {
    HIPCHK((hipError_t)vnl_domain_reset_(env->kc, env->spec, env->B, env->lds_bytes, stream, ds, (const int*)start_frame,
                                         (const vreal*)noise, env->debug ? env->dump : nullptr, env->debug ? env->trace : nullptr));
    return VNL_OK;
  }
  if (env->spec)
    hipLaunchKernelGGL((vnl_reset_kernel<VnlSpecRodent>), dim3(env->B), dim3(64), env->lds_bytes, (hipStream_t)stream,
                       (const KernelConsts*)env->kc, ds, (const int*)start_frame, (const vreal*)noise,
                       env->debug ? env->dump : nullptr, env->debug ? env->trace : nullptr);
  else
    hipLaunchKernelGGL((vnl_reset_kernel<VnlSpecGeneric>), dim3(env->B), dim3(64), env->lds_bytes, (hipStream_t)stream,
                       (const KernelConsts*)env->kc, ds, (const int*)start_frame, (const vreal*)noise,
                       env->debug ? env->dump : nullptr, env->debug ? env->trace : nullptr);
  HIPCHK(hipGetLastError());
  return VNL_OK;
}

// A fresh episode, drawn in the kernel, for the envs whose mask is set (include/vnl.h; EnvWaveT::reset_fresh)
// .. with the start frame and clip drawn from a table of start priorities and the ended episodes counted (include/vnl.h:
// vnl_start_priority; EnvWaveT::reset_fresh_weighted); a null `prio` = the uniform draws
extern "C" int vnl_env_reset_done_weighted(vnl_env* env, const float* mask, const vnl_reset_noise* noise,
                                           const vnl_start_priority* prio, const vnl_state* state, const vnl_reset_log* logs,
                                           int32_t num_logs, void* stream) {
  if (!env || !mask || !noise || !state) return fail(VNL_ERR_ARG, "vnl_env_reset_done: null argument");
  if (!noise->step_base) return fail(VNL_ERR_ARG, "vnl_reset_noise: step_base is null (a device pointer to the step counter)");
  if (noise->start_hi < 1) return fail(VNL_ERR_ARG, "vnl_reset_noise: start_hi must be at least 1");
  if (noise->step_offset < 0 || noise->env_offset < 0)
    return fail(VNL_ERR_ARG, "vnl_reset_noise: step_offset and env_offset must not be negative");
  if (noise->env_offset >= 0xFFFFFFFFll - (int64_t)env->B)  // (no sum: an offset near INT64_MAX must not wrap)
    return fail(VNL_ERR_ARG, "vnl_reset_noise: env_offset + num_envs must stay below 2^32 - 1");
  if (num_logs < 0 || num_logs > VNL_RESET_MAX_LOGS || (num_logs > 0 && !logs))
    return fail(VNL_ERR_ARG, "vnl_env_reset_done: num_logs must be 0..8, with logs given");
  for (int k = 0; k < num_logs; k++)
    if (!logs[k].src || !logs[k].log || logs[k].width <= 0) return fail(VNL_ERR_ARG, "vnl_env_reset_done: bad log");
  DevState ds;
  int rc = to_dev_state(state, &ds);
  if (rc != VNL_OK) return rc;
  if (prio) {
    if (!prio->cdf) return fail(VNL_ERR_ARG, "vnl_start_priority: cdf is null");
    if (prio->ncell > VNL_PRIORITY_MAX_CELLS) return fail(VNL_ERR_UNSUPPORTED, "vnl_start_priority: more than 32768 cells");
    if ((int64_t)prio->ncell != (int64_t)env->de.C * noise->start_hi)
      return fail(VNL_ERR_ARG, "vnl_start_priority: ncell must be num_clips * start_hi");
    if (!prio->ended != !prio->failed) return fail(VNL_ERR_ARG, "vnl_start_priority: ended and failed go together");
  }
  ResetDoneArgs a{};
  if (prio) {
    a.prio.cdf = prio->cdf, a.prio.ncell = prio->ncell, a.prio.ended = prio->ended, a.prio.failed = prio->failed;
    a.prio.truncation = prio->truncation;
  }
  a.mask = mask, a.step_base = noise->step_base, a.step_offset = noise->step_offset;
  a.key0 = (uint32_t)noise->seed, a.key1 = (uint32_t)(noise->seed >> 32), a.env0 = (uint32_t)noise->env_offset;
  a.start_hi = (uint32_t)noise->start_hi, a.noise_scale = noise->noise_scale, a.num_logs = num_logs;
  a.start_frame = noise->start_frame_out ? (int*)noise->start_frame_out : env->rd_start;
  a.clip_id = noise->clip_id_out ? (int*)noise->clip_id_out : env->rd_clip;
  a.noise = noise->noise_out ? (vreal*)noise->noise_out : env->rd_noise;
  for (int k = 0; k < num_logs; k++)
    a.logs[k].src = (const unsigned*)logs[k].src, a.logs[k].log = (unsigned*)logs[k].log, a.logs[k].width = logs[k].width;
  DeviceGuard guard(env->device);
  if (!guard.ok) return fail(VNL_ERR_HIP, "hipSetDevice failed");
  vreal* dump = env->debug ? env->dump : nullptr;
  int* trace = env->debug ? env->trace : nullptr;
  if (env->has_dom) {
    HIPCHK((hipError_t)vnl_domain_reset_done_(env->kc, env->spec, env->B, env->lds_bytes, stream, ds, a, dump, trace));
    return VNL_OK;
  }
  if (env->spec)
    hipLaunchKernelGGL((vnl_reset_done_kernel<VnlSpecRodent>), dim3(env->B), dim3(64), env->lds_bytes, (hipStream_t)stream,
                       (const KernelConsts*)env->kc, ds, a, dump, trace);
  else
    hipLaunchKernelGGL((vnl_reset_done_kernel<VnlSpecGeneric>), dim3(env->B), dim3(64), env->lds_bytes, (hipStream_t)stream,
                       (const KernelConsts*)env->kc, ds, a, dump, trace);
  HIPCHK(hipGetLastError());
  return VNL_OK;
}

extern "C" int vnl_env_reset_done(vnl_env* env, const float* mask, const vnl_reset_noise* noise, const vnl_state* state,
                                  const vnl_reset_log* logs, int32_t num_logs, void* stream) {
  return vnl_env_reset_done_weighted(env, mask, noise, nullptr, state, logs, num_logs, stream);
}

extern "C" int vnl_env_fk(vnl_env* env, const float* qpos, const vnl_state* state, void* stream) {
  if (!env || !qpos || !state) return fail(VNL_ERR_ARG, "vnl_env_fk: null argument");
  DevState ds;
  int rc = to_dev_state(state, &ds);
  if (rc != VNL_OK) return rc;
  DeviceGuard guard(env->device);
  if (!guard.ok) return fail(VNL_ERR_HIP, "hipSetDevice failed");
  hipLaunchKernelGGL(vnl_fk_kernel, dim3(env->B), dim3(64), env->lds_bytes, (hipStream_t)stream, (const KernelConsts*)env->kc, ds,
                     (const vreal*)qpos);
  HIPCHK(hipGetLastError());
  return VNL_OK;
}

// (vnl_rollout_post and vnl_env_step_post: one validation, one set of messages)
static int post_desc_check(const vnl_post_desc* desc, int32_t num_envs) {
  if (!desc || num_envs <= 0 || !desc->done) return fail(VNL_ERR_ARG, "vnl_rollout_post: null argument");
  if (desc->num_ops < 0 || desc->num_ops > VNL_POST_MAX_OPS) return fail(VNL_ERR_ARG, "vnl_rollout_post: too many ops");
  for (int k = 0; k < desc->num_ops; k++)
    if (!desc->ops[k].src || desc->ops[k].width <= 0) return fail(VNL_ERR_ARG, "vnl_rollout_post: bad op");
  if ((desc->log_reward && !desc->reward)) return fail(VNL_ERR_ARG, "vnl_rollout_post: log_reward without reward");
  return VNL_OK;
}

// (vnl_rollout_eval and vnl_env_step_post_eval: one validation, one set of messages, each naming its field)
static int eval_desc_check(const vnl_eval_desc* d, int32_t num_envs) {
  if (!d) return fail(VNL_ERR_ARG, "vnl_rollout_eval: desc is null");
  if (num_envs <= 0) return fail(VNL_ERR_ARG, "vnl_rollout_eval: num_envs must be positive");
  if (!d->done) return fail(VNL_ERR_ARG, "vnl_eval_desc: done is null");
  if (!d->steps) return fail(VNL_ERR_ARG, "vnl_eval_desc: steps is null");
  if (!d->reward) return fail(VNL_ERR_ARG, "vnl_eval_desc: reward is null");
  if (!d->metrics) return fail(VNL_ERR_ARG, "vnl_eval_desc: metrics is null");
  if (!d->run) return fail(VNL_ERR_ARG, "vnl_eval_desc: run is null");
  if (!d->count) return fail(VNL_ERR_ARG, "vnl_eval_desc: count is null");
  if (!d->records) return fail(VNL_ERR_ARG, "vnl_eval_desc: records is null");
  if (d->episodes_per_env < 1) return fail(VNL_ERR_ARG, "vnl_eval_desc: episodes_per_env must be at least 1");
  if (!d->cur_frame != !d->sub_clip_frame || !d->cur_frame != !d->clip_id)
    return fail(VNL_ERR_ARG, "vnl_eval_desc: cur_frame, sub_clip_frame and clip_id go together (all three or none)");
  return VNL_OK;
}

// `post`: the descriptor the step waves run as their epilogue, or null (num_ops < 0 in the kernel: no epilogue); `ev` (with
// `post`): the scoring after it -- the launch of vnl_step_eval_kernel -- or null
static int env_step_launch(vnl_env* env, const float* action, const vnl_state* state, const vnl_post_desc* post,
                           const vnl_eval_desc* ev, void* stream) {
  DevState ds;
  int rc = to_dev_state(state, &ds);
  if (rc != VNL_OK) return rc;
  DeviceGuard guard(env->device);
  if (!guard.ok) return fail(VNL_ERR_HIP, "hipSetDevice failed");
  vnl_post_desc none{};
  none.num_ops = -1;
  const vnl_post_desc& pd = post ? *post : none;
  if (ev) {
    HIPCHK((hipError_t)vnl_eval_step_(env->kc, env->spec, env->has_dom, env->B, env->lds_bytes, stream, ds, (const vreal*)action,
                                      env->debug == 1 ? env->dump : nullptr, env->debug == 2 ? env->dump : nullptr,
                                      env->debug ? env->trace : nullptr, pd, *ev));
    return VNL_OK;
  }
  if (env->has_dom) {
    HIPCHK((hipError_t)vnl_domain_step_(env->kc, env->spec, env->B, env->lds_bytes, stream, ds, (const vreal*)action,
                                        env->debug == 1 ? env->dump : nullptr, env->debug == 2 ? env->dump : nullptr,
                                        env->debug ? env->trace : nullptr, pd));
    return VNL_OK;
  }
  if (env->spec)
    hipLaunchKernelGGL((vnl_step_kernel<VnlSpecRodent>), dim3(env->B), dim3(64), env->lds_bytes, (hipStream_t)stream,
                       (const KernelConsts*)env->kc, ds, (const vreal*)action, env->debug == 1 ? env->dump : nullptr,
                       env->debug == 2 ? env->dump : nullptr, env->debug ? env->trace : nullptr, pd);
  else
    hipLaunchKernelGGL((vnl_step_kernel<VnlSpecGeneric>), dim3(env->B), dim3(64), env->lds_bytes, (hipStream_t)stream,
                       (const KernelConsts*)env->kc, ds, (const vreal*)action, env->debug == 1 ? env->dump : nullptr,
                       env->debug == 2 ? env->dump : nullptr, env->debug ? env->trace : nullptr, pd);
  HIPCHK(hipGetLastError());
  return VNL_OK;
}

extern "C" int vnl_env_step(vnl_env* env, const float* action, const vnl_state* state, void* stream) {
  if (!env || !action || !state) return fail(VNL_ERR_ARG, "vnl_env_step: null argument");
  return env_step_launch(env, action, state, nullptr, nullptr, stream);
}

// The step with vnl_rollout_post(desc, num_envs = the env's B) as the epilogue of each step wave (include/vnl.h)
extern "C" int vnl_env_step_post(vnl_env* env, const float* action, const vnl_state* state, const vnl_post_desc* desc,
                                 void* stream) {
  if (!env || !action || !state) return fail(VNL_ERR_ARG, "vnl_env_step_post: null argument");
  int rc = post_desc_check(desc, env->B);
  if (rc != VNL_OK) return rc;
  return env_step_launch(env, action, state, desc, nullptr, stream);
}

// .. and with vnl_rollout_eval(eval, num_envs = the env's B) after it in the same wave (include/vnl.h)
extern "C" int vnl_env_step_post_eval(vnl_env* env, const float* action, const vnl_state* state, const vnl_post_desc* desc,
                                      const vnl_eval_desc* eval, void* stream) {
  if (!env || !action || !state) return fail(VNL_ERR_ARG, "vnl_env_step_post_eval: null argument");
  int rc = post_desc_check(desc, env->B);
  if (rc != VNL_OK) return rc;
  rc = eval_desc_check(eval, env->B);
  if (rc != VNL_OK) return rc;
  return env_step_launch(env, action, state, desc, eval, stream);
}

// Domain randomisation (brax / MJX semantics: raw fields are replaced, the derived constants -- dof / body invweight0,
// meaninertia, scale -- stay as compiled), in two parts that compose: vnl_env_set_domain (friction, actuator gain, damping,
// armature) and vnl_env_set_body_domain (body mass, principal moments, centre of mass).  What the upload derives from these
// fields -- the contact rows' mu and inverse weight; the fold of the welded bodies, the packed inertia, 1 / total mass -- is
// derived here per env by the upload's own float64 code, so values equal to the compiled ones give bit-identical tables.  One
// set of randomised kernels reads all nine tables: the part that was not set holds the compiled values in every env.
// Synchronous: the calls wait for `stream`, read the inputs to the host, validate, derive, write the library-owned tables.

// the four-field tables of `v` (per field [B][n] float64): [B][ncg] mu | [B][ncg] invweight | [B][nu] gain | [B][nv] damping |
// [B][nv] armature, cast to vreal as the upload does
static std::vector<vreal> four_field_tables(const vnl_env* env, const std::vector<double> v[4]) {
  const DevModel& d = env->dm;
  std::vector<vreal> tab;
  tab.reserve((size_t)env->B * (2 * d.ncg + d.nu + 2 * d.nv));
  for (double x : v[0]) tab.push_back((vreal)x);
  for (size_t k = 0; k < v[0].size(); k++) tab.push_back((vreal)contact_invweight(env->cg_t[k % d.ncg], v[0][k], env->impratio));
  for (int f = 1; f < 4; f++)
    for (double x : v[f]) tab.push_back((vreal)x);
  return tab;
}
static std::vector<vreal> four_field_compiled(const vnl_env* env) {
  const std::vector<double>* model[4] = {&env->mu0, &env->gain0, &env->damp0, &env->arm0};
  std::vector<double> v[4];
  for (int f = 0; f < 4; f++)
    for (int e = 0; e < env->B; e++) v[f].insert(v[f].end(), model[f]->begin(), model[f]->end());
  return four_field_tables(env, v);
}

// One env's row of the body tables from its three raw arrays over the bodies as given (null: the compiled array): the
// upload's fold and packing.  out: [nd] mass | [3 nd] ipos | [6 nd] inertia6 | 1 / total mass, float64.  Returns the name of
// the field at fault (and `why`), or null; with a null `why` nothing is validated (the compiled values: what the upload
// accepted is what an unset part reads).
static const char* body_row(const vnl_env* env, const double* mass, const double* inertia, const double* ipos, std::vector<double>* out,
                            char* why, size_t nwhy) {
  const int nb = env->fmap->nb_out, nd = env->dm.nbody;
  std::vector<double> full;
  if (inertia) {  // compiled full inertia + R diag(moments - compiled moments) R': exactly the compiled one where they are equal
    full = env->ifull0;
    for (int b = 1; b < nb; b++)
      vnl_full_inertia(&env->ifull0[9 * (size_t)b], &env->R_iq0[9 * (size_t)b], &inertia[3 * (size_t)b], &env->inertia0[3 * (size_t)b],
                       &full[9 * (size_t)b]);
  }
  std::vector<double> M, nip, nI;
  fuse_inertial(*env->fmap, nd, mass ? mass : env->mass0.data(), ipos ? ipos : env->ipos0.data(),
                inertia ? full.data() : env->ifull0.data(), &M, &nip, &nI);
  double tm = 0;
  for (int b = 0; b < nd; b++) {
    tm += M[b];
    if (!why || b == 0 || env->dyn_dofnum[b] <= 0) continue;
    if (!(M[b] > 0)) {
      snprintf(why, nwhy, "dynamic body %d (body %d as given, with what is welded to it) carries dofs and has mass %g", b, env->fmap->body_out[b], M[b]);
      return "body_mass";
    }
    for (int k = 0; k < 3; k++)
      if (!(nI[9 * (size_t)b + 4 * k] > 0)) {
        snprintf(why, nwhy, "dynamic body %d (body %d as given) carries dofs and has inertia diagonal %g", b, env->fmap->body_out[b], nI[9 * (size_t)b + 4 * k]);
        return "body_inertia";
      }
  }
  if (why && !(tm > 0)) {
    snprintf(why, nwhy, "total mass %g", tm);
    return "body_mass";
  }
  const std::vector<double> i6 = pack_inertia6(nI);
  out->clear();
  out->insert(out->end(), M.begin(), M.end()), out->insert(out->end(), nip.begin(), nip.end());
  out->insert(out->end(), i6.begin(), i6.end()), out->push_back(total_mass_inv_of(M));
  return nullptr;
}
// rows [B][10 nd + 1] -> the body tables [B][nd] | [B][3 nd] | [B][6 nd] | [B], cast to vreal last
static std::vector<vreal> body_tables(const vnl_env* env, const std::vector<std::vector<double>>& rows) {
  const size_t B = (size_t)env->B, nd = (size_t)env->dm.nbody;
  std::vector<vreal> tab(B * (10 * nd + 1));
  const size_t off[4] = {0, B * nd, 4 * B * nd, 10 * B * nd}, w[4] = {nd, 3 * nd, 6 * nd, 1}, at[4] = {0, nd, 4 * nd, 10 * nd};
  for (size_t e = 0; e < B; e++) {
    const std::vector<double>& r = rows[rows.size() == 1 ? 0 : e];
    for (int t = 0; t < 4; t++)
      for (size_t k = 0; k < w[t]; k++) tab[off[t] + e * w[t] + k] = (vreal)r[at[t] + k];
  }
  return tab;
}
static std::vector<vreal> body_compiled(const vnl_env* env) {
  std::vector<std::vector<double>> rows(1);
  (void)body_row(env, nullptr, nullptr, nullptr, &rows[0], nullptr, 0);
  return body_tables(env, rows);
}

// allocates the tables once, both parts holding the compiled values, and points KernelConsts::dom at them
static int domain_tables(vnl_env* env) {
  if (env->dom) return VNL_OK;
  const DevModel& d = env->dm;
  const size_t B = (size_t)env->B, n4 = B * (2 * d.ncg + d.nu + 2 * d.nv), nd = (size_t)d.nbody;
  std::vector<vreal> tab = four_field_compiled(env);
  const std::vector<vreal> body = body_compiled(env);
  tab.insert(tab.end(), body.begin(), body.end());
  void* p = nullptr;
  HIPCHK(hipMalloc(&p, tab.size() * sizeof(vreal)));
  env->allocs.push_back(p);
  HIPCHK(hipMemcpy(p, tab.data(), tab.size() * sizeof(vreal), hipMemcpyHostToDevice));
  env->dom = (vreal*)p;
  DevDomain dd;
  dd.cg_mu = env->dom, dd.cg_invweight = env->dom + B * d.ncg, dd.act_gain = env->dom + 2 * B * d.ncg;
  dd.dof_damping = dd.act_gain + B * d.nu, dd.dof_armature = dd.dof_damping + B * d.nv;
  dd.body_mass = env->dom + n4, dd.body_ipos = dd.body_mass + B * nd, dd.body_inertia6 = dd.body_mass + 4 * B * nd;
  dd.total_mass_inv = dd.body_mass + 10 * B * nd;
  HIPCHK(hipMemcpy((char*)env->kc + offsetof(KernelConsts, dom), &dd, sizeof(DevDomain), hipMemcpyHostToDevice));
  return VNL_OK;
}

// DevDomainRanges::on: which of the two range sets the env has (one word, read by every reset env of a randomised kernel)
static int ranges_on(const vnl_env* env) {
  return (env->has_ranges ? VNL_RANGES_FOUR : 0) | (env->has_body_ranges ? VNL_RANGES_BODY : 0);
}
static int clear_domain_ranges(vnl_env* env) {
  if (env->has_ranges) {
    env->has_ranges = 0;
    DevDomainRanges none{};
    none.on = ranges_on(env);
    HIPCHK(hipMemcpy((char*)env->kc + offsetof(KernelConsts, rng), &none, sizeof(DevDomainRanges), hipMemcpyHostToDevice));
  }
  env->has_ranges = 0;
  return VNL_OK;
}
static int clear_body_ranges(vnl_env* env) {
  if (env->has_body_ranges) {
    env->has_body_ranges = 0;
    const int on = ranges_on(env);
    HIPCHK(hipMemcpy((char*)env->kc + offsetof(KernelConsts, rng) + offsetof(DevDomainRanges, on), &on, sizeof(int), hipMemcpyHostToDevice));
  }
  return VNL_OK;
}

extern "C" int vnl_env_set_domain(vnl_env* env, const vnl_domain* dom, void* stream) {
  if (!env) return fail(VNL_ERR_ARG, "vnl_env_set_domain: null env");
  DeviceGuard guard(env->device);
  if (!guard.ok) return fail(VNL_ERR_HIP, "hipSetDevice failed");
#ifndef VNL_FORKJOIN_DEFINED
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));  // (the inputs may have been written, the tables read, on the stream)
#else
  (void)stream;
#endif
  const DevModel& d = env->dm;
  const size_t B = (size_t)env->B;
  if (!dom) {
    if (env->dom) {  // (the tables outlive the clear -- the other part may be set, now or later: back to the compiled values)
      const std::vector<vreal> tab = four_field_compiled(env);
      if (!tab.empty()) HIPCHK(hipMemcpy(env->dom, tab.data(), tab.size() * sizeof(vreal), hipMemcpyHostToDevice));
    }
    env->has_dom4 = 0, env->has_dom = env->has_body;
    return clear_domain_ranges(env);  // (ranges without a four-field domain would redraw tables nobody owns)
  }
  struct Field {
    const char* name;
    const double* src;
    const std::vector<double>& model;
    int n;
    int rule;  // 0: > 0, 1: >= 0, 2: finite only
  } fields[] = {{"cg_friction", dom->cg_friction, env->mu0, d.ncg, 0}, {"act_gain", dom->act_gain, env->gain0, d.nu, 2},
                {"dof_damping", dom->dof_damping, env->damp0, d.nv, 1}, {"dof_armature", dom->dof_armature, env->arm0, d.nv, 1}};
  std::vector<double> v[4];
  for (int f = 0; f < 4; f++) {
    const Field& F = fields[f];
    v[f].resize(B * F.n);
    if (F.src) {
      if (F.n > 0) HIPCHK(hipMemcpy(v[f].data(), F.src, v[f].size() * sizeof(double), hipMemcpyDeviceToHost));
    } else {
      for (size_t e = 0; e < B; e++) std::copy(F.model.begin(), F.model.end(), v[f].begin() + e * F.n);
    }
    for (size_t k = 0; k < v[f].size(); k++) {
      const double x = v[f][k];
      const bool ok = std::isfinite(x) && (F.rule == 2 || (F.rule == 1 ? x >= 0 : x > 0));
      if (!ok) {
        char where[96];
        snprintf(where, sizeof(where), "env %zu, index %zu (%g)", k / F.n, k % F.n, x);
        return fail(VNL_ERR_ARG, F.rule == 0 ? "vnl_env_set_domain: %s must be finite and > 0: %s"
                                 : F.rule == 1 ? "vnl_env_set_domain: %s must be finite and >= 0: %s"
                                               : "vnl_env_set_domain: %s must be finite: %s",
                    F.name, where);
      }
    }
  }
  const std::vector<vreal> tab = four_field_tables(env, v);
  int rc = domain_tables(env);
  if (rc != VNL_OK) return rc;
  if (!tab.empty()) HIPCHK(hipMemcpy(env->dom, tab.data(), tab.size() * sizeof(vreal), hipMemcpyHostToDevice));
  env->has_dom4 = 1, env->has_dom = 1;
  return VNL_OK;
}

// Ranges of the domain redraw at fresh resets (include/vnl.h: vnl_domain_ranges).  The contract of vnl_env_set_domain: waits
// for `stream`, reads the bounds to the host, validates, and only then allocates and writes.
extern "C" int vnl_env_set_domain_ranges(vnl_env* env, const vnl_domain_ranges* rg, void* stream) {
  if (!env) return fail(VNL_ERR_ARG, "vnl_env_set_domain_ranges: null env");
  DeviceGuard guard(env->device);
  if (!guard.ok) return fail(VNL_ERR_HIP, "hipSetDevice failed");
#ifndef VNL_FORKJOIN_DEFINED
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
#else
  (void)stream;
#endif
  if (!rg) return clear_domain_ranges(env);
  const DevModel& d = env->dm;
  const struct {
    const char* name;
    int n;
    int rule;  // 0: lo > 0, 1: lo >= 0, 2: finite only
  } fields[4] = {{"cg_friction", d.ncg, 0}, {"act_gain", d.nu, 2}, {"dof_damping", d.nv, 1}, {"dof_armature", d.nv, 1}};
  if (rg->shared & ~0xFu) return fail(VNL_ERR_ARG, "vnl_env_set_domain_ranges: shared has bits beyond the four fields");
  std::vector<double> buf(env->cg_t.begin(), env->cg_t.end());
  buf.resize((size_t)d.ncg, 0.0);
  buf.push_back(env->impratio);
  size_t at[4] = {0, 0, 0, 0};  // offset of lo[f] in buf (hi[f] follows it), 0: the field has no bounds
  for (int f = 0; f < 4; f++) {
    const auto& F = fields[f];
    if (!rg->lo[f] != !rg->hi[f])
      return fail(VNL_ERR_ARG, "vnl_env_set_domain_ranges: %s: lo and hi must both be given or both be null", F.name);
    if (!rg->lo[f]) continue;
    at[f] = buf.size();
    buf.resize(buf.size() + 2 * (size_t)F.n);
    double *lo = buf.data() + at[f], *hi = lo + F.n;
    if (F.n > 0) {
      HIPCHK(hipMemcpy(lo, rg->lo[f], F.n * sizeof(double), hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(hi, rg->hi[f], F.n * sizeof(double), hipMemcpyDeviceToHost));
    }
    for (int k = 0; k < F.n; k++) {
      const bool ok = std::isfinite(lo[k]) && std::isfinite(hi[k]) && lo[k] <= hi[k] &&
                      (F.rule == 2 || (F.rule == 1 ? lo[k] >= 0 : lo[k] > 0));
      if (!ok) {
        char where[96];
        snprintf(where, sizeof(where), "index %d (lo %g, hi %g)", k, lo[k], hi[k]);
        return fail(VNL_ERR_ARG, F.rule == 0   ? "vnl_env_set_domain_ranges: %s needs finite 0 < lo <= hi: %s"
                                 : F.rule == 1 ? "vnl_env_set_domain_ranges: %s needs finite 0 <= lo <= hi: %s"
                                               : "vnl_env_set_domain_ranges: %s needs finite lo <= hi: %s",
                    F.name, where);
      }
    }
  }
  int rc = domain_tables(env);  // (an env without a domain: the tables at the compiled values)
  if (rc != VNL_OK) return rc;
  if (!env->rng_buf) {  // room for every field, whatever this call gives
    void* p = nullptr;
    HIPCHK(hipMalloc(&p, ((size_t)d.ncg + 1 + 2 * ((size_t)d.ncg + d.nu + 2 * (size_t)d.nv)) * sizeof(double)));
    env->allocs.push_back(p);
    env->rng_buf = (double*)p;
  }
  HIPCHK(hipMemcpy(env->rng_buf, buf.data(), buf.size() * sizeof(double), hipMemcpyHostToDevice));
  const size_t B = (size_t)env->B;
  DevDomainRanges dr{};
  env->has_ranges = 1;
  dr.on = ranges_on(env), dr.shared = rg->shared, dr.cg_t = env->rng_buf;
  for (int f = 0; f < 4; f++)
    if (at[f]) dr.lo[f] = env->rng_buf + at[f], dr.hi[f] = env->rng_buf + at[f] + fields[f].n;
  dr.cg_mu = env->dom, dr.cg_invweight = env->dom + B * d.ncg, dr.act_gain = env->dom + 2 * B * d.ncg;  // (the layout of domain_tables)
  dr.dof_damping = dr.act_gain + B * d.nu, dr.dof_armature = dr.dof_damping + B * d.nv;
  HIPCHK(hipMemcpy((char*)env->kc + offsetof(KernelConsts, rng), &dr, sizeof(DevDomainRanges), hipMemcpyHostToDevice));
  env->has_ranges = 1, env->has_dom4 = 1, env->has_dom = 1;
  return VNL_OK;
}

// The redraw of vnl_env_reset_done as a launch of its own (EnvWaveT::redraw_domain; include/vnl.h)
extern "C" int vnl_env_redraw_domain(vnl_env* env, const float* mask, const vnl_reset_noise* noise, int32_t initial, void* stream) {
  if (!env || !noise) return fail(VNL_ERR_ARG, "vnl_env_redraw_domain: null argument");
  if (!env->has_ranges && !env->has_body_ranges)
    return fail(VNL_ERR_ARG, "vnl_env_redraw_domain: the env has no ranges (vnl_env_set_domain_ranges, vnl_env_set_body_domain_ranges)");
  if (!noise->step_base) return fail(VNL_ERR_ARG, "vnl_reset_noise: step_base is null (a device pointer to the step counter)");
  if (noise->step_offset < 0 || noise->env_offset < 0)
    return fail(VNL_ERR_ARG, "vnl_reset_noise: step_offset and env_offset must not be negative");
  if (noise->env_offset >= 0xFFFFFFFFll - (int64_t)env->B)
    return fail(VNL_ERR_ARG, "vnl_reset_noise: env_offset + num_envs must stay below 2^32 - 1");
  if (initial != 0 && initial != 1) return fail(VNL_ERR_ARG, "vnl_env_redraw_domain: initial must be 0 or 1");
  DeviceGuard guard(env->device);
  if (!guard.ok) return fail(VNL_ERR_HIP, "hipSetDevice failed");
  HIPCHK((hipError_t)vnl_domain_redraw_(env->kc, env->spec, env->B, stream, mask, noise->step_base, noise->step_offset,
                                        (uint32_t)noise->seed, (uint32_t)(noise->seed >> 32), (uint32_t)noise->env_offset, initial));
  return VNL_OK;
}

// The device buffer of vnl_env_set_body_domain_ranges: float64 sections, then the integer ones (offsets in bytes)
struct BodyRangesLayout {
  size_t lo[3], hi[3], raw, out_pos, R_out, ifull0, inertia0, R_iq0, stage, mem_start, mem, body_out, total;
};
static BodyRangesLayout body_ranges_layout(const vnl_env* env) {
  const size_t B = (size_t)env->B, nb = (size_t)env->dm.nbody_out, nd = (size_t)env->dm.nbody, w[3] = {1, 3, 3};
  BodyRangesLayout L{};
  size_t o = 0;
  auto sec = [&o](size_t n, size_t size) {
    const size_t at = o;
    o += n * size;
    return at;
  };
  for (int f = 0; f < 3; f++) L.lo[f] = sec(w[f] * nb, 8), L.hi[f] = sec(w[f] * nb, 8);
  L.raw = sec(B * 7 * nb, 8), L.out_pos = sec(3 * nb, 8), L.R_out = sec(9 * nb, 8), L.ifull0 = sec(9 * nb, 8);
  L.inertia0 = sec(3 * nb, 8), L.R_iq0 = sec(9 * nb, 8), L.stage = sec(B * (VNL_FOLD_REC * nb + nd), 8);
  L.mem_start = sec(nd + 1, 4), L.mem = sec(nb, 4), L.body_out = sec(nd, 4);
  L.total = o;
  return L;
}
// [B][7 nb] mass | moments | ipos of every env: what vnl_env_set_body_domain was given, else the compiled values (moments of a
// model without body_inertia: zeros, as its compiled moments read -- the difference the full inertia is built from is zero)
static std::vector<double> body_raw_rows(const vnl_env* env) {
  const size_t B = (size_t)env->B, nb = (size_t)env->dm.nbody_out, w[3] = {1, 3, 3}, at[3] = {0, nb, 4 * nb};
  const std::vector<double> zeros(3 * nb, 0.0);
  const std::vector<double>* model[3] = {&env->mass0, env->inertia0.empty() ? &zeros : &env->inertia0, &env->ipos0};
  std::vector<double> raw(B * 7 * nb);
  for (size_t e = 0; e < B; e++)
    for (int f = 0; f < 3; f++) {
      const double* src = env->body_raw[f].empty() ? model[f]->data() : &env->body_raw[f][e * w[f] * nb];
      std::copy(src, src + w[f] * nb, raw.begin() + e * 7 * nb + at[f]);
    }
  return raw;
}

extern "C" int vnl_env_set_body_domain(vnl_env* env, const vnl_body_domain* bd, void* stream) {
  if (!env) return fail(VNL_ERR_ARG, "vnl_env_set_body_domain: null env");
  DeviceGuard guard(env->device);
  if (!guard.ok) return fail(VNL_ERR_HIP, "hipSetDevice failed");
#ifndef VNL_FORKJOIN_DEFINED
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
#else
  (void)stream;
#endif
  const DevModel& d = env->dm;
  const size_t B = (size_t)env->B, nb = (size_t)d.nbody_out, n4 = B * (2 * d.ncg + d.nu + 2 * d.nv);
  if (!bd) {
    if (env->dom) {
      const std::vector<vreal> tab = body_compiled(env);
      HIPCHK(hipMemcpy(env->dom + n4, tab.data(), tab.size() * sizeof(vreal), hipMemcpyHostToDevice));
    }
    env->has_body = 0, env->has_dom = env->has_dom4;
    for (auto& r : env->body_raw) r.clear();
    return clear_body_ranges(env);  // (ranges without a body domain would redraw tables nobody owns)
  }
  if (bd->body_inertia && env->inertia0.empty())
    return fail(VNL_ERR_BLOB, "vnl_env_set_body_domain: body_inertia needs the model's body_inertia and body_iquat sections");
  struct Field {
    const char* name;
    const double* src;
    const std::vector<double>& model;
    size_t w;
    bool nonneg;
  } fields[] = {{"body_mass", bd->body_mass, env->mass0, 1, true}, {"body_inertia", bd->body_inertia, env->inertia0, 3, true},
                {"body_ipos", bd->body_ipos, env->ipos0, 3, false}};
  std::vector<double> v[3];
  for (int f = 0; f < 3; f++) {
    const Field& F = fields[f];
    if (!F.src) continue;
    const size_t n = nb * F.w;
    v[f].resize(B * n);
    HIPCHK(hipMemcpy(v[f].data(), F.src, v[f].size() * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t e = 0; e < B; e++) std::copy(F.model.begin(), F.model.begin() + F.w, v[f].begin() + e * n);  // row 0 is not read
    for (size_t k = 0; k < v[f].size(); k++) {
      const double x = v[f][k];
      if (!(std::isfinite(x) && (!F.nonneg || x >= 0))) {
        char where[96];
        snprintf(where, sizeof(where), "env %zu, index %zu (%g)", k / n, k % n, x);
        return fail(VNL_ERR_ARG, F.nonneg ? "vnl_env_set_body_domain: %s must be finite and >= 0: %s"
                                          : "vnl_env_set_body_domain: %s must be finite: %s", F.name, where);
      }
    }
  }
  std::vector<std::vector<double>> rows(B);
  for (size_t e = 0; e < B; e++) {
    char why[160], where[200];
    const char* bad = body_row(env, v[0].empty() ? nullptr : &v[0][e * nb], v[1].empty() ? nullptr : &v[1][e * 3 * nb],
                               v[2].empty() ? nullptr : &v[2][e * 3 * nb], &rows[e], why, sizeof(why));
    if (bad) {
      snprintf(where, sizeof(where), "env %zu: %s", e, why);
      return fail(VNL_ERR_ARG, "vnl_env_set_body_domain: %s: %s", bad, where);
    }
  }
  const std::vector<vreal> tab = body_tables(env, rows);
  int rc = domain_tables(env);
  if (rc != VNL_OK) return rc;
  HIPCHK(hipMemcpy(env->dom + n4, tab.data(), tab.size() * sizeof(vreal), hipMemcpyHostToDevice));
  env->has_body = 1, env->has_dom = 1;
  for (int f = 0; f < 3; f++) env->body_raw[f] = v[f];
  if (env->brng_buf) {  // (a field without bounds takes these values at a redraw)
    const std::vector<double> raw = body_raw_rows(env);
    HIPCHK(hipMemcpy(env->brng_buf + body_ranges_layout(env).raw, raw.data(), raw.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  return VNL_OK;
}

// Ranges of the body-domain redraw at fresh resets (include/vnl.h: vnl_body_domain_ranges).  The contract of
// vnl_env_set_domain_ranges: waits for `stream`, reads the bounds to the host, validates, and only then allocates and writes.
extern "C" int vnl_env_set_body_domain_ranges(vnl_env* env, const vnl_body_domain_ranges* rg, void* stream) {
  if (!env) return fail(VNL_ERR_ARG, "vnl_env_set_body_domain_ranges: null env");
  DeviceGuard guard(env->device);
  if (!guard.ok) return fail(VNL_ERR_HIP, "hipSetDevice failed");
#ifndef VNL_FORKJOIN_DEFINED
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
#else
  (void)stream;
#endif
  if (!rg) return clear_body_ranges(env);
  const DevModel& d = env->dm;
  const size_t B = (size_t)env->B, nb = (size_t)d.nbody_out, nd = (size_t)d.nbody, n4 = B * (2 * d.ncg + d.nu + 2 * d.nv);
  const FuseMap& fm = *env->fmap;
  const struct {
    const char* name;
    size_t w;
    bool nonneg;
    const std::vector<double>& model;
  } fields[3] = {{"body_mass", 1, true, env->mass0}, {"body_inertia", 3, true, env->inertia0}, {"body_ipos", 3, false, env->ipos0}};
  if (rg->shared & ~0x7u) return fail(VNL_ERR_ARG, "vnl_env_set_body_domain_ranges: shared has bits beyond the three fields");
  if (rg->flags & ~VNL_BODY_RANGES_INERTIA_WITH_MASS) return fail(VNL_ERR_ARG, "vnl_env_set_body_domain_ranges: unknown flags");
  for (int f = 0; f < 3; f++)
    if (!rg->lo[f] != !rg->hi[f])
      return fail(VNL_ERR_ARG, "vnl_env_set_body_domain_ranges: %s: lo and hi must both be given or both be null", fields[f].name);
  if ((rg->flags & VNL_BODY_RANGES_INERTIA_WITH_MASS) && !rg->lo[0])
    return fail(VNL_ERR_ARG, "vnl_env_set_body_domain_ranges: INERTIA_WITH_MASS needs ranges for body_mass");
  if (rg->lo[1] && env->inertia0.empty())
    return fail(VNL_ERR_BLOB, "vnl_env_set_body_domain_ranges: body_inertia needs the model's body_inertia and body_iquat sections");
  std::vector<double> lo[3], hi[3];
  for (int f = 0; f < 3; f++) {
    const auto& F = fields[f];
    if (!rg->lo[f]) continue;
    const size_t n = F.w * nb;
    lo[f].resize(n), hi[f].resize(n);
    HIPCHK(hipMemcpy(lo[f].data(), rg->lo[f], n * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hi[f].data(), rg->hi[f], n * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < F.w; k++) lo[f][k] = hi[f][k] = F.model[k];  // row 0 is not read: never drawn
    for (size_t k = 0; k < n; k++)
      if (!(std::isfinite(lo[f][k]) && std::isfinite(hi[f][k]) && lo[f][k] <= hi[f][k] && (!F.nonneg || lo[f][k] >= 0))) {
        char where[96];
        snprintf(where, sizeof(where), "index %zu (lo %g, hi %g)", k, lo[f][k], hi[f][k]);
        return fail(VNL_ERR_ARG, F.nonneg ? "vnl_env_set_body_domain_ranges: %s needs finite 0 <= lo <= hi: %s"
                                          : "vnl_env_set_body_domain_ranges: %s needs finite lo <= hi: %s", F.name, where);
      }
  }
  // The sufficient condition for what the kernel stores (it does not validate): at the LOWER bounds -- a field without bounds:
  // the values it keeps -- every dynamic body that carries dofs has a member mass sum > 0 and a member with three moments > 0,
  // and the total mass is > 0 (include/vnl.h has the reasoning).
  const std::vector<double> raw = body_raw_rows(env);
  const bool per_env = !env->body_raw[0].empty() || !env->body_raw[1].empty() || !env->body_raw[2].empty();
  for (size_t e = 0; e < (per_env ? B : 1); e++) {
    const double *m = lo[0].empty() ? &raw[e * 7 * nb] : lo[0].data(), *mom = lo[1].empty() ? &raw[e * 7 * nb + nb] : lo[1].data();
    double tm = 0;
    for (size_t dyn = 0; dyn < nd; dyn++) {
      double M = 0;
      bool solid = env->inertia0.empty();
      for (int i = fm.mem_start[dyn]; i < fm.mem_start[dyn + 1]; i++) {
        const size_t b = (size_t)fm.mem[i];
        M += m[b], solid = solid || (mom[3 * b] > 0 && mom[3 * b + 1] > 0 && mom[3 * b + 2] > 0);
      }
      tm += M;
      if (dyn == 0 || env->dyn_dofnum[dyn] <= 0) continue;
      char why[200];
      if (!(M > 0)) {
        snprintf(why, sizeof(why), "dynamic body %zu (body %d as given, with what is welded to it) carries dofs and has mass %g", dyn,
                 fm.body_out[dyn], M);
        return fail(VNL_ERR_ARG, "vnl_env_set_body_domain_ranges: body_mass: at the lower bounds %s", why);
      }
      if (!solid) {
        snprintf(why, sizeof(why), "no member of dynamic body %zu (body %d as given) has three moments > 0", dyn, fm.body_out[dyn]);
        return fail(VNL_ERR_ARG, "vnl_env_set_body_domain_ranges: body_inertia: at the lower bounds %s", why);
      }
    }
    if (!(tm > 0)) {
      char why[64];
      snprintf(why, sizeof(why), "total mass %g", tm);
      return fail(VNL_ERR_ARG, "vnl_env_set_body_domain_ranges: body_mass: at the lower bounds %s", why);
    }
  }
  int rc = domain_tables(env);  // (an env without a domain: the tables at the compiled values)
  if (rc != VNL_OK) return rc;
  const BodyRangesLayout L = body_ranges_layout(env);
  if (!env->brng_buf) {  // room for every field, whatever this call gives
    void* p = nullptr;
    HIPCHK(hipMalloc(&p, L.total));
    env->allocs.push_back(p);
    env->brng_buf = (char*)p;
  }
  std::vector<char> buf(L.stage);  // (everything in front of the staging area, which needs no initial value)
  auto put = [&buf](size_t at, const std::vector<double>& src) {
    if (!src.empty()) memcpy(buf.data() + at, src.data(), src.size() * sizeof(double));
  };
  for (int f = 0; f < 3; f++) put(L.lo[f], lo[f]), put(L.hi[f], hi[f]);
  put(L.raw, raw), put(L.out_pos, fm.out_pos), put(L.R_out, fm.R_out), put(L.ifull0, env->ifull0);
  put(L.inertia0, env->inertia0), put(L.R_iq0, env->R_iq0);  // (absent: zeros, see body_raw_rows)
  HIPCHK(hipMemcpy(env->brng_buf, buf.data(), buf.size(), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(env->brng_buf + L.mem_start, fm.mem_start.data(), (nd + 1) * sizeof(int), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(env->brng_buf + L.mem, fm.mem.data(), nb * sizeof(int), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(env->brng_buf + L.body_out, fm.body_out.data(), nd * sizeof(int), hipMemcpyHostToDevice));
  DevBodyRanges br{};
  auto D = [&](size_t at) { return (double*)(env->brng_buf + at); };
  br.shared = rg->shared, br.flags = rg->flags;
  for (int f = 0; f < 3; f++)
    if (!lo[f].empty()) br.lo[f] = D(L.lo[f]), br.hi[f] = D(L.hi[f]);
  br.raw = D(L.raw), br.out_pos = D(L.out_pos), br.R_out = D(L.R_out), br.ifull0 = D(L.ifull0), br.inertia0 = D(L.inertia0);
  br.R_iq0 = D(L.R_iq0), br.stage = D(L.stage);
  br.mem_start = (const int*)(env->brng_buf + L.mem_start), br.mem = (const int*)(env->brng_buf + L.mem);
  br.body_out = (const int*)(env->brng_buf + L.body_out);
  br.body_mass = env->dom + n4, br.body_ipos = br.body_mass + B * nd, br.body_inertia6 = br.body_mass + 4 * B * nd;  // (domain_tables)
  br.total_mass_inv = br.body_mass + 10 * B * nd;
  HIPCHK(hipMemcpy((char*)env->kc + offsetof(KernelConsts, brng), &br, sizeof(DevBodyRanges), hipMemcpyHostToDevice));
  env->has_body_ranges = 1, env->has_body = 1, env->has_dom = 1;
  const int on = ranges_on(env);
  HIPCHK(hipMemcpy((char*)env->kc + offsetof(KernelConsts, rng) + offsetof(DevDomainRanges, on), &on, sizeof(int), hipMemcpyHostToDevice));
  return VNL_OK;
}

#ifdef VNL_PROFILE
// diagnostic build only: read and clear the per-stage cycle sums
extern "C" int vnl_prof_read(unsigned long long* out) {
  unsigned long long z[VNL_NPROF] = {0};
  HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_vnl_prof), sizeof(z)));
  HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_vnl_prof), z, sizeof(z)));
  return VNL_OK;
}
#endif

// ---- rollout post-processing (include/vnl.h: vnl_rollout_post) ----------------------------------
// One workgroup per env: the episode / auto-reset decision is taken once, then every op moves its
// row (coalesced 32-bit words).  HBM-bound: ~5 KB per env.
#ifndef VNL_POST_THREADS
#define VNL_POST_THREADS 256
#endif
__global__ void __launch_bounds__(VNL_POST_THREADS) vnl_post_kernel(vnl_post_desc d) {
  const unsigned e = blockIdx.x, tid = threadIdx.x;
  // every thread evaluates the (cheap) decision itself from the OLD values; thread 0 stores the new ones
  // only after all threads have read them
  float st = d.steps ? ((d.prev_done && d.prev_done[e] != 0.f) ? 0.f : d.steps[e]) + (float)d.action_repeat : 0.f;
  float done = d.done[e];
  bool over = d.steps && st >= (float)d.episode_length;
  float trunc = over ? 1.f - done : 0.f;
  done = over ? 1.f : done;
  __syncthreads();
  if (tid == 0) {
    if (d.steps) d.steps[e] = st;
    if (d.prev_done) d.prev_done[e] = done;
    d.done[e] = done;
    if (d.truncation) d.truncation[e] = trunc;
    if (d.log_reward) d.log_reward[e] = d.reward[e];
    if (d.log_discount) d.log_discount[e] = 1.f - done;
    if (d.log_truncation) d.log_truncation[e] = trunc;
  }
  const bool reset = done != 0.f;
  for (int k = 0; k < d.num_ops; k++) {
    const vnl_post_op& op = d.ops[k];
    const bool from_first = op.first && reset;
    const unsigned* src = (const unsigned*)(from_first ? op.first : op.src) + (size_t)e * op.width;
    unsigned* dst = op.dst ? (unsigned*)op.dst + (size_t)e * op.width : nullptr;
    unsigned* log = op.log ? (unsigned*)op.log + (size_t)e * op.width : nullptr;
    const bool store = dst && (from_first || (const float*)op.dst != op.src);
    for (int i = (int)tid; i < op.width; i += VNL_POST_THREADS) {
      unsigned v = src[i];
      if (store) dst[i] = v;
      if (log) log[i] = v;
    }
  }
}

extern "C" int vnl_rollout_post(const vnl_post_desc* desc, int32_t num_envs, void* stream) {
  int rc = post_desc_check(desc, num_envs);
  if (rc != VNL_OK) return rc;
  hipLaunchKernelGGL(vnl_post_kernel, dim3(num_envs), dim3(VNL_POST_THREADS), 0, (hipStream_t)stream, *desc);
  HIPCHK(hipGetLastError());
  return VNL_OK;
}

// ---- evaluation records (include/vnl.h: vnl_rollout_eval) ---------------------------------------
// One wave per env runs vnl_eval_epilogue (csrc/vnl_env_kernels.h), the code the step waves run in vnl_env_step_post_eval.
__global__ void __launch_bounds__(64) vnl_eval_kernel(vnl_eval_desc d) { vnl_eval_epilogue(d, blockIdx.x, threadIdx.x); }

extern "C" int vnl_rollout_eval(const vnl_eval_desc* desc, int32_t num_envs, void* stream) {
  int rc = eval_desc_check(desc, num_envs);
  if (rc != VNL_OK) return rc;
  hipLaunchKernelGGL(vnl_eval_kernel, dim3(num_envs), dim3(64), 0, (hipStream_t)stream, *desc);
  HIPCHK(hipGetLastError());
  return VNL_OK;
}

// ---- PPO loss head (include/vnl.h: vnl_ppo_head) -------------------------------------------------
// Three launches on the caller's stream: (1) GAE, one column per thread, + advantage / reward statistics;
// (2) the per-sample head, 32 lanes per sample (lane = action component: coalesced rows, shuffle sums),
// per-block partial sums; (3) the partials summed in a fixed order -> metrics (deterministic).
#ifndef VNL_HEAD_THREADS
#define VNL_HEAD_THREADS 256
#define VNL_HEAD_GROUP 32
#define VNL_GROUP_SUM(v) \
  (v += __shfl_xor(v, 16, 32), v += __shfl_xor(v, 8, 32), v += __shfl_xor(v, 4, 32), v += __shfl_xor(v, 2, 32), v += __shfl_xor(v, 1, 32))
#endif
#define VNL_HEAD_MAXBLK 256
#ifndef VNL_FINISH_THREADS
#define VNL_FINISH_THREADS 64
#define VNL_FINISH_SUM(v) \
  (v += __shfl_xor(v, 32), v += __shfl_xor(v, 16), v += __shfl_xor(v, 8), v += __shfl_xor(v, 4), v += __shfl_xor(v, 2), v += __shfl_xor(v, 1))
#endif
__device__ __forceinline__ float vnl_block_sum(float v, float* red) {
  const unsigned tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (unsigned w = VNL_HEAD_THREADS / 2; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  return red[0];
}
__device__ __forceinline__ float vnl_softplus(float x) { return x > 20.f ? x : log1pf(expf(x)); }  // torch F.softplus

// stats: [0] adv mean, [1] adv std (biased), [2] reward variance (biased), then VNL_HEAD_MAXBLK x 4 partial sums
__global__ void __launch_bounds__(VNL_HEAD_THREADS) vnl_ppo_gae_kernel(vnl_ppo_head_args a, float* stats) {
#if VNL_HEAD_THREADS > 1
  __shared__ float red[VNL_HEAD_THREADS];
#else
  float red[1];
#endif
  const int tid = (int)threadIdx.x, T = a.T, B = a.B, N = T * B;
  // compute_gae: reverse scan, intention_losses.py:63-87
  float sa = 0.f, sr = 0.f;
  for (int b = tid; b < B; b += VNL_HEAD_THREADS) {
    float acc = 0.f, v_next = a.bootstrap[b], vs_next = a.bootstrap[b];
    // eight time steps per trip: their 32 loads are in flight together, then the (sequential) recurrence runs on
    // registers -- one load latency per trip instead of one per time step (14 us -> a few for T = 20)
    for (int t1 = T; t1 > 0; t1 -= 8) {
      const int t0 = t1 > 8 ? t1 - 8 : 0;
      float tr[8], dc[8], rw[8], bl[8];
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const int t = t1 - 1 - k, n = (t >= t0 ? t : t0) * B + b;
        tr[k] = a.truncation[n], dc[k] = a.discount[n], rw[k] = a.reward[n], bl[k] = a.baseline[n];
      }
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const int t = t1 - 1 - k;
        if (t >= t0) {
          const int n = t * B + b;
          const float trunc = tr[k], mask = 1.f - trunc;
          const float term = (1.f - dc[k]) * (1.f - trunc);
          const float r = rw[k] * a.reward_scaling, v = bl[k];
          const float delta = (r + a.discounting * (1.f - term) * v_next - v) * mask;
          acc = delta + a.discounting * (1.f - term) * mask * a.gae_lambda * acc;
          const float vs = acc + v;
          const float adv = (r + a.discounting * (1.f - term) * vs_next - v) * mask;
          a.vs[n] = vs, a.advantages[n] = adv;
          sa += adv, sr += r;
          v_next = v, vs_next = vs;
        }
      }
    }
  }
  const float adv_mean = vnl_block_sum(sa, red) / (float)N, r_mean = vnl_block_sum(sr, red) / (float)N;
  float qa = 0.f, qr = 0.f;
  __syncthreads();
  const float inv_n = 1.f / (float)N;
  for (int n = tid; n < N; n += VNL_HEAD_THREADS) {
    const float da = a.advantages[n] - adv_mean, dr = a.reward[n] * a.reward_scaling - r_mean;
    qa += da * da, qr += dr * dr;
    // d v_loss / d baseline (v_loss = 0.25 mean((vs - baseline)^2), vs under stop_gradient: intention_losses.py:137-139) needs
    // nothing of the policy network: it is final here, so the value MLP's backward pass can start while the intention
    // network's forward is still running (csrc/vnl_ppo.hip)
    a.g_baseline[n] = -0.5f * (a.vs[n] - a.baseline[n]) * inv_n;
  }
  const float va = vnl_block_sum(qa, red) / (float)N, vr = vnl_block_sum(qr, red) / (float)N;
  if (tid == 0) stats[0] = adv_mean, stats[1] = sqrtf(va), stats[2] = vr;
}

__global__ void __launch_bounds__(VNL_HEAD_THREADS) vnl_ppo_head_kernel(vnl_ppo_head_args a, float* stats) {
#if VNL_HEAD_THREADS > 1
  __shared__ float red[VNL_HEAD_THREADS];
#else
  float red[1];
#endif
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_amdgcn_s_setprio(3);  // (in a PPO step this launch sits on the intention network's chain, beside the value MLP's GEMMs)
#endif
  const int tid = (int)threadIdx.x, A = a.act, N = a.T * a.B;
  const int lane = tid % VNL_HEAD_GROUP, group = (int)(blockIdx.x * (VNL_HEAD_THREADS / VNL_HEAD_GROUP)) + tid / VNL_HEAD_GROUP;
  const int ngroups = (int)gridDim.x * (VNL_HEAD_THREADS / VNL_HEAD_GROUP);
  const float adv_mean = stats[0], adv_std = stats[1];
  const float inv_n = 1.f / (float)N, half_log_2pi = 0.91893853320467274178f, ln2 = 0.69314718055994530942f;
  const float lo = 1.f - a.clipping_epsilon, hi = 1.f + a.clipping_epsilon;
  float s_pl = 0.f, s_vl = 0.f, s_ent = 0.f;  // counted once per sample (lane 0 of the group)
  for (int n = group; n < N; n += ngroups) {
    const float* lg = a.logits + (size_t)n * 2 * A;
    const float* ra = a.raw_action + (size_t)n * A;
    const float* ee = a.eps_entropy + (size_t)n * A;
    // tanh-Normal log-prob of the stored raw action and entropy estimate at loc + scale * eps, summed over actions
    float tlp = 0.f, ent = 0.f;
    for (int k = lane; k < A; k += VNL_HEAD_GROUP) {
      const float loc = lg[k], scale = (vnl_softplus(lg[A + k]) + a.min_std) * a.var_scale;
      const float x = ra[k], z = (x - loc) / scale, lsc = logf(scale);
      tlp += (-0.5f * z * z - half_log_2pi - lsc) - 2.f * (ln2 - x - vnl_softplus(-2.f * x));
      const float xe = loc + scale * ee[k];
      ent += (0.5f + half_log_2pi + lsc) + 2.f * (ln2 - xe - vnl_softplus(-2.f * xe));
    }
    VNL_GROUP_SUM(tlp);
    VNL_GROUP_SUM(ent);
    float adv = a.advantages[n];
    if (a.normalize_advantage) adv = (adv - adv_mean) / (adv_std + 1e-8f);
    const float rho = expf(tlp - a.behaviour_log_prob[n]);
    const float rc = fminf(fmaxf(rho, lo), hi);
    const float s1 = rho * adv, s2 = rc * adv;
    // d min(s1, s2) / d rho: adv where the unclipped branch is active (ties: both branches agree), else 0
    const float dmin = (s1 < s2 || (s1 == s2 && rho >= lo && rho <= hi)) ? adv : ((s1 == s2) ? 0.5f * adv : 0.f);
    const float g_tlp = -inv_n * dmin * rho;      // d policy_loss / d target_log_prob
    const float g_ent = -a.entropy_cost * inv_n;  // d entropy_loss / d entropy_n
    const float verr = a.vs[n] - a.baseline[n];
    if (lane == 0) s_pl += -fminf(s1, s2), s_vl += verr * verr, s_ent += ent;  // (d v_loss / d baseline: vnl_ppo_gae_kernel)
    float* gl = a.g_logits + (size_t)n * 2 * A;
    for (int k = lane; k < A; k += VNL_HEAD_GROUP) {
      const float sraw = lg[A + k], scale = (vnl_softplus(sraw) + a.min_std) * a.var_scale;
      const float loc = lg[k], z = (ra[k] - loc) / scale, xe = loc + scale * ee[k], th = tanhf(xe);
      const float dscale_ds = a.var_scale / (1.f + expf(-sraw));  // softplus' = sigmoid
      gl[k] = g_tlp * (z / scale) + g_ent * (-2.f * th);
      gl[A + k] = (g_tlp * ((z * z - 1.f) / scale) + g_ent * (1.f / scale - 2.f * th * ee[k])) * dscale_ds;
    }
  }
  // latent KL (kl_divergence: a mean over samples x latent), intention_losses.py:21-23
  float s_kl = 0.f;
  const int NL = N * a.latent;
  const float kscale = a.kl_weight / (float)NL;
  for (int i = (int)(blockIdx.x * VNL_HEAD_THREADS) + tid; i < NL; i += (int)gridDim.x * VNL_HEAD_THREADS) {
    const float mu = a.lat_mean[i], lv = a.lat_logvar[i], ev = expf(lv);
    s_kl += 1.f + lv - mu * mu - ev;
    a.g_lat_mean[i] = kscale * mu;
    a.g_lat_logvar[i] = -0.5f * kscale * (1.f - ev);
  }
  const float p0 = vnl_block_sum(s_pl, red), p1 = vnl_block_sum(s_vl, red), p2 = vnl_block_sum(s_ent, red),
              p3 = vnl_block_sum(s_kl, red);
  if (tid == 0) {
    float* part = stats + 4 + 4 * blockIdx.x;
    part[0] = p0, part[1] = p1, part[2] = p2, part[3] = p3;
  }
}

__global__ void vnl_ppo_finish_kernel(vnl_ppo_head_args a, const float* stats, int nblk) {
  // one 64-lane wave: lane l sums partials l, l+64, ... (fixed order), then a shuffle tree
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_amdgcn_s_setprio(3);
#endif
  const int lane = (int)threadIdx.x;
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  for (int b = lane; b < nblk; b += VNL_FINISH_THREADS)
    for (int k = 0; k < 4; k++) s[k] += stats[4 + 4 * b + k];
  for (int k = 0; k < 4; k++) VNL_FINISH_SUM(s[k]);
  if (lane != 0) return;
  const int N = a.T * a.B;
  const float inv_n = 1.f / (float)N, kscale = a.kl_weight / (float)(N * a.latent);
  const float pl = s[0] * inv_n, vl = 0.25f * s[1] * inv_n, el = -a.entropy_cost * s[2] * inv_n, kl = -0.5f * kscale * s[3];
  a.metrics[0] = pl + vl + el + kl, a.metrics[1] = pl, a.metrics[2] = vl, a.metrics[3] = el, a.metrics[4] = kl;
  a.metrics[5] = 1.f - vl / stats[2], a.metrics[6] = stats[0], a.metrics[7] = stats[1];
}

int vnl_ppo_head_phase_(const vnl_ppo_head_args* a, float* workspace, void* stream, int phase);
extern "C" int vnl_ppo_head(const vnl_ppo_head_args* a, float* workspace, void* stream) {
  if (!a || !workspace || a->T <= 0 || a->B <= 0 || a->act <= 0 || a->latent <= 0)
    return fail(VNL_ERR_ARG, "vnl_ppo_head: bad sizes");
  const void* need[] = {a->logits, a->baseline, a->bootstrap, a->lat_mean, a->lat_logvar, a->raw_action,
                        a->behaviour_log_prob, a->reward, a->truncation, a->discount, a->eps_entropy, a->g_logits,
                        a->g_baseline, a->g_lat_mean, a->g_lat_logvar, a->vs, a->advantages, a->metrics};
  for (const void* p : need)
    if (!p) return fail(VNL_ERR_ARG, "vnl_ppo_head: null buffer");
  return vnl_ppo_head_phase_(a, workspace, stream, 3);
}

// phase bit 1: GAE + statistics (needs the value outputs only); bit 2: per-sample head + the metrics.  vnl_ppo.hip runs
// phase 1 on the value stream while the intention network's forward is still in flight on the other one.
int vnl_ppo_head_phase_(const vnl_ppo_head_args* a, float* workspace, void* stream, int phase) {
  const int groups_per_block = VNL_HEAD_THREADS / VNL_HEAD_GROUP, N = a->T * a->B;
  int nblk = (N + groups_per_block - 1) / groups_per_block;
  if (nblk > VNL_HEAD_MAXBLK) nblk = VNL_HEAD_MAXBLK;
  if (phase & 1) hipLaunchKernelGGL(vnl_ppo_gae_kernel, dim3(1), dim3(VNL_HEAD_THREADS), 0, (hipStream_t)stream, *a, workspace);
  if (phase & 2) {
    hipLaunchKernelGGL(vnl_ppo_head_kernel, dim3(nblk), dim3(VNL_HEAD_THREADS), 0, (hipStream_t)stream, *a, workspace);
    hipLaunchKernelGGL(vnl_ppo_finish_kernel, dim3(1), dim3(VNL_FINISH_THREADS), 0, (hipStream_t)stream, *a, (const float*)workspace, nblk);
  }
  HIPCHK(hipGetLastError());
  return VNL_OK;
}

// ---- minibatch gather (include/vnl.h: vnl_gather_rows): one workgroup per selected row j, all arrays, all t
__global__ void __launch_bounds__(VNL_POST_THREADS) vnl_gather_kernel(vnl_gather_desc d) {
  const int j = (int)blockIdx.x, t = (int)blockIdx.y, tid = (int)threadIdx.x;
  const long long src_row = d.idx[j];
  for (int k = 0; k < d.num_ops; k++) {
    const vnl_gather_op& op = d.ops[k];
    if (t >= op.T) continue;
    const int w = op.width;
    const unsigned* src = (const unsigned*)op.src + ((size_t)t * d.N + src_row) * w;
    unsigned* dst = (unsigned*)op.dst + ((size_t)t * d.M + j) * w;
    for (int c = tid; c < w; c += VNL_POST_THREADS) dst[c] = src[c];
  }
}

extern "C" int vnl_gather_rows(const vnl_gather_desc* d, void* stream) {
  if (!d || !d->idx || d->N <= 0 || d->M <= 0 || d->num_ops < 0 || d->num_ops > VNL_POST_MAX_OPS)
    return fail(VNL_ERR_ARG, "vnl_gather_rows: bad descriptor");
  for (int k = 0; k < d->num_ops; k++)
    if (!d->ops[k].dst || !d->ops[k].src || d->ops[k].T <= 0 || d->ops[k].width <= 0)
      return fail(VNL_ERR_ARG, "vnl_gather_rows: bad op");
  int tmax = 1;
  for (int k = 0; k < d->num_ops; k++) tmax = d->ops[k].T > tmax ? d->ops[k].T : tmax;
  hipLaunchKernelGGL(vnl_gather_kernel, dim3(d->M, tmax), dim3(VNL_POST_THREADS), 0, (hipStream_t)stream, *d);
  HIPCHK(hipGetLastError());
  return VNL_OK;
}

// ---- Adam (include/vnl.h: vnl_adam_step) ----------------------------------------------------------
#ifndef VNL_ADAM_THREADS
#define VNL_ADAM_THREADS 256
#endif
__global__ void __launch_bounds__(VNL_ADAM_THREADS) vnl_adam_kernel(float* p, const float* g, float* mu, float* nu,
                                                                    const long long* count, long long n, double lr_,
                                                                    double b1_, double b2_, double eps_) {
  // the two bias corrections: one thread of the block evaluates the double-precision powers (they were most of this
  // kernel's time when every thread did), the others pick them up from LDS
#if VNL_ADAM_THREADS > 1
  __shared__ float bc[2];
  if (threadIdx.x == 0) {
    const double t = (double)count[0];
    bc[0] = (float)(1.0 - pow(b1_, t)), bc[1] = (float)(1.0 - pow(b2_, t));
  }
  __syncthreads();
  const float bc1 = bc[0], bc2 = bc[1];
#else
  const double t = (double)count[0];
  const float bc1 = (float)(1.0 - pow(b1_, t)), bc2 = (float)(1.0 - pow(b2_, t));
#endif
  const float b1 = (float)b1_, b2 = (float)b2_, omb1 = (float)(1.0 - b1_), omb2 = (float)(1.0 - b2_);
  const float lr = (float)lr_, eps = (float)eps_;
  for (long long i = (long long)blockIdx.x * VNL_ADAM_THREADS + threadIdx.x; i < n;
       i += (long long)gridDim.x * VNL_ADAM_THREADS) {
    const float gi = g[i];
    const float m = b1 * mu[i] + omb1 * gi, v = b2 * nu[i] + omb2 * gi * gi;
    mu[i] = m, nu[i] = v;
    p[i] -= lr * ((m / bc1) / (sqrtf(v / bc2) + eps));
  }
}

extern "C" int vnl_adam_step(float* params, const float* grads, float* mu, float* nu, const int64_t* count, int64_t n,
                             double lr, double b1, double b2, double eps, void* stream) {
  if (!params || !grads || !mu || !nu || !count || n <= 0) return fail(VNL_ERR_ARG, "vnl_adam_step: null argument");
  long long blocks = (n + VNL_ADAM_THREADS - 1) / VNL_ADAM_THREADS;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(vnl_adam_kernel, dim3((unsigned)blocks), dim3(VNL_ADAM_THREADS), 0, (hipStream_t)stream, params,
                     grads, mu, nu, (const long long*)count, (long long)n, lr, b1, b2, eps);
  HIPCHK(hipGetLastError());
  return VNL_OK;
}

// ---- start priorities (include/vnl.h: vnl_start_priority_update) -------------------------------------
// Counters -> table, all in integers: the result is exact and does not depend on the order of any sum.
// a cell's weight in Q16: its smoothed failure rate (f + a) / (n + 2 a) plus the uniform floor
static __host__ __device__ inline uint32_t vnl_priority_weight(uint32_t ended, uint32_t failed, uint32_t prior, uint32_t floor_q16) {
  const uint32_t n = ended < (1u << 20) ? ended : (1u << 20), f = failed < n ? failed : n;
  return (uint32_t)((((uint64_t)f + prior) << 16) / ((uint64_t)n + 2ull * prior)) + floor_q16;
}
#ifndef VNL_FORKJOIN_DEFINED
#define VNL_PRIORITY_THREADS 1024
// One workgroup.  Thread t owns the contiguous cells [t chunk, (t + 1) chunk): it sums their weights, an inclusive scan
// over the wave (shuffles) and over the waves' totals (LDS) turns the sums into 64-bit prefixes, and a second walk over the
// chunk writes cdf[c] = (P_c << 32) / S and the decayed counters.  A thread reads its counters in both walks and writes
// them at the end of the second: no other thread touches them.
__global__ void __launch_bounds__(VNL_PRIORITY_THREADS) vnl_priority_kernel(uint32_t* ended, uint32_t* failed, uint32_t* cdf,
                                                                            int ncell, uint32_t prior, uint32_t floor_q16,
                                                                            int decay_shift) {
  __shared__ unsigned long long wave_total[VNL_PRIORITY_THREADS / 64];
  const int t = (int)threadIdx.x, chunk = (ncell + VNL_PRIORITY_THREADS - 1) / VNL_PRIORITY_THREADS;
  const int c0 = t * chunk < ncell ? t * chunk : ncell, c1 = c0 + chunk < ncell ? c0 + chunk : ncell;
  unsigned long long sum = 0ull;
  for (int c = c0; c < c1; c++) sum += vnl_priority_weight(ended[c], failed[c], prior, floor_q16);
  unsigned long long incl = sum;  // inclusive scan over the wave
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long up = __shfl_up(incl, d, 64);
    if ((t & 63) >= d) incl += up;
  }
  if ((t & 63) == 63) wave_total[t >> 6] = incl;
  __syncthreads();
  unsigned long long before = 0ull, total = 0ull;
  for (int w = 0; w < VNL_PRIORITY_THREADS / 64; w++) {
    const unsigned long long v = wave_total[w];
    before += w < (t >> 6) ? v : 0ull;
    total += v;
  }
  unsigned long long run = before + incl - sum;  // the prefix in front of this thread's chunk
  for (int c = c0; c < c1; c++) {
    const uint32_t n = ended[c], f = failed[c];
    run += vnl_priority_weight(n, f, prior, floor_q16);
    cdf[c] = c == ncell - 1 ? 0xFFFFFFFFu : (uint32_t)((run << 32) / total);
    ended[c] = n >> decay_shift, failed[c] = f >> decay_shift;
  }
}
#endif

// (in the host simulation a plain serial loop instead of the kernel: the CPU tier tests the arithmetic, the GPU tier the kernel)
extern "C" int vnl_start_priority_update(uint32_t* ended, uint32_t* failed, uint32_t* cdf, int32_t ncell, uint32_t prior,
                                         uint32_t floor_q16, int32_t decay_shift, void* stream) {
  if (!ended || !failed || !cdf) return fail(VNL_ERR_ARG, "vnl_start_priority_update: null argument");
  if (ncell < 1 || prior < 1) return fail(VNL_ERR_ARG, "vnl_start_priority_update: ncell and prior must be at least 1");
  if (floor_q16 < 1 || floor_q16 > 65536 || decay_shift < 0 || decay_shift > 31)
    return fail(VNL_ERR_ARG, "vnl_start_priority_update: floor_q16 must be 1..65536, decay_shift 0..31");
  if (ncell > VNL_PRIORITY_MAX_CELLS) return fail(VNL_ERR_UNSUPPORTED, "vnl_start_priority_update: more than 32768 cells");
#ifndef VNL_FORKJOIN_DEFINED
  hipLaunchKernelGGL(vnl_priority_kernel, dim3(1), dim3(VNL_PRIORITY_THREADS), 0, (hipStream_t)stream, ended, failed, cdf,
                     (int)ncell, prior, floor_q16, (int)decay_shift);
  HIPCHK(hipGetLastError());
#else
  (void)stream;
  uint64_t total = 0, run = 0;
  for (int c = 0; c < ncell; c++) total += vnl_priority_weight(ended[c], failed[c], prior, floor_q16);
  for (int c = 0; c < ncell; c++) {
    run += vnl_priority_weight(ended[c], failed[c], prior, floor_q16);
    cdf[c] = c == ncell - 1 ? 0xFFFFFFFFu : (uint32_t)((run << 32) / total);
    ended[c] >>= decay_shift, failed[c] >>= decay_shift;
  }
#endif
  return VNL_OK;
}

// the policy-forward entry points (vnl_policy_*) live in vnl_policy.hip

// What csrc/vnl_record.hip (vnl_env_record: a translation unit of its own) reads of an env, whose struct is private to this
// file: host code only, no kernel of this unit changes with it.
void vnl_env_record_view_(const vnl_env* env, int* device, int* num_envs, int* nq, DevEnv* ev) {
  *device = env->device, *num_envs = env->B, *nq = env->dm.nq, *ev = env->de;
}

#ifdef VNL_FORKJOIN_DEFINED
// host simulation (tests/hostsim): this file is its one translation unit, so the randomised instantiations come in here
#include "vnl_domain.hip"
#include "vnl_eval.hip"
#include "vnl_record.hip"
#endif
