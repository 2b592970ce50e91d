// TEST-ONLY stand-alone driver (its own main) for csrc/vnl_record.hip under AddressSanitizer + UndefinedBehaviorSanitizer:
// the entry vnl_env_record and its kernel, compiled for the host against tests/hostsim/stub (a launch = a serial loop), on
// synthetic buffers allocated at their exact sizes, so that a word read or written out of bounds is a report.  The env is a
// stand-in that holds what the entry reads of one (the clip's pose tables and the bounds); the rows are compared with a
// restatement of include/vnl.h above vnl_record_desc.  Built and run by tests/test_record_sanitizer.py as a plain executable.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

struct vnl_env {
  int B, nq, T, C;
  std::vector<float> position, quaternion, joints;
};

#include "../../vnl-brax-imitation_amd/csrc/vnl_record.hip"

static std::string g_msg;
void vnl_set_error_(const char* msg) { g_msg = msg; }
void vnl_env_record_view_(const vnl_env* env, int* device, int* num_envs, int* nq, DevEnv* ev) {
  memset(ev, 0, sizeof(*ev));
  *device = 0, *num_envs = env->B, *nq = env->nq;
  ev->T = env->T, ev->C = env->C;
  ev->position = env->position.data(), ev->quaternion = env->quaternion.data(), ev->joints = env->joints.data();
}

static uint32_t g_rng = 12345u;
static uint32_t rnd() {
  g_rng ^= g_rng << 13, g_rng ^= g_rng >> 17, g_rng ^= g_rng << 5;
  return g_rng;
}
static float as_float(uint32_t w) {
  float f;
  memcpy(&f, &w, 4);
  return f;
}
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
      return 1;                                                       \
    }                                                                 \
  } while (0)

static const uint32_t SENTINEL = 0xC29A0000u;  // -77.0f
static const int STEPS = 6;

// one synthetic case: `B` envs, columns of `widths` (a negative width: a NULL column of that many words), with / without the pose
static int run_case(int B, bool ref, const std::vector<int>& widths, int capacity, int stop_at_done, bool use_index) {
  vnl_env env;
  env.B = B, env.nq = 11, env.T = 9, env.C = 2;
  env.position.resize((size_t)env.C * env.T * 3), env.quaternion.resize((size_t)env.C * env.T * 4);
  env.joints.resize((size_t)env.C * env.T * (env.nq - 7));
  for (auto* v : {&env.position, &env.quaternion, &env.joints})
    for (float& x : *v) x = as_float(rnd());
  std::vector<int32_t> index;
  for (int e = 0; e < B; e++) index.push_back((e * 3 + 1) % B);  // (a permutation when 3 does not divide B)
  index.push_back(index[0]), index.push_back(-1), index.push_back(B);
  const int R = use_index ? (int)index.size() : B;
  int W = ref ? env.nq : 0;
  for (int w : widths) W += w < 0 ? -w : w;
  std::vector<uint32_t> rows((size_t)R * capacity * W, SENTINEL), want(rows);
  std::vector<int32_t> count(R, 0), open(R, 1), wcount(R, 0), wopen(R, 1);
  const int special[4] = {-3, 0, env.T - 1, env.T + 5};
  for (int t = 0; t < STEPS; t++) {
    std::vector<std::vector<uint32_t>> cols;
    for (int w : widths) {
      cols.emplace_back(w < 0 ? 0 : (size_t)B * w);
      for (uint32_t& x : cols.back()) x = rnd();
    }
    std::vector<float> done(B);
    std::vector<int32_t> frame(B), clip(B);
    for (int e = 0; e < B; e++) {
      done[e] = (e != 0 && rnd() % 4 == 0) ? 1.f : 0.f;
      frame[e] = (rnd() & 1) ? special[rnd() % 4] : (int)(rnd() % env.T);
      clip[e] = (int)(rnd() % env.C);
    }
    vnl_record_desc d;
    memset(&d, 0, sizeof(d));
    d.env_index = use_index ? index.data() : nullptr;
    d.done = done.data();
    if (ref) d.ref_frame = frame.data(), d.ref_clip = clip.data();
    d.count = count.data(), d.open = open.data(), d.rows = (float*)rows.data();
    d.num_rec = R, d.capacity = capacity, d.row_width = W, d.stop_at_done = stop_at_done, d.num_cols = (int)widths.size();
    for (size_t k = 0; k < widths.size(); k++) {
      d.cols[k].src = widths[k] < 0 ? nullptr : cols[k].data();
      d.cols[k].width = widths[k] < 0 ? -widths[k] : widths[k];
    }
    CHECK(vnl_env_record(&env, &d, nullptr) == VNL_OK);
    for (int r = 0; r < R; r++) {  // the restatement
      const int e = use_index ? index[r] : r;
      if (e < 0 || e >= B || wopen[r] == 0 || wcount[r] >= capacity) continue;
      uint32_t* row = want.data() + ((size_t)r * capacity + wcount[r]) * W;
      if (ref) {
        const int f = frame[e] < 0 ? 0 : (frame[e] > env.T - 1 ? env.T - 1 : frame[e]);
        const size_t ct = (size_t)clip[e] * env.T + f;
        memcpy(row, &env.position[ct * 3], 12), memcpy(row + 3, &env.quaternion[ct * 4], 16);
        memcpy(row + 7, &env.joints[ct * (env.nq - 7)], 4 * (env.nq - 7));
        row += env.nq;
      }
      for (size_t k = 0; k < widths.size(); k++) {
        const int w = widths[k] < 0 ? -widths[k] : widths[k];
        for (int i = 0; i < w; i++) row[i] = widths[k] < 0 ? 0x7FC00000u : cols[k][(size_t)e * w + i];
        row += w;
      }
      wcount[r]++;
      if (stop_at_done && done[e] != 0.f) wopen[r] = 0;
    }
  }
  CHECK(rows == want && count == wcount && open == wopen);
  return 0;
}

static int run_validation() {
  vnl_env env;
  env.B = 3, env.nq = 11, env.T = 9, env.C = 1;
  env.position.assign(27, 0.f), env.quaternion.assign(36, 0.f), env.joints.assign(36, 0.f);
  std::vector<float> rows(3 * 2 * 15, -77.f), src(9, 1.f);
  std::vector<int32_t> count(3, 0), open(3, 1), frame(3, 0), clip(3, 0);
  auto good = [&]() {
    vnl_record_desc d;
    memset(&d, 0, sizeof(d));
    d.ref_frame = frame.data(), d.ref_clip = clip.data(), d.count = count.data(), d.open = open.data(), d.rows = rows.data();
    d.num_rec = 3, d.capacity = 2, d.row_width = 15, d.stop_at_done = 1, d.num_cols = 2;
    d.cols[0].src = src.data(), d.cols[0].width = 3, d.cols[1].src = nullptr, d.cols[1].width = 1;
    return d;
  };
  auto bad = [&](const vnl_record_desc& d, const char* word) {
    return vnl_env_record(&env, &d, nullptr) == VNL_ERR_ARG && g_msg.find(word) != std::string::npos;
  };
  vnl_record_desc d = good();
  CHECK(vnl_env_record(nullptr, &d, nullptr) == VNL_ERR_ARG && vnl_env_record(&env, nullptr, nullptr) == VNL_ERR_ARG);
  d = good(), d.rows = nullptr;
  CHECK(bad(d, "rows"));
  d = good(), d.count = nullptr;
  CHECK(bad(d, "count"));
  d = good(), d.open = nullptr;
  CHECK(bad(d, "open"));
  d = good(), d.num_rec = 0;
  CHECK(bad(d, "num_rec"));
  d = good(), d.capacity = 0;
  CHECK(bad(d, "capacity"));
  d = good(), d.num_cols = 17;
  CHECK(bad(d, "num_cols"));
  d = good(), d.num_cols = -1;
  CHECK(bad(d, "num_cols"));
  d = good(), d.cols[1].width = 0;
  CHECK(bad(d, "width"));
  d = good(), d.ref_clip = nullptr;
  CHECK(bad(d, "ref_frame and ref_clip"));
  d = good(), d.ref_frame = nullptr;
  CHECK(bad(d, "ref_frame and ref_clip"));
  d = good(), d.row_width = 14;
  CHECK(bad(d, "row_width"));
  for (float x : rows) CHECK(x == -77.f);
  for (int r = 0; r < 3; r++) CHECK(count[r] == 0 && open[r] == 1);
  return 0;
}

int main() {
  const std::vector<std::vector<int>> layouts = {{1}, {1, 63, -64, 65, 130}, {}, {63, -1, 65, 130}};
  const bool refs[4] = {false, false, true, true};
  for (int B : {5, 70})
    for (size_t l = 0; l < layouts.size(); l++)
      for (int capacity : {1, 4})
        for (int stop : {0, 1})
          for (bool use_index : {true, false})
            if (run_case(B, refs[l], layouts[l], capacity, stop, use_index)) return 1;
  if (run_validation()) return 1;
  printf("record ok\n");
  return 0;
}
