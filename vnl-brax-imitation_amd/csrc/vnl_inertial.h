// The inertial fold of the welded bodies, one expression for the host and the device: the model upload, vnl_env_set_body_domain
// (vnl_lib.hip) and the body-domain redraw of a fresh reset (EnvWaveT::redraw_body_domain) all call the helpers below.  float64
// throughout and no multiply-add contraction, so that host and device round alike; the callers cast to vreal last.
//
// Per body AS GIVEN (vnl_fold_member) a record of VNL_FOLD_REC doubles: its mass m, m c (c: its centre of mass in the frame of
// the dynamic body it rides on), its full inertia turned into that frame and moved to that frame's origin (parallel axes), and
// its own ipos.  Per DYNAMIC body (vnl_fold_gather) the records of its members are summed in ascending body index, every
// accumulator from 0.0 -- the order in which a loop over the bodies as given scatters into them -- and vnl_fold_finish shifts
// the sum back to the fused centre of mass.
#pragma once
#include "vnl_types.h"

#if defined(__clang__)
#define VNL_FP_EXACT _Pragma("clang fp contract(off)")
#else
#define VNL_FP_EXACT
#endif

#define VNL_FOLD_REC 16 /* m | m c [3] | J about the dynamic body's origin [9] | ipos [3] */
#define VNL_FOLD_ACC 13 /* M | sum m c [3] | sum J [9] */

/* (The rotation matrices of out_quat and of the compiled body_iquat come from the host's qmat_d, once: the device reads them.)
 * The full inertia of a body as given from its principal moments: the compiled full inertia plus
 * R(iquat) diag(moments - compiled moments) R(iquat)', exactly the compiled one where all three differences are zero. */
VNL_HOST_DEVICE inline void vnl_full_inertia(const double* full0, const double* Riq, const double* moments, const double* moments0,
                                             double* full) {
  VNL_FP_EXACT
  for (int k = 0; k < 9; k++) full[k] = full0[k];
  double dl[3];
  for (int k = 0; k < 3; k++) dl[k] = moments[k] - moments0[k];
  if (dl[0] == 0 && dl[1] == 0 && dl[2] == 0) return;
  for (int r = 0; r < 3; r++)
    for (int q = 0; q < 3; q++) {
      double v = 0;
      for (int a = 0; a < 3; a++) v += Riq[3 * r + a] * dl[a] * Riq[3 * q + a];
      full[3 * r + q] += v;
    }
}

/* One body's record: R, opos its fixed transform in the frame of its dynamic body; m, ipos, I (full, 9) its inertial fields */
VNL_HOST_DEVICE inline void vnl_fold_member(const double* R, const double* opos, double m, const double* ipos, const double* I,
                                            double* rec) {
  VNL_FP_EXACT
  double c[3];
  for (int r = 0; r < 3; r++) c[r] = opos[r] + (R[3 * r] * ipos[0] + R[3 * r + 1] * ipos[1] + R[3 * r + 2] * ipos[2]);
  const double cc = c[0] * c[0] + c[1] * c[1] + c[2] * c[2];
  rec[0] = m;
  for (int k = 0; k < 3; k++) rec[1 + k] = m * c[k];
  for (int r = 0; r < 3; r++)
    for (int q = 0; q < 3; q++) {
      double v = 0;  // (R I R')(r, q)
      for (int a = 0; a < 3; a++)
        for (int e = 0; e < 3; e++) v += R[3 * r + a] * I[3 * a + e] * R[3 * q + e];
      rec[4 + 3 * r + q] = v + m * ((r == q ? cc : 0.0) - c[r] * c[q]);
    }
  for (int k = 0; k < 3; k++) rec[13 + k] = ipos[k];
}

/* The sums of one dynamic body over its members (ascending body indices), every accumulator from 0.0 */
VNL_HOST_DEVICE inline void vnl_fold_gather(const int* members, int n, const double* recs, double* acc) {
  VNL_FP_EXACT
  for (int k = 0; k < VNL_FOLD_ACC; k++) acc[k] = 0.0;
  for (int i = 0; i < n; i++) {
    const double* rec = recs + (size_t)VNL_FOLD_REC * members[i];
    for (int k = 0; k < VNL_FOLD_ACC; k++) acc[k] += rec[k];
  }
}

/* Fused centre of mass (a massless body keeps its own ipos) and the full inertia about it */
VNL_HOST_DEVICE inline void vnl_fold_finish(const double* acc, const double* own_ipos, double* nip, double* nI) {
  VNL_FP_EXACT
  const double M = acc[0];
  double c[3];
  if (M > 0)
    for (int k = 0; k < 3; k++) c[k] = acc[1 + k] / M;
  else
    for (int k = 0; k < 3; k++) c[k] = own_ipos[k];
  const double cc = c[0] * c[0] + c[1] * c[1] + c[2] * c[2];
  for (int k = 0; k < 3; k++) nip[k] = c[k];
  for (int r = 0; r < 3; r++)
    for (int q = 0; q < 3; q++) nI[3 * r + q] = acc[4 + 3 * r + q] - M * ((r == q ? cc : 0.0) - c[r] * c[q]);
}

/* full inertia [9] -> xx yy zz xy xz yz */
VNL_HOST_DEVICE inline void vnl_pack_inertia6(const double* s, double* o) {
  o[0] = s[0], o[1] = s[4], o[2] = s[8], o[3] = s[1], o[4] = s[2], o[5] = s[5];
}

/* 1 / total mass: the serial sum in ascending order (elements `stride` apart) */
VNL_HOST_DEVICE inline double vnl_total_mass_inv(const double* mass, int n, int stride = 1) {
  VNL_FP_EXACT
  double tm = 0;
  for (int k = 0; k < n; k++) tm += mass[(size_t)k * stride];
  return 1.0 / tm;
}
