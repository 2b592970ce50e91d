// Counter-based noise shared by the acting kernel (vnl_policy.hip, streams 0..2) and the fresh episode reset (vnl_body.h:
// EnvWaveT::reset_fresh, stream 3); layout in include/vnl.h (vnl_policy_noise, vnl_reset_noise), restated in torch ops in
// ppo_imitation/philox.py.  Compiles for the device and, with the host simulation's VNL_HD, for the CPU.
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef VNL_HD
#define VNL_HD __device__ __forceinline__
#endif

// high 32 bits of a 32 x 32 -> 64 bit product
VNL_HD uint32_t vnl_mulhi32(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umulhi(a, b);
#else
  return (uint32_t)(((uint64_t)a * b) >> 32);
#endif
}

// Philox4x32-10 (Salmon et al. 2011)
VNL_HD void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&x)[4]) {
#pragma unroll
  for (int r = 0; r < 10; r++) {
    const uint32_t hi0 = vnl_mulhi32(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = vnl_mulhi32(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0, c1 = lo1, c2 = hi0 ^ c3 ^ k1, c3 = lo0;
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
  x[0] = c0, x[1] = c1, x[2] = c2, x[3] = c3;
}

// A value uniform between two bounds from one word (the domain redraw, EnvWaveT::redraw_domain): u = (x + 0.5) 2^-32, exact in
// float64 and strictly inside (0, 1), then lo + u * (hi - lo) with the difference, the product and the sum each rounded on
// its own -- no multiply-add contraction, so that the device, the host build and philox.py (domain_draws) give the same bits.
// lo == hi gives lo; lo < hi gives a value in [lo, hi].
VNL_HD double vnl_domain_value(double lo, double hi, uint32_t x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double u = ((double)x + 0.5) * 0x1p-32;
  const double w = hi - lo;
  const double p = u * w;
  return lo + p;
}

// One Box-Muller pair from two words: u = ((x >> 8) + 0.5) 2^-24 = (2 k + 1) 2^-25 with k = x >> 8.  float32 holds u exactly
// for k < 2^23 and 1 - u exactly above, so the upper half goes through ln u = log1p(-(1 - u)) and the angle through
// cos(2 pi u) = cos(2 pi (1 - u)), sin(2 pi u) = -sin(2 pi (1 - u)): no rounding of u anywhere (rounded to 1 it would
// turn a radius of 2.4e-4 into 0).
VNL_HD void box_muller(uint32_t xa, uint32_t xb, float& n0, float& n1) {
  const uint32_t ka = xa >> 8, kb = xb >> 8;
  const bool ha = ka >= (1u << 23), hb = kb >= (1u << 23);
  const float da = (float)(ha ? (1u << 25) - 1u - 2u * ka : 2u * ka + 1u) * 0x1p-25f;  // u or 1 - u, exact
  const float db = (float)(hb ? (1u << 25) - 1u - 2u * kb : 2u * kb + 1u) * 0x1p-25f;
  const float r = sqrtf(-2.f * (ha ? log1pf(-da) : logf(da)));
  float sn, cs;
  sincosf(6.283185307179586f * db, &sn, &cs);
  n0 = r * cs, n1 = r * (hb ? -sn : sn);
}
