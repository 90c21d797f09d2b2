// noise_bodies.hip.h — Gaussian noise on one ActorOutput column, as ONE text that the host and the device both compile (as
// lr_schedule.hip.h is): the standard normal draw from the counter-based generator, the Ornstein-Uhlenbeck step, and the apply-and-clamp
// of one column.  The env kernels (env.hip.h) evaluate it per worker and column, k_target_smooth (head_kernels.hip.h) per minibatch row and column; tests/cpp/noise_host.cpp evaluates the same text on
// the host, and tests/noise_ref.py restates it in numpy.  Bodies only: no kernel.
// Rounding: the normal draw is evaluated in double and rounded to float32 ONCE (as adam_correction and lr_rate are); every other
// operation is a separately rounded float32 operation — the functions switch contraction off, so no fma is formed and numpy float32
// reproduces them bit for bit.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "learner_args.hip.h"      // inverting_bounds: the one table of ActorOutput bounds; kNA, kNO

namespace dqnhip {

// = dqnhip_noise_config (include/dqnhip.h) without its struct_size.  Sigmas and clip are in units of the column's range; clip bounds target smoothing's sigma z (exploration does not read it).
struct NoiseCfg {
  float sigma_logits, sigma_params, theta, clip;
  int clamp, pad;
  unsigned long long seed;
};

// Philox-4x32-10 as philox_u32 (update_bodies.hip.h) has it — the ten rounds restated for both sides, so that the device code of
// the kernels that call philox_u32 stays what it was
__host__ __device__ inline uint32_t noise_philox_u32(uint64_t seed, uint64_t ctr, uint32_t lane) {
  uint32_t c0 = (uint32_t)ctr, c1 = (uint32_t)(ctr >> 32), c2 = lane, c3 = 0x9E3779B9u;
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return c0;
}

// Box-Muller on two draws: u1 in (0, 1] (the logarithm is finite), u2 in [0, 1).  |z| <= sqrt(-2 log 2^-24) = 5.768
__host__ __device__ inline float noise_normal_of(uint32_t x1, uint32_t x2) {
  const double u1 = (double)((x1 >> 8) + 1u) * (1.0 / 16777216.0);
  const double u2 = (double)(x2 >> 8) * (1.0 / 16777216.0);
  return (float)(sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2));
}
// the standard normal draw of the key (seed, ctr, lane0): lanes lane0 and lane0 + 1 of the generator
__host__ __device__ inline float noise_normal(uint64_t seed, uint64_t ctr, uint32_t lane0) {
  return noise_normal_of(noise_philox_u32(seed, ctr, lane0), noise_philox_u32(seed, ctr, lane0 + 1u));
}
// the lane0 of ActorOutput column j of row (worker, minibatch row) r: 32 lanes per row, two per column
__host__ __device__ inline uint32_t noise_lane0(int r, int j) { return (uint32_t)r * 32u + 2u * (uint32_t)j; }

__host__ __device__ inline float noise_sigma(const NoiseCfg& c, int j) { return j < kNA ? c.sigma_logits : c.sigma_params; }
__host__ __device__ inline float noise_range(int j) { float mn, mx; inverting_bounds(j, mn, mx); return mx - mn; }

// x <- (x - theta x) + sigma z.  theta = 1 is white Gaussian noise: x - 1 x is exactly 0
__host__ __device__ inline float noise_ou_step(float x, float theta, float sigma, float z) {
#pragma clang fp contract(off)
  const float decay = theta * x;
  const float kept = x - decay;
  const float kick = sigma * z;
  return kept + kick;
}

// target smoothing's term: sigma z, clipped to [-clip, clip] where clip > 0
__host__ __device__ inline float noise_clipped(float sigma, float z, float clip) {
#pragma clang fp contract(off)
  float t = sigma * z;
  if (clip > 0.0f) t = fminf(fmaxf(t, -clip), clip);
  return t;
}

// column j with the noise t (in units of its range) on it: v + range_j t, clamped to the column's bounds where asked
__host__ __device__ inline float noise_apply(float v, int j, float t, int clamp) {
#pragma clang fp contract(off)
  float mn, mx;
  inverting_bounds(j, mn, mx);
  const float scaled = (mx - mn) * t;
  float out = v + scaled;
  if (clamp) out = fminf(fmaxf(out, mn), mx);
  return out;
}

// what dqnhip_env_set_noise / dqnhip_target_noise_enable refuse; 0: accepted, else the message is in msg
inline int noise_config_check(const NoiseCfg& c, char* msg, size_t n) {
  const double sl = (double)c.sigma_logits, sp = (double)c.sigma_params, th = (double)c.theta, cl = (double)c.clip;
  if (!(sl >= 0.0 && isfinite(sl))) { snprintf(msg, n, "noise: sigma_logits >= 0 and finite required (got %g)", sl); return 1; }
  if (!(sp >= 0.0 && isfinite(sp))) { snprintf(msg, n, "noise: sigma_params >= 0 and finite required (got %g)", sp); return 1; }
  if (!(th > 0.0 && th <= 1.0)) { snprintf(msg, n, "noise: 0 < theta <= 1 required (got %g)", th); return 1; }
  if (!(cl >= 0.0 && isfinite(cl))) { snprintf(msg, n, "noise: clip >= 0 and finite required (got %g)", cl); return 1; }
  return 0;
}

}  // namespace dqnhip
