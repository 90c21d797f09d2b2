// noise_host.cpp — the host build of dqn-hfo_amd/csrc/noise_bodies.hip.h as a stand-alone program: prints normal draws, OU sequences,
// clipped terms and applied columns for a fixed key list as float32 bit patterns; tests/test_noise_host.py compares them with
// tests/noise_ref.py.  Also checks the extreme generator words and the config refusals' wording itself.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "noise_bodies.hip.h"

using namespace dqnhip;

static unsigned bits(float f) { unsigned u; memcpy(&u, &f, 4); return u; }

static int expect_refusal(NoiseCfg c, const char* what) {
  char msg[256] = "";
  if (!noise_config_check(c, msg, sizeof msg) || !strstr(msg, what)) { printf("FAIL: expected a refusal naming '%s', got '%s'\n", what, msg); return 1; }
  return 0;
}

int main() {
  int bad = 0;
  // Z seed ctr lane0 z
  const unsigned long long seeds[3] = {1ull, 0x123456789ABCDEFull, 0xFFFFFFFFFFFFFFFFull};
  const unsigned long long ctrs[4] = {0ull, 1ull, 0xFFFFFFFFull, 0x100000005ull};
  for (unsigned long long seed : seeds)
    for (unsigned long long ctr : ctrs)
      for (int r : {0, 1, 63, 2047})
        for (int j = 0; j < kNO; ++j) {
          const uint32_t lane0 = noise_lane0(r, j);
          printf("Z %llu %llu %u %08x\n", seed, ctr, lane0, bits(noise_normal(seed, ctr, lane0)));
        }
  // E x1 x2 z: the extreme words (u1 = 2^-24, u1 = 1; u2 = 0, u2 just below 1)
  for (uint32_t x1 : {0u, 0xFFu, 0xFFFFFF00u, 0xFFFFFFFFu, 0x80000000u})
    for (uint32_t x2 : {0u, 0xFFFFFFFFu, 0x40000000u, 0x80000000u, 0xC0000000u}) {
      const float z = noise_normal_of(x1, x2);
      if (!isfinite(z) || fabsf(z) > 5.78f) { printf("FAIL: z(%08x, %08x) = %g\n", x1, x2, (double)z); bad = 1; }
      printf("E %u %u %08x\n", x1, x2, bits(z));
    }
  // O theta sigma_logits sigma_params seed worker | then one "o ctr j z x" line per step and column: the state starts at zero
  const float thetas[3] = {1.0f, 0.15f, 0.5f};
  for (int t = 0; t < 3; ++t) {
    NoiseCfg c{}; c.sigma_logits = t == 1 ? 0.0f : 0.05f; c.sigma_params = 0.1f * (float)(t + 1); c.theta = thetas[t]; c.seed = 77 + t;
    const int w = 3 + 20 * t;
    printf("O %08x %08x %08x %llu %d\n", bits(c.theta), bits(c.sigma_logits), bits(c.sigma_params), c.seed, w);
    float x[kNO] = {0};
    for (unsigned long long g = 5; g < 25; ++g)
      for (int j = 0; j < kNO; ++j) {
        const float z = noise_normal(c.seed, g, noise_lane0(w, j));
        x[j] = noise_ou_step(x[j], c.theta, noise_sigma(c, j), z);
        if (c.theta == 1.0f && x[j] != noise_sigma(c, j) * z) { printf("FAIL: theta = 1 is not sigma z\n"); bad = 1; }
        printf("o %llu %d %08x %08x\n", g, j, bits(z), bits(x[j]));
      }
  }
  // C sigma z clip t;  A j clamp v t out
  const float zs[6] = {0.0f, 0.3f, -0.9f, 2.5f, -5.7f, 1.0f};
  for (float sigma : {0.0f, 0.1f, 0.3f})
    for (float z : zs)
      for (float clip : {0.0f, 0.25f, 0.05f}) printf("C %08x %08x %08x %08x\n", bits(sigma), bits(z), bits(clip), bits(noise_clipped(sigma, z, clip)));
  const float vs[7] = {0.0f, -0.999f, 0.73f, 99.5f, -179.9f, 12.345678f, 180.0f};
  const float ts[6] = {0.0f, 0.013f, -0.25f, 0.25f, 1e-3f, -0.0421f};
  for (int j = 0; j < kNO; ++j)
    for (int clamp = 0; clamp < 2; ++clamp)
      for (float v : vs)
        for (float t : ts) printf("A %d %d %08x %08x %08x\n", j, clamp, bits(v), bits(t), bits(noise_apply(v, j, t, clamp)));
  // R j range
  for (int j = 0; j < kNO; ++j) printf("R %d %08x\n", j, bits(noise_range(j)));

  NoiseCfg ok{}; ok.sigma_logits = 0.0f; ok.sigma_params = 0.1f; ok.theta = 0.15f; ok.clip = 0.0f;
  char msg[256];
  if (noise_config_check(ok, msg, sizeof msg)) { printf("FAIL: a valid config was refused: %s\n", msg); bad = 1; }
  NoiseCfg c = ok; c.sigma_logits = -0.1f; bad |= expect_refusal(c, "sigma_logits >= 0");
  c = ok; c.sigma_params = INFINITY; bad |= expect_refusal(c, "sigma_params >= 0");
  c = ok; c.sigma_params = NAN; bad |= expect_refusal(c, "sigma_params >= 0");
  c = ok; c.theta = 0.0f; bad |= expect_refusal(c, "0 < theta <= 1");
  c = ok; c.theta = 1.5f; bad |= expect_refusal(c, "0 < theta <= 1");
  c = ok; c.theta = NAN; bad |= expect_refusal(c, "0 < theta <= 1");
  c = ok; c.clip = -1.0f; bad |= expect_refusal(c, "clip >= 0");
  if (bad) return 1;
  printf("noise host OK\n");
  return 0;
}
