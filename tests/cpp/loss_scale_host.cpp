// The decision function of dynamic loss scaling (loss_scale_step, dqn-hfo_amd/csrc/learner_args.hip.h) on the host: the same code the
// optimiser launch runs in one lane on the device.  Built and run by tests/test_loss_scale_host.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "learner_args.hip.h"

using namespace dqnhip;

static int g_fail = 0;
#define CHECK(c)                                                         \
  do {                                                                   \
    if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); g_fail = 1; } \
  } while (0)

// the rule of the issue's table, restated
struct Ref { float mult; int good; };
static int ref_step(Ref& s, bool finite, int interval, float lo, float hi) {
  if (!finite) {
    s.good = 0;
    if (s.mult == lo) return 1;                 // at the floor: report, stay
    s.mult /= 2;
    return 0;
  }
  s.good += 1;
  if (interval > 0 && s.good == interval) { s.mult = std::fmin(2 * s.mult, hi); s.good = 0; }
  return 0;
}

int main() {
  const float lo = 1.0f / 4096.0f;
  {   // halving on a non-finite norm, good reset on a skip, no flag above the floor
    const LossScaleCfg c{2000, lo, 1.0f};
    const LossScaleStep r = loss_scale_step(LossScaleState{1.0f, 17}, false, c);
    CHECK(r.st.mult == 0.5f && r.st.good == 0 && r.raise_flag == 0 && r.backed_off == 1 && r.grew == 0);
    const LossScaleStep r2 = loss_scale_step(r.st, false, c);
    CHECK(r2.st.mult == 0.25f && r2.st.good == 0 && r2.raise_flag == 0 && r2.backed_off == 1);
  }
  {   // the flag only at the floor; the multiplier stays there
    const LossScaleCfg c{0, 0.25f, 1.0f};
    LossScaleState s{1.0f, 0};
    int raised = 0;
    for (int i = 0; i < 6; ++i) {
      const LossScaleStep r = loss_scale_step(s, false, c);
      CHECK(r.raise_flag == (i >= 2 ? 1 : 0));
      CHECK(r.backed_off == (i < 2 ? 1 : 0));
      raised += r.raise_flag; s = r.st;
      CHECK(s.mult >= 0.25f && s.good == 0);
    }
    CHECK(s.mult == 0.25f && raised == 4);
    const LossScaleStep ok = loss_scale_step(s, true, c);      // a finite step at the floor is just a step
    CHECK(ok.raise_flag == 0 && ok.st.mult == 0.25f && ok.st.good == 1);
  }
  {   // growth exactly at good == interval, good wraps
    const LossScaleCfg c{4, lo, 1.0f};
    LossScaleState s{0.125f, 0};
    for (int i = 1; i <= 3; ++i) { const LossScaleStep r = loss_scale_step(s, true, c); CHECK(r.st.mult == 0.125f && r.st.good == i && r.grew == 0); s = r.st; }
    const LossScaleStep r = loss_scale_step(s, true, c);
    CHECK(r.st.mult == 0.25f && r.st.good == 0 && r.grew == 1 && r.raise_flag == 0 && r.backed_off == 0);
    const LossScaleStep skip = loss_scale_step(LossScaleState{0.125f, 3}, false, c);      // a skip one short of the interval starts the count again
    CHECK(skip.st.good == 0 && skip.st.mult == 0.0625f);
    const LossScaleStep after = loss_scale_step(skip.st, true, c);
    CHECK(after.st.good == 1 && after.st.mult == 0.0625f);
  }
  {   // interval 0: never grows, good keeps counting
    const LossScaleCfg c{0, lo, 1.0f};
    LossScaleState s{0.5f, 0};
    for (int i = 1; i <= 5000; ++i) { const LossScaleStep r = loss_scale_step(s, true, c); s = r.st; CHECK(r.grew == 0); }
    CHECK(s.mult == 0.5f && s.good == 5000);
  }
  {   // the cap
    const LossScaleCfg c{1, lo, 0.25f};
    LossScaleState s{0.0625f, 0};
    const float want[5] = {0.125f, 0.25f, 0.25f, 0.25f, 0.25f};
    for (int i = 0; i < 5; ++i) {
      const LossScaleStep r = loss_scale_step(s, true, c);
      CHECK(r.st.mult == want[i] && r.st.good == 0 && r.grew == (i < 2 ? 1 : 0));
      s = r.st;
    }
    const LossScaleCfg c8{2, lo, 8.0f};                        // a cap above 1
    s = LossScaleState{4.0f, 1};
    const LossScaleStep r = loss_scale_step(s, true, c8);
    CHECK(r.st.mult == 8.0f && r.grew == 1);
    CHECK(loss_scale_step(LossScaleState{8.0f, 1}, true, c8).st.mult == 8.0f);
  }
  // 10 000 random steps against the restatement, three configurations
  const int intervals[3] = {0, 3, 50};
  const float los[3] = {lo, 1.0f / 16.0f, 0.5f}, his[3] = {1.0f, 8.0f, 1.0f};
  const int pct_bad[3] = {30, 45, 10};
  for (int k = 0; k < 3; ++k) {
    const LossScaleCfg c{intervals[k], los[k], his[k]};
    LossScaleState s{1.0f, 0};
    Ref ref{1.0f, 0};
    uint64_t x = 0x9E3779B97F4A7C15ull + (uint64_t)k;
    int flags = 0, backoffs = 0, growths = 0;
    for (int i = 0; i < 10000; ++i) {
      x = x * 6364136223846793005ull + 1442695040888963407ull;
      const bool finite = (int)((x >> 33) % 100) >= pct_bad[k];
      const float before = ref.mult;
      const int want_flag = ref_step(ref, finite, c.growth_interval, c.min_mult, c.max_mult);
      const LossScaleStep r = loss_scale_step(s, finite, c);
      s = r.st;
      if (!(s.mult == ref.mult && s.good == ref.good && r.raise_flag == want_flag)) { printf("sequence %d diverges at step %d\n", k, i); g_fail = 1; break; }
      CHECK(r.backed_off == (ref.mult < before ? 1 : 0) && r.grew == (ref.mult > before ? 1 : 0));
      CHECK(s.mult >= c.min_mult && s.mult <= c.max_mult);
      flags += r.raise_flag; backoffs += r.backed_off; growths += r.grew;
    }
    printf("sequence %d: mult %g good %d, %d reports, %d backoffs, %d growths\n", k, (double)s.mult, s.good, flags, backoffs, growths);
    CHECK(backoffs > 0);
    if (c.growth_interval == 3) CHECK(growths > 0);
  }
  if (g_fail) return 1;
  printf("loss scale host OK\n");
  return 0;
}
