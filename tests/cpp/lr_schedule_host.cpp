// The host build of lr_rate / lr_current_step / lr_schedule_check (dqn-hfo_amd/csrc/lr_schedule.hip.h): the text the scalars block of
// the gather runs on the device.  Prints, per schedule of the table below, a header line
//   S <policy> <gamma bits> <power bits> <stepsize> <max_iter> <n> <stepvalue>... | <base bits actor> <base bits critic>
// and per iteration 0 .. 2000 (and a few far ones) a line  R <iter> <rate bits actor> <rate bits critic> <current_step>;
// tests/test_lr_schedule_host.py compares them with tests/sched_ref.py.  The create-time refusals are checked here, message by message.
// Plain C++: built once as it is and once with the address and undefined-behaviour sanitizers.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "lr_schedule.hip.h"

using namespace dqnhip;

static int g_fail = 0;
#define CHECK(c)                                                         \
  do {                                                                   \
    if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); g_fail = 1; } \
  } while (0)

static uint32_t bits(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }

static LrSchedule make(int policy, float gamma, float power, int stepsize, int max_iter, int n, const int* sv) {
  LrSchedule s{};
  s.policy = policy; s.base_lr[0] = 1e-5f; s.base_lr[1] = 1e-3f; s.gamma = gamma; s.power = power;
  s.stepsize = stepsize; s.max_iter = max_iter; s.n_stepvalue = n;
  for (int i = 0; sv != nullptr && i < n && i < kLrMaxStepvalues; ++i) s.stepvalue[i] = sv[i];
  return s;
}

static void dump(const LrSchedule& s) {
  printf("S %d %08x %08x %d %d %d", s.policy, bits(s.gamma), bits(s.power), s.stepsize, s.max_iter, s.n_stepvalue);
  for (int i = 0; i < s.n_stepvalue; ++i) printf(" %d", s.stepvalue[i]);
  printf(" | %08x %08x\n", bits(s.base_lr[0]), bits(s.base_lr[1]));
  const int far[] = {2001, 4095, 4096, 65536, 1000000, 2147483647};
  for (int i = 0; i <= 2000 + 6; ++i) {
    const int it = i <= 2000 ? i : far[i - 2001];
    printf("R %d %08x %08x %d\n", it, bits(lr_rate(s, 0, it)), bits(lr_rate(s, 1, it)), lr_current_step(s, it));
  }
}

static bool refused(const LrSchedule& s, float decay, int reg, const char* needle) {
  char msg[256] = "";
  const int rc = lr_schedule_check(s, decay, reg, msg, sizeof msg);
  if (rc == 0 || strstr(msg, needle) == nullptr) { printf("refusal '%s' missing: rc %d, message '%s'\n", needle, rc, msg); return false; }
  return true;
}

int main() {
  const int sv2[] = {3, 5}, sv3[] = {1, 1000, 1999};
  int sv16[16];
  for (int i = 0; i < 16; ++i) sv16[i] = 7 * (i + 1);
  const LrSchedule table[] = {
      make(kLrFixed, 0.f, 0.f, 0, 0, 0, nullptr),
      make(kLrStep, 0.5f, 0.f, 2, 0, 0, nullptr), make(kLrStep, 0.1f, 0.f, 100, 0, 0, nullptr), make(kLrStep, 0.999f, 0.f, 1, 0, 0, nullptr),
      make(kLrExp, 0.5f, 0.f, 0, 0, 0, nullptr), make(kLrExp, 0.999f, 0.f, 0, 0, 0, nullptr), make(kLrExp, 1.001f, 0.f, 0, 0, 0, nullptr),
      make(kLrInv, 0.5f, 1.f, 0, 0, 0, nullptr), make(kLrInv, 1e-4f, 0.75f, 0, 0, 0, nullptr), make(kLrInv, 0.f, 2.f, 0, 0, 0, nullptr),
      make(kLrMultistep, 0.1f, 0.f, 0, 0, 2, sv2), make(kLrMultistep, 0.5f, 0.f, 0, 0, 3, sv3), make(kLrMultistep, 0.9f, 0.f, 0, 0, 16, sv16),
      make(kLrPoly, 0.f, 2.f, 0, 8, 0, nullptr), make(kLrPoly, 0.f, 0.5f, 0, 1000, 0, nullptr), make(kLrPoly, 0.f, 0.f, 0, 1500, 0, nullptr),
      make(kLrSigmoid, 1.f, 0.f, 2, 0, 0, nullptr), make(kLrSigmoid, -0.01f, 0.f, 1000, 0, 0, nullptr), make(kLrSigmoid, 0.05f, 0.f, 0, 0, 0, nullptr),
  };
  for (const LrSchedule& s : table) {
    char msg[256];
    CHECK(lr_schedule_check(s, 0.f, kRegL2, msg, sizeof msg) == 0);
    CHECK(lr_schedule_check(s, 1e-2f, kRegL1, msg, sizeof msg) == 0);
    dump(s);
  }
  // names
  CHECK(!strcmp(lr_policy_name(kLrFixed), "fixed") && !strcmp(lr_policy_name(kLrSigmoid), "sigmoid") && lr_policy_name(-1) == nullptr && lr_policy_name(kLrPolicies) == nullptr);
  // the refusals, each naming the policy (Caffe's wording where it has one)
  const int bad0[] = {0, 5}, bad1[] = {5, 5}, bad2[] = {5, 3}, bad3[] = {-1, 3};
  CHECK(refused(make(7, 0.5f, 0.f, 1, 1, 0, nullptr), 0.f, 0, "Unknown learning rate policy: 7"));
  CHECK(refused(make(-1, 0.5f, 0.f, 1, 1, 0, nullptr), 0.f, 0, "Unknown learning rate policy: -1"));
  CHECK(refused(make(kLrStep, 0.5f, 0.f, 0, 0, 0, nullptr), 0.f, 0, "step: stepsize > 0"));
  CHECK(refused(make(kLrStep, 0.5f, 0.f, -3, 0, 0, nullptr), 0.f, 0, "step: stepsize > 0"));
  CHECK(refused(make(kLrStep, 0.f, 0.f, 2, 0, 0, nullptr), 0.f, 0, "step: gamma > 0"));
  CHECK(refused(make(kLrExp, -0.5f, 0.f, 0, 0, 0, nullptr), 0.f, 0, "exp: gamma > 0"));
  CHECK(refused(make(kLrExp, NAN, 0.f, 0, 0, 0, nullptr), 0.f, 0, "exp: gamma > 0"));
  CHECK(refused(make(kLrMultistep, 0.f, 0.f, 0, 0, 2, sv2), 0.f, 0, "multistep: gamma > 0"));
  CHECK(refused(make(kLrInv, -1e-3f, 1.f, 0, 0, 0, nullptr), 0.f, 0, "inv: gamma >= 0"));
  CHECK(refused(make(kLrMultistep, 0.5f, 0.f, 0, 0, 0, nullptr), 0.f, 0, "multistep: 1 to 16 stepvalues"));
  CHECK(refused(make(kLrMultistep, 0.5f, 0.f, 0, 0, 17, sv16), 0.f, 0, "multistep: 1 to 16 stepvalues"));
  CHECK(refused(make(kLrMultistep, 0.5f, 0.f, 0, 0, 2, bad0), 0.f, 0, "multistep: stepvalues must be positive and strictly increasing"));
  CHECK(refused(make(kLrMultistep, 0.5f, 0.f, 0, 0, 2, bad1), 0.f, 0, "strictly increasing"));
  CHECK(refused(make(kLrMultistep, 0.5f, 0.f, 0, 0, 2, bad2), 0.f, 0, "strictly increasing"));
  CHECK(refused(make(kLrMultistep, 0.5f, 0.f, 0, 0, 2, bad3), 0.f, 0, "positive"));
  CHECK(refused(make(kLrPoly, 0.f, 1.f, 0, 0, 0, nullptr), 0.f, 0, "poly: max_iter > 0"));
  CHECK(refused(make(kLrPoly, 0.f, -1.f, 0, 10, 0, nullptr), 0.f, 0, "poly: power >= 0"));
  CHECK(refused(make(kLrSigmoid, 1.f, 0.f, -1, 0, 0, nullptr), 0.f, 0, "sigmoid: stepsize >= 0"));
  CHECK(refused(make(kLrFixed, 0.f, 0.f, 0, 0, 0, nullptr), -1e-3f, 0, "weight_decay >= 0"));
  CHECK(refused(make(kLrFixed, 0.f, 0.f, 0, 0, 0, nullptr), NAN, 0, "weight_decay >= 0"));
  CHECK(refused(make(kLrFixed, 0.f, 0.f, 0, 0, 0, nullptr), 1e-3f, 2, "Unknown regularization type: 2"));
  CHECK(refused(make(kLrExp, 0.5f, 0.f, 0, 0, 0, nullptr), 0.f, -1, "Unknown regularization type: -1"));
  // a fixed learner reads none of the schedule's other fields
  { char msg[256]; CHECK(lr_schedule_check(make(kLrFixed, -1.f, -1.f, -1, -1, 99, nullptr), 0.f, 0, msg, sizeof msg) == 0); }
  if (g_fail) return 1;
  printf("lr schedule host OK\n");
  return 0;
}
