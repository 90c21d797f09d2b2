// learner_features.hip — the opt-in features that have no launcher of their own, and the one place a call refuses a learner for
// carrying a feature: n-step returns (dqnhip_nstep_enable / _get / _debug_read*; k_gather_n: small_kernels.hip.h, launched by
// learner.hip; dqnhip_nstep_validate checks the ring and lives with it, learner_io.hip), target policy smoothing
// (dqnhip_target_noise_enable / _get; k_target_smooth: head_kernels.hip.h, launched by learner.hip), feature_refuse.  Host only.
#include "learner_internal.hip.h"

namespace dqnhip_host {

// The v1 refusals of a learner that carries an opt-in feature, in the fixed order lr policy / weight decay, prioritized replay,
// n-step returns, target smoothing: fails, as `what`, naming the first of `mask` that is enabled on h
int feature_refuse(const H* h, unsigned mask, const char* what) {
  if ((mask & kFeatSched) && (has_policy(h) || has_decay(h)))
    return fail("%s: not available on a learner with lr_policy %s / weight_decay %g in this version (single learner, inside an update only, no diagnostics: DESIGN.md 9)",
                what, dqnhip_lr_policy_name(h->cfg.lr_policy), (double)h->cfg.weight_decay);
  if ((mask & kFeatPer) && h->per) return fail("%s: not available on a learner with prioritized replay (dqnhip_per_enable) in this version", what);
  if ((mask & kFeatNstep) && h->nstep) return fail("%s: not available on a learner with n-step returns (dqnhip_nstep_enable) in this version", what);
  if ((mask & kFeatSmooth) && h->tnoise) return fail("%s: not available on a learner with target smoothing (dqnhip_target_noise_enable) in this version", what);
  return 0;
}
void smooth_free(H* h) {
  TargetNoiseHost* p = h->tnoise;
  if (!p) return;
  hipFree(p->smoothed16); hipFree(p->z16); hipFree(p->counter);
  delete p;
  h->tnoise = nullptr;
}
void nstep_free(H* h) {
  NstepHost* p = h->nstep;
  if (!p) return;
  hipFree(p->disc); hipFree(p->steps); hipFree(p->viol);
  delete p;
  h->nstep = nullptr;
}
static int nstep_ready(dqnhip_handle h, const char* what, const char* name, const void* host) {
  if (!h || !name || !host) return fail("%s: null argument", what);
  if (!h->nstep) return fail("%s: n-step returns are not enabled on this learner (dqnhip_nstep_enable)", what);
  HIPCHK(hipSetDevice(h->cfg.device));
  return 0;
}

}  // namespace dqnhip_host

extern "C" {

// ---- n-step returns (include/dqnhip.h) ----
int dqnhip_nstep_enable(dqnhip_handle h, int32_t n) {
  if (!h) return fail("dqnhip_nstep_enable: null handle (n-step returns are enabled on an existing learner)");
  if (n < 1 || n > kNstepMax) return fail("dqnhip_nstep_enable: n-step returns take n in [1, %d] (got %d)", kNstepMax, n);
  if (dp_grouped(h)) return fail("dqnhip_nstep_enable: n-step returns on a data-parallel learner (dp_world > 1, dqnhip_dp_init) are not supported in this version");
  if (h->next_phase != 0) return fail("dqnhip_nstep_enable: a phased update is in progress (next phase %d)", h->next_phase);
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (!h->nstep) {
    NstepHost* p = new NstepHost();
    h->nstep = p;               // (from here on nstep_free releases whatever was allocated)
    const size_t B = h->B;
    auto alloc = [&](void** d, size_t bytes) -> int { HIPCHK(hipMalloc(d, bytes)); HIPCHK(hipMemset(*d, 0, bytes)); return 0; };
    if (alloc((void**)&p->disc, B * sizeof(double)) || alloc((void**)&p->steps, B * sizeof(int)) || alloc((void**)&p->viol, 2 * sizeof(unsigned long long))) { nstep_free(h); return 1; }
  }
  h->nstep->n = n;
  h->epoch += 1;
  drop_graphs(h);
  return 0;
}

int dqnhip_nstep_get(dqnhip_handle h, int32_t* n) {
  if (!h || !n) return fail("dqnhip_nstep_get: null argument");
  *n = h->nstep ? h->nstep->n : 0;
  return 0;
}

int dqnhip_nstep_debug_read(dqnhip_handle h, const char* name, float* host, size_t count) {
  RC(nstep_ready(h, "dqnhip_nstep_debug_read", name, host));
  const size_t B = h->B;
  const bool is_steps = !strcmp(name, "steps");
  if (!is_steps && strcmp(name, "reward")) return fail("dqnhip_nstep_debug_read: unknown buffer '%s' (reward|steps; \"disc\" is a double: dqnhip_nstep_debug_read_f64)", name);
  if (count < B) return fail("buffer too small for '%s': %zu < %zu", name, count, B);
  HIPCHK(hipMemcpyAsync(host, is_steps ? (const void*)h->nstep->steps : (const void*)h->mb_reward, B * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (is_steps) for (size_t i = 0; i < B; ++i) { int v; memcpy(&v, &host[i], sizeof v); host[i] = (float)v; }
  return 0;
}
int dqnhip_nstep_debug_read_f64(dqnhip_handle h, const char* name, double* host, size_t count) {
  RC(nstep_ready(h, "dqnhip_nstep_debug_read_f64", name, host));
  const size_t B = h->B;
  if (strcmp(name, "disc")) return fail("dqnhip_nstep_debug_read_f64: unknown buffer '%s' (disc)", name);
  if (count < B) return fail("buffer too small for '%s': %zu < %zu", name, count, B);
  HIPCHK(hipMemcpyAsync(host, h->nstep->disc, B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

// ---- target policy smoothing (include/dqnhip.h) ----
int dqnhip_target_noise_enable(dqnhip_handle h, const dqnhip_noise_config* cfg) {
  if (!h) return fail("dqnhip_target_noise_enable: null handle (target smoothing is enabled on an existing learner)");
  if (!cfg) { h->epoch += 1; HIPCHK(hipSetDevice(h->cfg.device)); HIPCHK(hipStreamSynchronize(h->stream)); smooth_free(h); drop_graphs(h); return 0; }
  if (cfg->struct_size != (int32_t)sizeof(dqnhip_noise_config)) return fail("dqnhip_target_noise_enable: dqnhip_noise_config.struct_size mismatch");
  NoiseCfg c{};
  c.sigma_logits = cfg->sigma_logits; c.sigma_params = cfg->sigma_params; c.theta = cfg->theta; c.clip = cfg->clip;
  c.clamp = cfg->clamp ? 1 : 0; c.seed = cfg->seed;
  char msg[256];
  if (noise_config_check(c, msg, sizeof msg)) return fail("dqnhip_target_noise_enable: %s", msg);
  if (c.theta != 1.0f) return fail("dqnhip_target_noise_enable: target smoothing draws white noise: theta must be 1 (got %g)", (double)c.theta);
  if (h->fp16) return fail("dqnhip_target_noise_enable: target smoothing on a learner with precision = DQNHIP_FP16 is not supported in this version");
  if (dp_grouped(h)) return fail("dqnhip_target_noise_enable: target smoothing on a data-parallel learner (dp_world > 1, dqnhip_dp_init) is not supported in this version");
  if (shares_params(h) || h->ring_owner || h->shared_fl[0] || h->shared_fl[1]) return fail("dqnhip_target_noise_enable: target smoothing on a learner that shares parameters or its replay memory is not supported in this version");
  if (h->next_phase != 0) return fail("dqnhip_target_noise_enable: a phased update is in progress (next phase %d)", h->next_phase);
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (!h->tnoise) {
    TargetNoiseHost* p = new TargetNoiseHost();
    h->tnoise = p;              // (from here on smooth_free releases whatever was allocated)
    const size_t n = (size_t)h->B * kAP * sizeof(float);
    auto alloc = [&](void** d, size_t bytes) -> int { HIPCHK(hipMalloc(d, bytes)); HIPCHK(hipMemset(*d, 0, bytes)); return 0; };
    if (alloc((void**)&p->smoothed16, n) || alloc((void**)&p->z16, n) || alloc((void**)&p->counter, sizeof(unsigned long long))) { smooth_free(h); return 1; }
  }
  h->tnoise->cfg = c;
  h->epoch += 1;
  drop_graphs(h);
  return 0;
}
int dqnhip_target_noise_get(dqnhip_handle h, int32_t* enabled, dqnhip_noise_config* cfg) {
  if (!h || !enabled) return fail("dqnhip_target_noise_get: null argument");
  *enabled = h->tnoise ? 1 : 0;
  if (cfg && h->tnoise) {
    const NoiseCfg& c = h->tnoise->cfg;
    *cfg = dqnhip_noise_config{(int32_t)sizeof(dqnhip_noise_config), c.clamp, c.sigma_logits, c.sigma_params, c.theta, c.clip, c.seed};
  }
  return 0;
}

}  // extern "C"
