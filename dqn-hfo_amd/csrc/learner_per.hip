// learner_per.hip — prioritized replay (include/dqnhip.h; the kernels and the tree's definition: per_kernels.hip.h): the per_*
// launchers and helpers the other units call (learner_internal.hip.h) and the dqnhip_per_* API.  dqnhip_per_refresh is a replay
// sweep: learner_eval.hip.
#include "learner_internal.hip.h"
#include "per_kernels.hip.h"

namespace dqnhip_host {

static PerTree per_tree(const PerHost* p) {
  PerTree t{};
  for (int k = 0; k < kPerMaxLevels; ++k) { t.lvl[k] = p->tree.lvl[k]; t.n[k] = p->tree.n[k]; }
  t.levels = p->tree.levels;
  return t;
}
// one k_per_sync (src null) or one set pass (src: n_set leaves for the logical range from `first`), on the learner's stream
static int per_sync_launch(H* h, const float* src, int first, int n_set) {
  PerHost* p = h->per;
  const long long cap = h->ring.cap;
  // waves stride over the level-1 nodes above the slots that may change: what is pending (twice: as many may have been evicted) —
  // any grid is correct
  const long long touched = src ? n_set : std::min(2 * (p->pending + h->per_env_slack), 2 * cap);
  const int blocks = (int)std::max(1LL, std::min(1024LL, (touched / 64 + 8 + 3) / 4));
  PerSyncArgs a{per_tree(p), (PerDev*)p->dev, (const DevState*)h->st, (int)cap, src, first, n_set};
  HIPCHK(launch(timed(h, kFamPerSync, h->stream), k_per_sync, dim3(blocks), dim3(256), 0, a));
  if (!src) { p->pending = 0; p->changed = false; p->syncs += 1; }
  return 0;
}
int per_sync_if_needed(H* h) {
  if (!h->per || !(h->per->changed || h->per->pending > 0)) return 0;
  return per_sync_launch(h, nullptr, 0, 0);
}
// The sync reads the ring's (head, size) as they are at ITS place in the stream, so the bound only has to hold between two syncs:
// appended since the last one (+ what env front-ends may still hold back from before it) + this call's n stays below cap
void per_note_append(H* h, long long n) {
  H* o = RO(h);
  if (!o->per) return;
  PerHost* p = o->per;
  // (an AddTransitions into a full deque evicts one more than it appends: cap - 2)
  if (p->pending > 0 && p->pending + o->per_env_slack + n > (long long)o->ring.cap - 2) per_sync_launch(o, nullptr, 0, 0);
  p->pending += n; p->changed = true;
}
int per_sample_launch(H* h) {
  PerHost* p = h->per;
  PerSampleArgs a{per_tree(p), (const DevState*)h->st, (const DevState*)h->st, h->ring.cap, h->B, 1.0f / (float)h->B, p->cfg.seed,
                  1, 0ull, p->idx, p->slot, p->prob, p->u};
  HIPCHK(launch(timed(h, kFamPerSample, h->stream), k_per_sample, dim3((h->B + 3) / 4), dim3(256), 0, a));
  return 0;
}
int per_fill_launch(H* h, const int* idx_dev) {
  PerHost* p = h->per;
  HIPCHK(launch(h->stream, k_per_fill, dim3((h->B + 255) / 256), dim3(256), 0, per_tree(p), (const DevState*)h->st, h->ring.cap, h->B, idx_dev, p->slot, p->prob));
  return 0;
}
int per_update_launch(H* h) {
  PerHost* p = h->per;
  PerUpdateArgs a{per_tree(p), (PerDev*)p->dev, h->B, p->slot, p->td_abs, p->cfg.eps, p->cfg.alpha};
  HIPCHK(launch(timed(h, kFamPerUpdate, h->stream), k_per_update, dim3(1), dim3(256), 0, a));
  return 0;
}
int per_clear(H* h) {
  H* o = RO(h);
  if (!o->per) return 0;
  PerHost* p = o->per;
  HIPCHK(hipMemsetAsync(p->tree_base, 0, p->tree_floats * sizeof(float), h->stream));
  HIPCHK(hipMemsetAsync(&((PerDev*)p->dev)->head_seen, 0, 2 * sizeof(int), h->stream));     // head_seen, size_seen: the empty window at slot 0
  p->pending = 0; p->changed = false;
  return 0;
}
// for the units that do not see PerDev (learner_state.hip, and learner_save_async.hip, whose pack kernel reads it on the device)
const float* per_p_max_dev(const H* h) { return h->per ? &((const PerDev*)h->per->dev)->p_max : nullptr; }
// dqnhip_save_state / dqnhip_load_state (learner_state.hip, which launches nothing)
int per_read_p_max(H* h, float* p_max) {
  HIPCHK(hipMemcpyAsync(p_max, per_p_max_dev(h), sizeof *p_max, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}
// The tree of a window of `size` transitions at physical slot `head` (the ring's DevState already says so) with the given leaves, logical
// order: everything zero, the leaves and the level-1 nodes above them by the set pass, every node of the levels above recomputed — a
// node is the sum of its 64 children in one fixed order whoever computes it, so these are the bits of the tree the leaves were read from
int per_restore(H* h, const float* leaves, int head, int size, float p_max, long long syncs) {
  PerHost* p = h->per;
  HIPCHK(hipStreamSynchronize(h->stream));         // the staging buffer may still be in flight
  HIPCHK(hipMemsetAsync(p->tree_base, 0, p->tree_floats * sizeof(float), h->stream));
  const PerDev d{p_max, head, size, 0};
  HIPCHK(hipMemcpyAsync(p->dev, &d, sizeof d, hipMemcpyHostToDevice, h->stream));
  if (size > 0) {
    RC(ensure_stage(h, (size_t)size * sizeof(float)));
    HIPCHK(hipMemcpyAsync(h->stage_dev, leaves, (size_t)size * sizeof(float), hipMemcpyHostToDevice, h->stream));
    RC(per_sync_launch(h, (const float*)h->stage_dev, 0, size));
  }
  HIPCHK(hipStreamSynchronize(h->stream));         // (d is on this stack, leaves the caller's)
  p->pending = 0; p->changed = false; p->syncs = syncs;
  return 0;
}
void per_free(H* h) {
  PerHost* p = h->per;
  if (!p) return;
  hipFree(p->tree_base); hipFree(p->dev); hipFree(p->idx); hipFree(p->slot);
  hipFree(p->prob); hipFree(p->u); hipFree(p->w); hipFree(p->td_abs);
  delete p;
  h->per = nullptr;
}
static float per_beta_host(const PerHost* p, int critic_iter) {
  if (p->cfg.beta_anneal_iters <= 0) return p->cfg.beta0;
  return std::min(1.0f, p->cfg.beta0 + (1.0f - p->cfg.beta0) * ((float)critic_iter / (float)p->cfg.beta_anneal_iters));
}
// brings the tree in step with the ring; the caller holds no RingUse (a prioritized learner shares no ring)
static int per_ready(dqnhip_handle h, const char* what) {
  if (!h) return fail("%s: null handle", what);
  if (!h->per) return fail("%s: prioritized replay is not enabled on this learner (dqnhip_per_enable)", what);
  HIPCHK(hipSetDevice(h->cfg.device));
  RC(per_sync_if_needed(h));
  return 0;
}

}  // namespace dqnhip_host

extern "C" {

void dqnhip_per_default_config(dqnhip_per_config* c) {
  if (!c) return;
  memset(c, 0, sizeof *c);
  c->struct_size = (int32_t)sizeof *c;
  // the customary values of Schaul et al. 2016 (proportional variant) — not measured on this workload
  c->alpha = 0.6f; c->beta0 = 0.4f; c->beta_anneal_iters = 0; c->eps = 1e-6f; c->seed = 0x5045525F53454544ull;
}

int dqnhip_per_enable(dqnhip_handle h, const dqnhip_per_config* c) {
  // (the config first: a caller built against another header learns so whatever it passes as the handle)
  if (!c) return fail("dqnhip_per_enable: null config");
  if (c->struct_size != (int32_t)sizeof(dqnhip_per_config)) return fail("dqnhip_per_config.struct_size %d != %zu (ABI mismatch)", c->struct_size, sizeof(dqnhip_per_config));
  if (!h) return fail("dqnhip_per_enable: null handle (prioritized replay is enabled on an existing learner)");
  if (h->per) return fail("dqnhip_per_enable: prioritized replay is already enabled on this learner");
  if (!(c->alpha >= 0.0f && c->alpha <= 1.0f)) return fail("dqnhip_per_enable: alpha %g outside [0, 1]", (double)c->alpha);
  if (!(c->beta0 >= 0.0f && c->beta0 <= 1.0f)) return fail("dqnhip_per_enable: beta0 %g outside [0, 1]", (double)c->beta0);
  if (c->beta_anneal_iters < 0) return fail("dqnhip_per_enable: beta_anneal_iters %d < 0", c->beta_anneal_iters);
  if (!(c->eps >= 0.0f) || !std::isfinite(c->eps)) return fail("dqnhip_per_enable: eps %g must be finite and >= 0", (double)c->eps);
  if (shares_ring(h) || h->sharers) return fail("dqnhip_per_enable: prioritized replay on a learner that shares a replay memory is not supported in this version");
  if (dp_grouped(h)) return fail("dqnhip_per_enable: prioritized replay on a data-parallel learner (dp_world > 1, dqnhip_dp_init) is not supported in this version");
  if (h->next_phase != 0) return fail("dqnhip_per_enable: a phased update is in progress (next phase %d)", h->next_phase);
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipStreamSynchronize(h->stream));
  PerHost* p = new PerHost();
  p->cfg = *c;
  h->per = p;                 // (from here on per_free releases whatever was allocated)
  auto bail = [&](int rc) { per_free(h); return rc; };
  // levels: n[0] = cap leaves, n[k + 1] = ceil(n[k] / 64) down to one node; every level stored padded to a multiple of 64
  size_t off[kPerMaxLevels] = {0}, total = 0;
  int k = 0;
  p->tree.n[0] = h->ring.cap;
  for (;; ++k) {
    off[k] = total; total += round_up_z((size_t)p->tree.n[k], 64);
    if (k > 0 && p->tree.n[k] == 1) break;
    if (k + 1 >= kPerMaxLevels) return bail(fail("dqnhip_per_enable: replay capacity %d needs more tree levels than %d", h->ring.cap, kPerMaxLevels - 1));
    p->tree.n[k + 1] = (p->tree.n[k] + 63) / 64;
  }
  p->tree.levels = k; p->tree_floats = total;
  auto alloc = [&](void** d, size_t bytes) -> int { HIPCHK(hipMalloc(d, bytes)); HIPCHK(hipMemsetAsync(*d, 0, bytes, h->stream)); return 0; };
  if (alloc((void**)&p->tree_base, total * sizeof(float))) return bail(1);
  for (int i = 0; i <= k; ++i) p->tree.lvl[i] = p->tree_base + off[i];
  const size_t B = h->B;
  if (alloc(&p->dev, sizeof(PerDev)) || alloc((void**)&p->idx, B * 4) || alloc((void**)&p->slot, B * 4) || alloc((void**)&p->prob, B * 4) ||
      alloc((void**)&p->u, B * 4) || alloc((void**)&p->w, B * 4) || alloc((void**)&p->td_abs, B * 4)) return bail(1);
  const PerDev init{1.0f, 0, 0, 0};
  HIPCHK(hipMemcpyAsync(p->dev, &init, sizeof init, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));       // (init is on this stack)
  // the transitions already there: seen as the empty window at the ring's head, so the first sync appends all of them at p_max
  RC(refresh_ring(h));
  { const int hs[2] = {(int)h->h_head, 0}; HIPCHK(hipMemcpy(&((PerDev*)p->dev)->head_seen, hs, sizeof hs, hipMemcpyHostToDevice)); }
  p->pending = h->h_size; p->changed = true;
  h->epoch += 1;
  drop_graphs(h);
  return 0;
}

int dqnhip_per_get_state(dqnhip_handle h, dqnhip_per_state* out) {
  if (!h || !out) return fail("dqnhip_per_get_state: null argument");
  if (out->struct_size != (int32_t)sizeof(dqnhip_per_state)) return fail("dqnhip_per_state.struct_size %d != %zu (ABI mismatch)", out->struct_size, sizeof(dqnhip_per_state));
  memset(out, 0, sizeof *out);
  out->struct_size = (int32_t)sizeof *out;
  if (!h->per) return 0;
  RC(per_ready(h, "dqnhip_per_get_state"));
  PerHost* p = h->per;
  PerDev d{}; float total = 0.0f; DevState s{};
  HIPCHK(hipMemcpyAsync(&d, p->dev, sizeof d, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(&total, p->tree.lvl[p->tree.levels], sizeof total, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(&s, h->st, sizeof s, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  out->enabled = 1; out->levels = p->tree.levels; out->size = d.size_seen;
  out->total = total; out->p_max = d.p_max; out->beta_now = per_beta_host(p, s.critic_iter);
  out->next_counter = s.update_counter; out->syncs = p->syncs;
  return 0;
}

int dqnhip_per_get_priorities(dqnhip_handle h, int32_t first, int32_t n, float* leaf_host) {
  RC(per_ready(h, "dqnhip_per_get_priorities"));
  if (!leaf_host) return fail("dqnhip_per_get_priorities: null buffer");
  RC(refresh_ring(h));
  if (n < 1 || first < 0 || (long long)first + n > h->h_size) return fail("dqnhip_per_get_priorities: range [%d,%d) outside [0,%lld)", first, first + n, h->h_size);
  const long long cap = h->ring.cap, s0 = (h->h_head + first) % cap;
  const long long n0 = std::min<long long>(n, cap - s0);
  HIPCHK(hipMemcpyAsync(leaf_host, h->per->tree.lvl[0] + s0, n0 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  if (n0 < n) HIPCHK(hipMemcpyAsync(leaf_host + n0, h->per->tree.lvl[0], (n - n0) * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

int dqnhip_per_set_priorities(dqnhip_handle h, int32_t first, int32_t n, const float* leaf_host) {
  RC(per_ready(h, "dqnhip_per_set_priorities"));
  if (!leaf_host) return fail("dqnhip_per_set_priorities: null buffer");
  RC(refresh_ring(h));
  if (n < 1 || first < 0 || (long long)first + n > h->h_size) return fail("dqnhip_per_set_priorities: range [%d,%d) outside [0,%lld)", first, first + n, h->h_size);
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(leaf_host[i]) || leaf_host[i] < 0.0f) return fail("dqnhip_per_set_priorities: priority %d = %g is not finite and >= 0", i, (double)leaf_host[i]);
  h->epoch += 1;
  HIPCHK(hipStreamSynchronize(h->stream));       // the staging buffer may still be in flight
  RC(ensure_stage(h, (size_t)n * sizeof(float)));
  HIPCHK(hipMemcpyAsync(h->stage_dev, leaf_host, (size_t)n * sizeof(float), hipMemcpyHostToDevice, h->stream));
  RC(per_sync_launch(h, (const float*)h->stage_dev, first, n));
  HIPCHK(hipStreamSynchronize(h->stream));       // (leaf_host is the caller's)
  return 0;
}

int dqnhip_per_sample(dqnhip_handle h, uint64_t counter, int32_t n_batches, int32_t* idx_host, float* prob_host) {
  RC(per_ready(h, "dqnhip_per_sample"));
  if (n_batches < 1 || n_batches > 65535) return fail("dqnhip_per_sample: n_batches %d outside [1, 65535]", n_batches);
  RC(refresh_ring(h));
  if (h->h_size < 1) return fail("replay memory is empty");
  PerHost* p = h->per;
  const size_t cnt = (size_t)n_batches * h->B, blk = round_up_z(cnt * 4, 256);
  HIPCHK(hipStreamSynchronize(h->stream));
  RC(ensure_stage(h, 3 * blk));
  char* base = (char*)h->stage_dev;
  PerSampleArgs a{per_tree(p), (const DevState*)h->st, (const DevState*)h->st, h->ring.cap, h->B, 1.0f / (float)h->B, p->cfg.seed,
                  0, (unsigned long long)counter, (int*)base, (int*)(base + blk), (float*)(base + 2 * blk), nullptr};
  HIPCHK(launch(h->stream, k_per_sample, dim3((h->B + 3) / 4, n_batches), dim3(256), 0, a));
  if (idx_host) HIPCHK(hipMemcpyAsync(idx_host, base, cnt * 4, hipMemcpyDeviceToHost, h->stream));
  if (prob_host) HIPCHK(hipMemcpyAsync(prob_host, base + 2 * blk, cnt * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

int dqnhip_per_debug_read(dqnhip_handle h, const char* name, float* host, size_t count) {
  if (!name || !host) return fail("dqnhip_per_debug_read: null argument");
  RC(per_ready(h, "dqnhip_per_debug_read"));
  PerHost* p = h->per;
  const size_t B = h->B;
  if (!strncmp(name, "level", 5) && name[5] >= '0' && name[5] <= '9') {
    const int k = atoi(name + 5);
    if (k > p->tree.levels) return fail("dqnhip_per_debug_read: '%s': the tree has levels 0 .. %d", name, p->tree.levels);
    const size_t n = p->tree.n[k];
    if (count < n) return fail("buffer too small for '%s': %zu < %zu", name, count, n);
    HIPCHK(hipMemcpyAsync(host, p->tree.lvl[k], n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
  }
  const float* src = !strcmp(name, "u") ? p->u : !strcmp(name, "prob") ? p->prob : !strcmp(name, "w") ? p->w : !strcmp(name, "td_abs") ? p->td_abs : nullptr;
  const bool is_slot = !strcmp(name, "slot");
  if (!src && !is_slot) return fail("dqnhip_per_debug_read: unknown buffer '%s' (level<k>|u|slot|prob|w|td_abs)", name);
  if (count < B) return fail("buffer too small for '%s': %zu < %zu", name, count, B);
  HIPCHK(hipMemcpyAsync(host, is_slot ? (const void*)p->slot : (const void*)src, B * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (is_slot) for (size_t i = 0; i < B; ++i) { int v; memcpy(&v, &host[i], sizeof v); host[i] = (float)v; }
  return 0;
}

}  // extern "C"
