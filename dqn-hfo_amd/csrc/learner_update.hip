// learner_update.hip — the update entry points of include/dqnhip.h: index staging, graph capture (capture_updates: the one
// place that sets up and tears down a capture), replay-or-run, dqnhip_update* / dqnhip_get_update_plan / dqnhip_read_stats and the
// in-library benchmark loops.  What an update launches is run_phase's business (learner.hip); this translation unit launches no
// kernel and embeds no device code.
#include "learner_internal.hip.h"

namespace dqnhip_host {

// re-read (head,size) after the env front-end appended episodes on the device
int refresh_ring(H* h) {
  if (!RO(h)->ring_stale) return 0;
  int hs[2];
  HIPCHK(hipMemcpyAsync(hs, RO(h)->st, sizeof hs, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  RO(h)->h_head = hs[0]; RO(h)->h_size = hs[1]; RO(h)->ring_stale = false;
  return 0;
}

// every index inside the replay memory's current size (`what`: "sampled" / "next sampled")
int check_indices(H* h, const int32_t* idx, const char* what) {
  const long long size = RO(h)->h_size;
  for (int i = 0; i < h->B; ++i)
    if (idx[i] < 0 || idx[i] >= size) return fail("%s index %d = %d out of range [0,%lld)", what, i, idx[i], size);
  return 0;
}

int stage_indices(H* h, const int32_t* idx_host, const int** idx_dev) {
  *idx_dev = nullptr;
  if (idx_host || RO(h)->h_size < 1) RC(refresh_ring(h));
  if (RO(h)->h_size < 1) return fail("replay memory is empty");
  if (idx_host) {
    RC(check_indices(h, idx_host, "sampled"));
    // the pinned staging buffer may still be in flight from the previous update
    HIPCHK(hipStreamSynchronize(h->stream));
    memcpy(h->idx_pinned, idx_host, h->B * sizeof(int));
    *idx_dev = h->idx_pinned_dev;           // the gather reads them from the pinned host buffer itself
  }
  return 0;
}

// A prioritized learner's update: [sampler | fill for explicit indices] . the stand-alone sequence on the sampler's buffer . write-back
int run_update(H* h, const int* idx_dev) {
  if (h->per) {
    if (h->cap_u >= 0) return fail("internal: a prioritized update inside a multi-update schedule");
    if (idx_dev) RC(per_fill_launch(h, idx_dev));
    else { RC(per_sample_launch(h)); idx_dev = h->per->idx; }
  }
  for (int p = 0; p < 3; ++p) RC(run_phase(h, p, idx_dev));
  if (h->per) RC(per_update_launch(h));
  return 0;
}

// ---- graph capture ------------------------------------------------------------------------------------------------------------
// Captures s.updates runs of s.body on the learner's stream into *graph.  Nothing executes: replays re-read every changing scalar
// from DevState, so the host's iteration mirrors are put back, and every capture ends with panel parity 0 selected and the
// capture position cleared, whichever way it ends.  A failed body's error text survives the clean-up.
int capture_updates(H* h, const CaptureSpec& s, hipGraph_t* graph) {
  *graph = nullptr;
  HIPCHK(hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
  const int it_a = h->h_actor_iter, it_c = h->h_critic_iter;
  int rc = 0;
  h->cap_n = s.of;
  h->cap_idx = s.idx_bank; h->cap_stats = s.stats_bank;
  h->chain_cap = s.chain_pos >= 0;
  for (int u = 0; u < s.updates && !rc; ++u) {
    h->cap_u = s.multi ? u : s.chain_pos;
    rc = s.body(h, s.idx_dev);
  }
  h->cap_u = -1; h->chain_cap = false; h->cap_n = kMultiU;
  h->cap_idx = nullptr; h->cap_stats = nullptr;
  select_panels(h, 0);
  h->h_actor_iter = it_a; h->h_critic_iter = it_c;
  const std::string msg = g_err;
  const hipError_t e = hipStreamEndCapture(h->stream, graph);
  if (rc) { if (*graph) hipGraphDestroy(*graph); *graph = nullptr; g_err = msg; return rc; }
  if (e != hipSuccess) return fail("hipStreamEndCapture: %s", hipGetErrorString(e));
  return 0;
}
static int count_kernel_nodes(hipGraph_t g, int* out);
// ... instantiated into *out (nullptr on failure); kernel_nodes: the number of kernels it launches
int capture_exec(H* h, const CaptureSpec& s, hipGraphExec_t* out, int* kernel_nodes) {
  hipGraph_t graph = nullptr;
  RC(capture_updates(h, s, &graph));
  if (kernel_nodes && count_kernel_nodes(graph, kernel_nodes)) { hipGraphDestroy(graph); *out = nullptr; return 1; }
  const hipError_t e = hipGraphInstantiate(out, graph, nullptr, nullptr, 0);
  hipGraphDestroy(graph);
  if (e != hipSuccess) { *out = nullptr; return fail("hipGraphInstantiate: %s", hipGetErrorString(e)); }
  return 0;
}

// n updates per replay.  Two consecutive hipGraphLaunch calls leave the GPU idle for ~8.4 us between the last kernel of one and the
// first kernel of the next (kernel trace, profiles/r04_graph_gap.txt; two instances of the graph launched alternately: the same) -
// 2.8 % of a 300-us update; inside a graph the same boundary is a plain kernel boundary, and the gather of update u + 1 rides in
// update u's last launch (adam_launch, DevState::gbase).
// (a prioritized or n-step learner's graph: n stand-alone sequences back to back — no rider serves a successor)
static CaptureSpec multi_spec(const H* h, int n) { CaptureSpec s; s.updates = n; s.multi = !standalone_updates(h); s.of = n; return s; }

// what each slot of graph_exec captures.  idx_dev: the pipelined slots' index buffer (already on the device)
static CaptureSpec slot_spec(const H* h, GraphSlot slot, const int* idx_dev) {
  CaptureSpec s;
  switch (slot) {
    case kGraphExplicit: s.idx_dev = h->idx_pinned_dev; break;
    case kGraphPipe0: case kGraphPipe1: s.idx_dev = idx_dev; break;
    case kGraphMulti: s = multi_spec(h, kMultiU); break;
    // dqnhip_update_chained: ONE update captured as position 0 (head: own gather), 1 or 2 (continued at parity 1 / 0) of a
    // multi-update graph, its riders reading the next update's explicit indices
    case kGraphChainHead: s.chain_pos = 0; s.idx_dev = h->idx_pinned_dev; break;
    case kGraphChainPar1: s.chain_pos = 1; break;
    case kGraphChainPar0: s.chain_pos = 2; break;
    default: break;     // kGraphSampled: one update, indices sampled on the device
  }
  return s;
}

// *g, captured from `s` on first use; nullptr where graphs are off, kernel timing is on, or a capture has failed (which turns
// graphs off for this learner)
static hipGraphExec_t graph_of(H* h, hipGraphExec_t* g, const CaptureSpec& s, int* kernel_nodes = nullptr) {
  if (!h->cfg.use_graph || h->timing || h->graph_failed) return nullptr;
  if (!*g && capture_exec(h, s, g, kernel_nodes)) h->graph_failed = true;
  return *g;
}
static hipGraphExec_t graph_of(H* h, GraphSlot slot, const int* idx_dev = nullptr) {
  return graph_of(h, &h->graph_exec[slot], slot_spec(h, slot, idx_dev));
}
static int replay(H* h, hipGraphExec_t g, int updates) {
  HIPCHK(hipGraphLaunch(g, h->stream));
  h->h_actor_iter += updates; h->h_critic_iter += updates;
  return 0;
}
// one update: the slot's graph, or the three phases eagerly
static int replay_or_run(H* h, GraphSlot slot, const int* idx_dev) {
  if (hipGraphExec_t g = graph_of(h, slot, idx_dev)) return replay(h, g, 1);
  return run_update(h, idx_dev);
}

int run_chunks(H* h, hipGraphExec_t* g, int n_chunks, int (*body)(H*, const int*)) {
  CaptureSpec s; s.body = body;
  const hipGraphExec_t ge = graph_of(h, g, s);
  for (int c = 0; c < n_chunks; ++c) {
    if (ge) HIPCHK(hipGraphLaunch(ge, h->stream));
    else RC(body(h, nullptr));
  }
  return 0;
}

// kernel nodes of a captured sequence
static int count_kernel_nodes(hipGraph_t g, int* out) {
  size_t cnt = 0;
  HIPCHK(hipGraphGetNodes(g, nullptr, &cnt));
  std::vector<hipGraphNode_t> nodes(cnt);
  if (cnt) HIPCHK(hipGraphGetNodes(g, nodes.data(), &cnt));
  int k = 0;
  for (hipGraphNode_t nd : nodes) {
    hipGraphNodeType t;
    HIPCHK(hipGraphNodeGetType(nd, &t));
    if (t == hipGraphNodeTypeKernel) ++k;
  }
  *out = k;
  return 0;
}
// the kernels `updates` consecutive updates launch — as a multi-update graph captures them (multi) or stand-alone.  A capture that
// is thrown away: nothing executes, nothing is instantiated.
static int count_launches(H* h, bool multi, int updates, int* out) {
  CaptureSpec s; s.updates = updates; s.multi = multi && !standalone_updates(h);
  hipGraph_t graph = nullptr;
  RC(capture_updates(h, s, &graph));
  const int rc = count_kernel_nodes(graph, out);
  hipGraphDestroy(graph);
  return rc;
}

// ---- dqnhip_update_indexed_n: banks ---------------------------------------------------------------------------------------------
// A captured graph has its index and stats addresses baked into its kernel arguments, and two graph launches may be in flight
// without the host having waited, so one set of slots is not enough.  Chosen here: kIxBanks banks, each with its OWN captured
// graphs (ix_graph[bank][size]) - the alternative, one set of graphs whose kernel nodes are re-pointed before every launch
// (hipGraphExecKernelNodeSetParams on 16 gathers + 16 ticks), costs a host round per node per launch, where a second set of
// graphs costs one more capture, once.  A bank is guarded by the event recorded behind its graph; the host waits on it only when
// the round robin comes back to a bank that is still busy, i.e. with two banks it waits for the graph BEFORE the one that is
// running, and the device always has the next graph queued.
static int ix_ensure_banks(H* h) {
  if (h->ix_idx[0]) return 0;
  for (int b = 0; b < kIxBanks; ++b) {
    // (system-scope release: the ticks' stores into the stats bank are visible to the host once the event has completed)
    HIPCHK(hipEventCreateWithFlags(&h->ix_ev[b], hipEventDisableTiming | hipEventReleaseToSystem));
    HIPCHK(hipHostMalloc((void**)&h->ix_stats[b], kMultiU * 4 * sizeof(float), hipHostMallocMapped));
    memset(h->ix_stats[b], 0, kMultiU * 4 * sizeof(float));
    { void* d = nullptr; HIPCHK(hipHostGetDevicePointer(&d, h->ix_stats[b], 0)); h->ix_stats_dev[b] = (float*)d; }
    HIPCHK(hipHostMalloc((void**)&h->ix_idx[b], (size_t)kMultiU * h->B * sizeof(int), hipHostMallocMapped));
    memset(h->ix_idx[b], 0, (size_t)kMultiU * h->B * sizeof(int));
    { void* d = nullptr; HIPCHK(hipHostGetDevicePointer(&d, h->ix_idx[b], 0)); h->ix_idx_dev[b] = (const int*)d; }
  }
  return 0;
}
// waits for bank b's graph and files its updates' scalars, in update order
static int ix_harvest(H* h, int b) {
  if (!h->ix_busy[b]) return 0;
  HIPCHK(hipEventSynchronize(h->ix_ev[b]));
  for (int u = 0; u < h->ix_busy[b]; ++u) {
    const float* s = h->ix_stats[b] + 4 * u;
    int fl = 0; memcpy(&fl, &s[2], sizeof fl);
    h->ix_pairs.push_back(s[0]); h->ix_pairs.push_back(s[1]);
    // the device flags are sticky: what THIS update raised is what the one before it had not left behind
    if (fl & ~h->ix_prev_flags) h->ix_flagged.emplace_back(h->ix_harvested, fl & ~h->ix_prev_flags);
    h->ix_prev_flags = fl;
    h->ix_harvested += 1;
  }
  h->ix_busy[b] = 0;
  return 0;
}
int ix_harvest_all(H* h) {
  // oldest first: the busy banks are the last ones the round robin handed out
  for (int k = 0; k < kIxBanks; ++k) RC(ix_harvest(h, (h->ix_next + k) % kIxBanks));
  return 0;
}
// `sz` updates (a graph size: 16 / 8 / 4 / 2 / 1, kind = its index in that list) on idx[0 .. sz * B), through the next bank
static int ix_run(H* h, const int32_t* idx, int sz, int kind) {
  const int b = h->ix_next;
  RC(ix_harvest(h, b));                       // the only host wait: a bank that is still busy when its turn comes round again
  h->ix_next = (b + 1) % kIxBanks;
  memcpy(h->ix_idx[b], idx, (size_t)sz * h->B * sizeof(int));
  CaptureSpec s;
  // (one update: the stand-alone form, as dqnhip_update_async(idx) captures it)
  s.updates = sz; s.of = sz; s.multi = sz > 1;
  s.idx_dev = h->ix_idx_dev[b]; s.idx_bank = h->ix_idx_dev[b]; s.stats_bank = h->ix_stats_dev[b];
  int rc = 0;
  if (hipGraphExec_t g = graph_of(h, &h->ix_graph[b][kind], s, &h->ix_nodes[kind])) rc = replay(h, g, sz);
  else
    for (int u = 0; u < sz && !rc; ++u) {     // eagerly: the same slots
      h->cap_stats = s.stats_bank + 4 * u;
      rc = run_update(h, s.idx_bank + (size_t)u * h->B);
      h->cap_stats = nullptr;
    }
  const hipError_t e = hipEventRecord(h->ix_ev[b], h->stream);
  if (rc || e != hipSuccess) {
    // whatever was enqueued before the failure still reads and writes the bank: nothing may reuse it before that has drained, and
    // what it wrote belongs to no update the caller was told about (the bank stays free, its slots are not harvested)
    const std::string msg = g_err;
    hipStreamSynchronize(h->stream);
    if (rc) { g_err = msg; return rc; }
    return fail("hipEventRecord: %s", hipGetErrorString(e));
  }
  h->ix_busy[b] = sz;
  return 0;
}

// dqnhip_get_update_plan's report, whole (the caller's struct may be the shorter one of an earlier header)
static int update_plan_fill(H* h, dqnhip_update_plan* out) {
  HIPCHK(hipSetDevice(h->cfg.device));
  const UpdatePlan p = plan_of(h);
  memset(out, 0, sizeof *out);
  out->struct_size = (int32_t)sizeof *out;
  out->lr_policy = h->cfg.lr_policy; out->regularised = has_decay(h) ? 1 : 0;
  out->forms = (p.fp16 ? DQNHIP_PLAN_FP16 : 0) | (p.dp ? DQNHIP_PLAN_DATA_PARALLEL : 0) | (p.shifted_c ? DQNHIP_PLAN_BWD_SHIFTED_CRITIC : 0) |
               (p.shifted_a ? DQNHIP_PLAN_BWD_SHIFTED_ACTOR : 0) | (p.head_rides_c ? DQNHIP_PLAN_HEAD_WGRAD_RIDES_CRITIC : 0) |
               (p.head_rides_a ? DQNHIP_PLAN_HEAD_WGRAD_RIDES_ACTOR : 0) | (p.fuse_q ? DQNHIP_PLAN_Q_TRAIN_IN_DGRAD : 0) |
               (p.fused_seed ? DQNHIP_PLAN_HEAD_SEED_FUSED : 0) | (p.fuse_head ? DQNHIP_PLAN_DQDA_HEAD_BWD : 0) |
               (p.critic_l0 ? DQNHIP_PLAN_CRITIC_L0_RIDES : 0) | (p.first_layers_merged ? DQNHIP_PLAN_FIRST_LAYERS_MERGED : 0) |
               (p.early_l0 ? DQNHIP_PLAN_EARLY_GATHER_L0 : 0) | (p.tails_ride ? DQNHIP_PLAN_DP_TAILS_RIDE : 0) |
               (p.prioritized ? DQNHIP_PLAN_PRIORITIZED : 0) | (p.nstep ? DQNHIP_PLAN_NSTEP : 0) |
               (p.smooth ? DQNHIP_PLAN_TARGET_SMOOTHING : 0);
  out->updates_per_graph = kMultiU; out->solver_type = h->cfg.solver_type;
  // per net and update: one all-reduce (per-layer buckets: one per tower layer + the head slice; bf16 exchange: the tails travel in a
  // second call beside the actor's; sharded optimiser: reduce-scatter + the 4-float all-reduce + 2 (fp16 learner: 4) all-gathers)
  if (h->comm) out->collectives = h->dp_shard ? 2 * (2 + (h->fp16 ? 4 : 2)) : h->dp_per_layer ? 2 * (h->L + 1) : h->dp_half ? 3 : 2;
  if (h->dp_shard) return 0;
  int n1 = 0, nf = 0, n2 = 0;
  RC(count_launches(h, false, 1, &n1));
  RC(count_launches(h, true, 1, &nf));
  RC(count_launches(h, true, 2, &n2));
  out->launches_single = n1; out->launches_graph_first = nf; out->launches_in_graph = n2 - nf;
  return 0;
}

}  // namespace dqnhip_host

extern "C" {

int dqnhip_get_update_plan(dqnhip_handle h, dqnhip_update_plan* out) {
  if (!h || !out) return fail("null argument");
  // the struct as it is, or as it was before lr_policy / regularised were appended (the caller gets the words it knows)
  const int32_t asked = out->struct_size;
  if (asked != (int32_t)sizeof(dqnhip_update_plan) && asked != (int32_t)offsetof(dqnhip_update_plan, lr_policy))
    return fail("dqnhip_update_plan.struct_size %d != %zu (ABI mismatch)", out->struct_size, sizeof(dqnhip_update_plan));
  if (h->next_phase != 0) return fail("dqnhip_get_update_plan: a phased update is in progress (next phase %d)", h->next_phase);
  if (h->timing) return fail("dqnhip_get_update_plan: kernel timing is on (timed launches are not captured)");
  dqnhip_update_plan full;
  RC(update_plan_fill(h, &full));
  memcpy(out, &full, (size_t)asked);
  out->struct_size = asked;
  return 0;
}

int dqnhip_update_async(dqnhip_handle h, const int32_t* idx_host) {
  if (!h) return fail("null handle");
  h->epoch += 1;
  HIPCHK(hipSetDevice(h->cfg.device));
  if (h->cfg.dp_world > 1) return fail("dqnhip_update_async: dp_world > 1 requires dqnhip_update_phase + all-reduce (or dqnhip_dp_update)");
  if (h->dp_half) return fail("dqnhip_update_async: this learner exchanges bf16 gradients (DQNHIP_DP_HALF_GRADS): use dqnhip_dp_update");
  if (h->dp_shard) return fail("dqnhip_update_async: this learner's optimiser is sharded over its group (DQNHIP_DP_SHARD_OPT): use dqnhip_dp_update");
  if (h->next_phase != 0) return fail("dqnhip_update_async: a phased update is in progress (next phase %d)", h->next_phase);
  RingUse ring_use(h);
  RC(sync_dirty16(h));
  const int* idx_dev = nullptr;
  RC(stage_indices(h, idx_host, &idx_dev));
  RC(per_sync_if_needed(h));
  return replay_or_run(h, idx_host ? kGraphExplicit : kGraphSampled, idx_dev);
}

int dqnhip_update_async_n(dqnhip_handle h, int32_t n) {
  if (!h) return fail("null handle");
  h->epoch += 1;
  if (n < 0) return fail("dqnhip_update_async_n: n must be >= 0");
  HIPCHK(hipSetDevice(h->cfg.device));
  if (dp_exchanges(h)) return fail("dqnhip_update_async_n: data-parallel learners use dqnhip_dp_update");
  if (h->next_phase != 0) return fail("dqnhip_update_async_n: a phased update is in progress (next phase %d)", h->next_phase);
  RingUse ring_use(h);
  RC(sync_dirty16(h));
  if (RO(h)->h_size < 1) RC(refresh_ring(h));
  if (RO(h)->h_size < 1) return fail("replay memory is empty");
  RC(per_sync_if_needed(h));
  hipGraphExec_t g;
  while (n >= kMultiU && (g = graph_of(h, kGraphMulti)) != nullptr) { RC(replay(h, g, kMultiU)); n -= kMultiU; }
  // the remainder as graphs of 8 / 4 / 2 updates (the same launch sequence as the sixteen-update graph, cut shorter), then one by
  // one: a remainder of r one-update graphs would pay r gathers, r first-layer launches and the gap between two graph launches
  // (the driver's 20 timed steps are 16 + 4)
  for (int k = 0; k < 3; ++k) {
    const int sz = 8 >> k;
    if (n >= sz && (g = graph_of(h, &h->graph_small[k], multi_spec(h, sz))) != nullptr) { RC(replay(h, g, sz)); n -= sz; }
  }
  for (; n > 0; --n) RC(replay_or_run(h, kGraphSampled, nullptr));
  return 0;
}

// n updates on caller-supplied indices as multi-update graphs (see dqnhip.h): what the reference's driver asks for with
// `for (i < n_updates) dqn->Update()` (src/dqn_main.cpp:359-361, :340-343) once the adaptor stops reading every update's scalars back
// (Update() is void, src/dqn.cpp:799-826 only logs and snapshots).  Same cut as dqnhip_update_async_n, same capture machinery.
int dqnhip_update_indexed_n(dqnhip_handle h, const int32_t* idx_host, int32_t n) {
  if (!h) return fail("null handle");
  h->epoch += 1;
  if (n < 0) return fail("dqnhip_update_indexed_n: n must be >= 0");
  RC(feature_refuse(h, kFeatSampling, "dqnhip_update_indexed_n"));
  HIPCHK(hipSetDevice(h->cfg.device));
  if (dp_exchanges(h)) return fail("dqnhip_update_indexed_n: data-parallel learners use dqnhip_dp_update");
  if (h->next_phase != 0) return fail("dqnhip_update_indexed_n: a phased update is in progress (next phase %d)", h->next_phase);
  if (n == 0) return 0;
  if (!idx_host) return fail("dqnhip_update_indexed_n: explicit indices required (on-device sampling: dqnhip_update_async_n)");
  RingUse ring_use(h);
  RC(refresh_ring(h));
  if (RO(h)->h_size < 1) return fail("replay memory is empty");
  // all of them before anything is enqueued
  const long long size = RO(h)->h_size;
  for (int u = 0; u < n; ++u)
    for (int i = 0; i < h->B; ++i) {
      const int32_t v = idx_host[(size_t)u * h->B + i];
      if (v < 0 || v >= size) return fail("update %d: sampled index %d = %d out of range [0,%lld)", u, i, v, size);
    }
  RC(sync_dirty16(h));
  RC(ix_ensure_banks(h));
  const int32_t* idx = idx_host;
  for (int kind = 0; kind < kIxSizes; ++kind) {
    const int sz = kMultiU >> kind;
    while (n >= sz) {
      RC(ix_run(h, idx, sz, kind));
      idx += (size_t)sz * h->B; n -= sz;
      if (sz < kMultiU) break;              // (16s repeat; of each smaller size at most one)
    }
  }
  // dqnhip_read_stats reads the learner's one pinned triple: the last update's, copied behind the last graph of the call (a tick
  // has one host pointer, and that is its slot of the bank)
  HIPCHK(hipMemcpyAsync(h->pinned_stats, &h->st->critic_loss, 3 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  return 0;
}

int dqnhip_collect_stats(dqnhip_handle h, float* critic_loss, float* avg_q, int32_t cap, int32_t* n_out) {
  if (!h || !n_out) return fail("null argument");
  *n_out = 0;
  if (cap < 0 || (cap > 0 && (!critic_loss || !avg_q))) return fail("dqnhip_collect_stats: cap must be >= 0 and both arrays given");
  HIPCHK(hipSetDevice(h->cfg.device));
  RC(ix_harvest_all(h));
  const int n = (int)std::min<size_t>((size_t)cap, h->ix_pairs.size() / 2);
  int bad = -1;                               // first update of this collection that raised a flag or left a non-finite loss
  for (int i = 0; i < n; ++i) {
    critic_loss[i] = h->ix_pairs[2 * i]; avg_q[i] = h->ix_pairs[2 * i + 1];
    if (bad < 0 && !std::isfinite(critic_loss[i])) bad = i;
  }
  h->ix_pairs.erase(h->ix_pairs.begin(), h->ix_pairs.begin() + 2 * n);
  const unsigned long long end = h->ix_collected + (unsigned long long)n;
  int flags = 0; bool any = false;
  for (; !h->ix_flagged.empty() && h->ix_flagged.front().first < end; h->ix_flagged.pop_front()) {
    const int pos = (int)(h->ix_flagged.front().first - h->ix_collected);
    if (!any && (bad < 0 || pos <= bad)) { bad = pos; flags = h->ix_flagged.front().second; }
    any = true;
  }
  h->ix_collected = end;
  *n_out = n;
  if (any) {      // sticky on the device until reported: cleared as dqnhip_read_stats clears them
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemsetAsync(&h->st->flags, 0, sizeof(int), h->stream));
    h->pinned_stats[2] = 0.0f; h->ix_prev_flags = 0;
  }
  if (bad < 0) return 0;
  if (flags & kFlagTarget) return fail("collected update %d: Target not finite!", bad);
  if (flags & kFlagGradNorm) return fail("collected update %d: Gradient norm not finite: the clip+Adam step was skipped (fp16: lower cfg.loss_scale or use loss_scale_mode = dynamic)", bad);
  return fail("collected update %d: Critic loss not finite!", bad);
}

int dqnhip_update_phase(dqnhip_handle h, int32_t phase, const int32_t* idx_host) {
  if (!h) return fail("null handle");
  RC(feature_refuse(h, kFeatSampling, "dqnhip_update_phase"));
  h->epoch += 1;
  HIPCHK(hipSetDevice(h->cfg.device));
  // (with DQNHIP_DP_HALF_GRADS the exchange — bf16 image, all-reduce, widening by the clip-norm pass — lives inside
  // dqnhip_dp_update: a caller-driven exchange between phases would leave phase 1 / 2 reading a stale bf16 image)
  if (h->dp_half) return fail("dqnhip_update_phase: this learner exchanges bf16 gradients (DQNHIP_DP_HALF_GRADS): use dqnhip_dp_update");
  if (h->dp_shard) return fail("dqnhip_update_phase: this learner's optimiser is sharded over its group (DQNHIP_DP_SHARD_OPT): use dqnhip_dp_update");
  // 0 -> 1 -> 2 or 10 -> 11 -> 1 -> 2: a phase run out of order would apply stale gradients
  // and advance the iteration counters
  const int expect = h->next_phase;
  const bool ok = (phase == 0 || phase == 10) ? (expect == 0) : (phase == expect);
  if (!ok) return fail("dqnhip_update_phase: phase %d out of order (expected %s)", phase,
                       expect == 0 ? "0 or 10" : expect == 1 ? "1" : expect == 2 ? "2" : "11");
  const int* idx_dev = nullptr;
  int rc;
  if (phase != 0 && phase != 10) rc = run_phase(h, phase, idx_dev);
  else {
    RingUse ring_use(h);
    rc = sync_dirty16(h);
    if (!rc) rc = stage_indices(h, idx_host, &idx_dev);
    if (!rc) rc = run_phase(h, phase, idx_dev);
  }
  // a failed phase abandons the update: the next one starts from phase 0 / 10 again (one transient error must not
  // wedge the learner in "out of order" for good)
  h->next_phase = rc ? 0 : (phase == 0 ? 1 : phase == 10 ? 11 : phase == 11 ? 1 : phase == 1 ? 2 : 0);
  return rc;
}

int dqnhip_update_abort(dqnhip_handle h) {
  if (!h) return fail("null handle");
  h->next_phase = 0;
  return 0;
}

int dqnhip_read_stats(dqnhip_handle h, float* critic_loss, float* avg_q) {
  if (!h) return fail("null handle");
  HIPCHK(hipSetDevice(h->cfg.device));
  // {critic_loss, avg_q, flags}: the last block of every update writes them into this pinned, host-mapped buffer itself
  // (tick_body): no device-to-host copy, the stream sync is the only wait
  HIPCHK(hipStreamSynchronize(h->stream));
  RC(ix_harvest_all(h));     // (indexed updates: files their scalars - nothing to wait for any more - so that ix_prev_flags is the device's)
  if (critic_loss) *critic_loss = h->pinned_stats[0];
  if (avg_q) *avg_q = h->pinned_stats[1];
  int flags = 0; memcpy(&flags, &h->pinned_stats[2], sizeof flags);
  if (flags) { HIPCHK(hipMemsetAsync(&h->st->flags, 0, sizeof(int), h->stream)); h->pinned_stats[2] = 0.0f; h->ix_prev_flags = 0; }   // sticky until reported
  // CHECK(std::isfinite(target)) (src/dqn.cpp:898) and CHECK(std::isfinite(critic_loss)) (:906) — the
  // reference aborts; here: an error code from the first read after the offending update, whichever
  // entry point (blocking, async, phased, hipGraph) ran it
  if (flags & kFlagTarget) return fail("Target not finite!");
  if (flags & kFlagGradNorm) return fail("Gradient norm not finite: the clip+Adam step was skipped (fp16: lower cfg.loss_scale or use loss_scale_mode = dynamic)");
  if (!std::isfinite(h->pinned_stats[0])) return fail("Critic loss not finite!");
  return 0;
}

int dqnhip_skipped_steps(dqnhip_handle h, int64_t* count) {
  if (!h || !count) return fail("null argument");
  HIPCHK(hipSetDevice(h->cfg.device));
  int v = 0;
  HIPCHK(hipMemcpyAsync(h->pinned_stats + 8, &h->st->skipped_steps, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  memcpy(&v, h->pinned_stats + 8, sizeof v);
  *count = v;
  return 0;
}

// Dynamic loss scaling: the state the optimiser launches keep in DevState.  Stream-ordered like dqnhip_skipped_steps: copied behind
// everything enqueued so far, one sync.
int dqnhip_get_loss_scale(dqnhip_handle h, dqnhip_loss_scale_state* out) {
  if (!h || !out) return fail("null argument");
  HIPCHK(hipSetDevice(h->cfg.device));
  struct Tail { float mult[2][2]; int good[2], backoffs[2], growths[2]; } t;
  static_assert(offsetof(DevState, ls_good) == offsetof(DevState, ls_mult) + offsetof(Tail, good) &&
                offsetof(DevState, ls_backoffs) == offsetof(DevState, ls_mult) + offsetof(Tail, backoffs) &&
                offsetof(DevState, ls_growths) == offsetof(DevState, ls_mult) + offsetof(Tail, growths) && sizeof(Tail) <= 15 * sizeof(float),
                "the loss-scale fields of DevState are contiguous and fit pinned_stats[16 .. 31)");
  int skipped = 0;
  HIPCHK(hipMemcpyAsync(h->pinned_stats + 16, h->st->ls_mult, sizeof t, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(h->pinned_stats + 31, &h->st->skipped_steps, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  memcpy(&t, h->pinned_stats + 16, sizeof t);
  memcpy(&skipped, h->pinned_stats + 31, sizeof skipped);
  memset(out, 0, sizeof *out);
  out->struct_size = (int32_t)sizeof *out;
  out->mode = h->ls_dynamic ? DQNHIP_LOSS_SCALE_DYNAMIC : DQNHIP_LOSS_SCALE_STATIC;
  out->mult_actor = h->ls_dynamic ? t.mult[DQNHIP_ACTOR][0] : 1.0f; out->mult_critic = h->ls_dynamic ? t.mult[DQNHIP_CRITIC][0] : 1.0f;
  out->good_actor = t.good[DQNHIP_ACTOR]; out->good_critic = t.good[DQNHIP_CRITIC];
  out->backoffs_actor = t.backoffs[DQNHIP_ACTOR]; out->backoffs_critic = t.backoffs[DQNHIP_CRITIC];
  out->growths_actor = t.growths[DQNHIP_ACTOR]; out->growths_critic = t.growths[DQNHIP_CRITIC];
  out->skipped_steps = skipped;
  return 0;
}

int dqnhip_set_loss_scale(dqnhip_handle h, float mult_critic, float mult_actor) {
  if (!h) return fail("null handle");
  if (!h->ls_dynamic) return fail("dqnhip_set_loss_scale: this learner's loss_scale_mode is static (cfg.loss_scale is fixed at create time)");
  if (h->next_phase != 0) return fail("dqnhip_set_loss_scale: a phased update is in progress (next phase %d)", h->next_phase);
  const float m[2] = {mult_actor, mult_critic};      // DevState order: [actor, critic]
  for (int i = 0; i < 2; ++i) {
    const char* who = i == DQNHIP_ACTOR ? "mult_actor" : "mult_critic";
    if (!is_pow2(m[i])) return fail("dqnhip_set_loss_scale: %s = %g is not a power of two", who, (double)m[i]);
    if (m[i] < h->cfg.loss_scale_min_mult || m[i] > h->cfg.loss_scale_max_mult)
      return fail("dqnhip_set_loss_scale: %s = %g is outside [loss_scale_min_mult, loss_scale_max_mult] = [%g, %g]", who, (double)m[i],
                  (double)h->cfg.loss_scale_min_mult, (double)h->cfg.loss_scale_max_mult);
  }
  HIPCHK(hipSetDevice(h->cfg.device));
  h->epoch += 1;                                     // (a chained update's riders are dropped: the next call starts a chain afresh)
  struct { float mult[2][2]; int good[2]; } v = {{{m[0], 1.0f / m[0]}, {m[1], 1.0f / m[1]}}, {0, 0}};
  static_assert(offsetof(DevState, ls_good) == offsetof(DevState, ls_mult) + sizeof v.mult, "ls_good follows ls_mult");
  HIPCHK(hipStreamSynchronize(h->stream));           // behind every update enqueued so far; the copy below is synchronous (v is on this stack)
  HIPCHK(hipMemcpy(h->st->ls_mult, &v, sizeof v, hipMemcpyHostToDevice));
  return 0;
}

int dqnhip_update(dqnhip_handle h, const int32_t* idx_host, float* critic_loss, float* avg_q) {
  RC(dqnhip_update_async(h, idx_host));
  return dqnhip_read_stats(h, critic_loss, avg_q);
}

// dqnhip_update with the NEXT update's indices known one call ahead (see dqnhip.h).  The reference's driver runs its updates in
// bursts (src/dqn_main.cpp:359-361: `for (i < n_updates) dqn->Update()`), one blocking call at a time; with idx_next the burst gets the
// schedule of a multi-update graph — the next update's gather in this update's critic optimiser launch, its four first layers in the
// actor's — one graph launch per update.  What rode along is used only if the next call's idx equals idx_next and nothing changed
// weights, iteration counters or the replay memory in between; otherwise that call starts a fresh chain (own gather, own first
// layers: what the riders left is overwritten).  Every update computes exactly what dqnhip_update computes on the same indices.
int dqnhip_update_chained(dqnhip_handle h, const int32_t* idx_host, const int32_t* idx_next, float* critic_loss, float* avg_q) {
  if (!h) return fail("null handle");
  if (!idx_host) return fail("dqnhip_update_chained: explicit indices required (on-device sampling: dqnhip_update_async_n)");
  RC(feature_refuse(h, kFeatSampling, "dqnhip_update_chained"));
  HIPCHK(hipSetDevice(h->cfg.device));
  const UpdatePlan P = plan_of(h);
  const bool can = P.early_l0 && !P.dp && !h->comm && h->cfg.use_graph && !h->timing && !h->graph_failed && !shares_params(h);
  if (!can) { h->chain_valid = false; return dqnhip_update(h, idx_host, critic_loss, avg_q); }
  if (h->next_phase != 0) return fail("dqnhip_update_chained: a phased update is in progress (next phase %d)", h->next_phase);
  {
    RingUse ring_use(h);
    RC(refresh_ring(h));
    if (RO(h)->h_size < 1) return fail("replay memory is empty");
    RC(check_indices(h, idx_host, "sampled"));
    if (idx_next) RC(check_indices(h, idx_next, "next sampled"));
    if (!h->idx_next_pinned[0])
      for (int i = 0; i < 2; ++i) {
        HIPCHK(hipHostMalloc((void**)&h->idx_next_pinned[i], h->B * sizeof(int), hipHostMallocMapped));
        memset(h->idx_next_pinned[i], 0, h->B * sizeof(int));
        void* d = nullptr; HIPCHK(hipHostGetDevicePointer(&d, h->idx_next_pinned[i], 0)); h->idx_next_dev[i] = (const int*)d;
      }
    HIPCHK(hipStreamSynchronize(h->stream));       // the pinned index buffers may still be in flight from an earlier (asynchronous) update
    const bool cont = h->chain_valid && h->chain_epoch == h->epoch && h->chain_ring_epoch == RO(h)->epoch &&
                      memcmp(h->chain_idx.data(), idx_host, h->B * sizeof(int32_t)) == 0;
    const int par = cont ? h->chain_par : 0;         // this update's panel parity
    const GraphSlot slot = !cont ? kGraphChainHead : par ? kGraphChainPar1 : kGraphChainPar0;
    if (!cont) memcpy(h->idx_pinned, idx_host, h->B * sizeof(int));
    h->chain_valid = false;
    if (idx_next) {
      memcpy(h->idx_next_pinned[par ^ 1], idx_next, h->B * sizeof(int));
      h->chain_idx.assign(idx_next, idx_next + h->B);
    }
    hipGraphExec_t g = graph_of(h, slot);
    if (!g) return dqnhip_update(h, idx_host, critic_loss, avg_q);
    RC(replay(h, g, 1));
    h->epoch += 1;
    if (idx_next) { h->chain_valid = true; h->chain_par = par ^ 1; h->chain_epoch = h->epoch; h->chain_ring_epoch = RO(h)->epoch; }
  }
  // (both null: enqueue only — the caller does its own work while the update runs, e.g. drawing the prediction after next, and
  // collects the scalars with dqnhip_read_stats)
  if (critic_loss == nullptr && avg_q == nullptr) return 0;
  return dqnhip_read_stats(h, critic_loss, avg_q);
}

// One-deep pipelined form of dqnhip_update: enqueues update t and returns the scalars of update t-1 (zeros on the
// first call).  The host then waits for update t-1 only, while update t is already queued behind it — the device
// never idles on the host's index draw, the H2D of the indices or the read-back, which dqnhip_update pays on
// every call.  Indices and scalars use two pinned slots each (nothing in flight is overwritten).
int dqnhip_update_pipelined(dqnhip_handle h, const int32_t* idx_host, float* critic_loss, float* avg_q) {
  if (!h) return fail("null handle");
  RC(feature_refuse(h, kFeatSampling, "dqnhip_update_pipelined"));
  h->epoch += 1;
  HIPCHK(hipSetDevice(h->cfg.device));
  if (dp_exchanges(h)) return fail("dqnhip_update_pipelined: data-parallel learners use dqnhip_update_phase / dqnhip_dp_update");
  if (h->next_phase != 0) return fail("dqnhip_update_pipelined: a phased update is in progress (next phase %d)", h->next_phase);
  if (!h->pipe_ev[0]) {
    for (int i = 0; i < 2; ++i) {
      HIPCHK(hipEventCreateWithFlags(&h->pipe_ev[i], hipEventDisableTiming));
      HIPCHK(hipHostMalloc((void**)&h->pipe_idx_pinned[i], h->B * sizeof(int), hipHostMallocMapped));
      { void* d = nullptr; HIPCHK(hipHostGetDevicePointer(&d, h->pipe_idx_pinned[i], 0)); h->pipe_idx_dev[i] = (int*)d; }
      HIPCHK(hipHostMalloc((void**)&h->pipe_stats[i], 64, hipHostMallocDefault));
      memset(h->pipe_stats[i], 0, 64);
    }
  }
  const int slot = (int)(h->pipe_count & 1);
  {
    RingUse ring_use(h);
    RC(sync_dirty16(h));
    const int* idx_dev = nullptr;
    if (idx_host) {
      RC(refresh_ring(h));
      RC(check_indices(h, idx_host, "sampled"));
      // slot's previous user was update t-2, whose completion the previous call already waited for
      memcpy(h->pipe_idx_pinned[slot], idx_host, h->B * sizeof(int));
      idx_dev = h->pipe_idx_dev[slot];      // device alias of the pinned slot (no H2D copy)
    } else if (RO(h)->h_size < 1) {
      RC(refresh_ring(h));
      if (RO(h)->h_size < 1) return fail("replay memory is empty");
    }
    RC(replay_or_run(h, !idx_host ? kGraphSampled : slot ? kGraphPipe1 : kGraphPipe0, idx_dev));
  }
  HIPCHK(hipMemcpyAsync(h->pipe_stats[slot], &h->st->critic_loss, 4 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipEventRecord(h->pipe_ev[slot], h->stream));
  const int prev = slot ^ 1;
  float loss = 0.f, q = 0.f; int flags = 0;
  if (h->pipe_count > 0) {
    HIPCHK(hipEventSynchronize(h->pipe_ev[prev]));
    loss = h->pipe_stats[prev][0]; q = h->pipe_stats[prev][1];
    memcpy(&flags, &h->pipe_stats[prev][2], sizeof flags);
  }
  h->pipe_count += 1;
  if (critic_loss) *critic_loss = loss;
  if (avg_q) *avg_q = q;
  if (flags) {     // sticky on the device: report through the blocking path, which clears them
    float l2, q2;
    const int rc = dqnhip_read_stats(h, &l2, &q2);      // syncs the stream: update t (enqueued above) has completed too
    // update t's read-back into the other slot was enqueued BEFORE the flags were cleared and still carries them: this
    // report covers it, so the next call must not raise the same flag again
    memset(&h->pipe_stats[slot][2], 0, sizeof(float));
    return rc ? 1 : fail("update flags raised");
  }
  if (!std::isfinite(loss)) return fail("Critic loss not finite!");
  return 0;
}

int dqnhip_benchmark(dqnhip_handle h, int32_t warmup, int32_t iterations, float* avg_ms) {
  if (!h) return fail("null handle");
  if (iterations < 1) return fail("iterations must be >= 1");
  HIPCHK(hipSetDevice(h->cfg.device));
  if (warmup > 0) RC(dqnhip_update_async_n(h, warmup));
  hipEvent_t a, b;
  HIPCHK(hipEventCreate(&a)); HIPCHK(hipEventCreate(&b));
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipEventRecord(a, h->stream));
  RC(dqnhip_update_async_n(h, iterations));
  HIPCHK(hipEventRecord(b, h->stream));
  HIPCHK(hipEventSynchronize(b));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, a, b));
  hipEventDestroy(a); hipEventDestroy(b);
  if (avg_ms) *avg_ms = ms / iterations;
  return 0;
}


// What the reference's driver gets from this library (src/dqn_main.cpp:361 -> DQN::Update -> UpdateActorCritic, and
// DQN::Benchmark, src/dqn.cpp:487-498, which loops over it): host-drawn indices (std::mt19937 +
// uniform_int_distribution, SampleTransitionsFromMemory :501-509), staged to the device, and a BLOCKING read of
// (critic_loss, avg_q) after every update.  pipelined != 0: dqnhip_update_pipelined instead.
int dqnhip_benchmark_blocking(dqnhip_handle h, int32_t warmup, int32_t iterations, uint64_t seed, int32_t pipelined, float* avg_ms) {
  if (!h) return fail("null handle");
  if (iterations < 1) return fail("iterations must be >= 1");
  HIPCHK(hipSetDevice(h->cfg.device));
  int32_t size = 0;
  RC(dqnhip_memory_size(h, &size));
  if (size < 1) return fail("replay memory is empty");
  std::mt19937 rng((uint32_t)seed);
  std::vector<int32_t> idx(h->B);
  float loss = 0, avgq = 0;
  std::vector<int32_t> nxt(h->B);
  bool have_next = false;
  // pipelined == 3, the drop-in's -deferred_updates form: the draws of the other modes, a submit every sixteen updates, one collection
  // every 1000 updates and at the end
  std::vector<int32_t> pend; int n_pend = 0, since_collect = 0;
  std::vector<float> cl(1024), cq(1024);
  auto submit = [&]() -> int {
    const int rc = n_pend ? dqnhip_update_indexed_n(h, pend.data(), n_pend) : 0;
    n_pend = 0;
    return rc;
  };
  auto collect = [&]() -> int {
    RC(submit());
    for (int32_t got = 1; got > 0;) RC(dqnhip_collect_stats(h, cl.data(), cq.data(), (int32_t)cl.size(), &got));
    since_collect = 0;
    return 0;
  };
  if (pipelined == 3) pend.resize((size_t)kMultiU * h->B);
  auto one = [&]() -> int {
    if (pipelined == 3) {
      for (int i = 0; i < h->B; ++i) pend[(size_t)n_pend * h->B + i] = std::uniform_int_distribution<int>(0, size - 1)(rng);
      if (++n_pend == kMultiU) RC(submit());
      if (++since_collect == 1000) RC(collect());
      return 0;
    }
    if (pipelined == 2) {
      // the drop-in's chained form (dqn_dropin.cpp UpdateActorCritic): the next update's indices are drawn one call ahead
      // (drawing the prediction after next while the update runs — an enqueue-only call, then dqnhip_read_stats — was measured
      // too: 3 334-3 350 against 3 335-3 347 updates/s, the draw of 256 indices is ~1 us; not kept)
      if (have_next) idx.swap(nxt); else for (int32_t& i : idx) i = std::uniform_int_distribution<int>(0, size - 1)(rng);
      for (int32_t& i : nxt) i = std::uniform_int_distribution<int>(0, size - 1)(rng);
      have_next = true;
      return dqnhip_update_chained(h, idx.data(), nxt.data(), &loss, &avgq);
    }
    for (int32_t& i : idx) i = std::uniform_int_distribution<int>(0, size - 1)(rng);
    return pipelined ? dqnhip_update_pipelined(h, idx.data(), &loss, &avgq) : dqnhip_update(h, idx.data(), &loss, &avgq);
  };
  for (int i = 0; i < warmup; ++i) RC(one());
  if (pipelined == 3) RC(collect());
  HIPCHK(hipStreamSynchronize(h->stream));
  const auto t0 = std::chrono::steady_clock::now();
  for (int i = 0; i < iterations; ++i) RC(one());
  if (pipelined == 3) RC(collect());
  HIPCHK(hipStreamSynchronize(h->stream));
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (pipelined == 1) RC(dqnhip_read_stats(h, &loss, &avgq));      // drains the one outstanding read-back
  if (avg_ms) *avg_ms = (float)(ms / iterations);
  return 0;
}

}  // extern "C"
