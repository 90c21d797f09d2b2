// learner_eval.hip — what looks at a learner without training it: update diagnostics (dqnhip_diag_collect; the kernels and the order
// of every sum: diag_kernels.hip.h) and the replay sweep (dqnhip_evaluate_memory / dqnhip_per_refresh; the row kernel, the finaliser
// and the order of every sum: sweep_kernels.hip.h, which reduces in diag_kernels.hip.h's DiagLds — so the two share a unit; the
// forward launches of a chunk: sweep_forward, learner.hip).  include/dqnhip.h has the definitions.
#include "learner_internal.hip.h"
#include "diag_kernels.hip.h"
#include "sweep_kernels.hip.h"

namespace dqnhip_host {

// ---- update diagnostics --------------------------------------------------------------

struct DiagHost {
  std::vector<DiagSeg> segs;            // blobs (actor's, then critic's, dense Caffe order), then panels (pass-major)
  int n_blobs = 0, n_panels = 0, n_items = 0;
  DiagSeg* segs_dev = nullptr; DiagItem* items_dev = nullptr;
  DiagPart* parts = nullptr; DiagPart* out = nullptr; DiagRows* rows = nullptr;
  std::vector<int> blob_layer, blob_bias;
};
void diag_free(H* h) {
  DiagHost* d = h->diag;
  if (!d) return;
  hipFree(d->segs_dev); hipFree(d->items_dev); hipFree(d->parts); hipFree(d->out); hipFree(d->rows);
  delete d;
  h->diag = nullptr;
}
// the work table: one segment per blob and per panel, one item per (segment, chunk), the rows items first (they are the longest)
static int diag_build(H* h) {
  DiagHost* d = new DiagHost();
  h->diag = d;                          // (from here on diag_free releases whatever was allocated)
  std::vector<DiagItem> items;
  for (int r = 0; r < kDiagRowItems; ++r) items.push_back(DiagItem{-1, r});
  auto add = [&](DiagSeg s, int n_items) {
    s.first_item = d->n_items; s.n_items = n_items;
    for (int c = 0; c < n_items; ++c) items.push_back(DiagItem{(int)d->segs.size(), c});
    d->segs.push_back(s); d->n_items += n_items;
  };
  for (int net = 0; net < 2; ++net) {
    const NetLayout& l = layout_of(h, net);
    auto blob = [&](size_t off, int rows, int cols, int pitch, int layer, int is_bias) {
      DiagSeg s{};
      s.w = h->w[net] + off; s.wt = h->w[net + 2] + off; s.g = h->g[net] + off; s.m = h->m[net] + off; s.v = h->v[net] + off;
      s.type = DIAG_BLOB; s.net = net; s.rows = rows; s.cols = cols; s.pitch = pitch;
      add(s, (int)(((size_t)rows * pitch + kDiagChunk - 1) / kDiagChunk));
      d->blob_layer.push_back(layer); d->blob_bias.push_back(is_bias);
    };
    for (int i = 0; i < l.L; ++i) {
      blob(l.w_off[i], l.dims[i + 1], l.dims[i], l.kp[i], i, 0);
      blob(l.b_off[i], 1, l.dims[i + 1], l.dims[i + 1], i, 1);
    }
    const int Hh = l.dims[l.L];
    if (l.NH == kNO) {
      blob(l.hw_off, kNA, Hh, Hh, l.L, 0); blob(l.hb_off, 1, kNA, kNA, l.L, 1);
      blob(l.hw_off + (size_t)kNA * Hh, kNP, Hh, Hh, l.L + 1, 0); blob(l.hb_off + kNA, 1, kNP, kNP, l.L + 1, 1);
    } else { blob(l.hw_off, 1, Hh, Hh, l.L, 0); blob(l.hb_off, 1, 1, 1, l.L, 1); }
  }
  d->n_blobs = (int)d->segs.size();
  for (int p = 0; p < 5; ++p)
    for (int i = 1; i <= h->L; ++i) {
      const NetLayout& l = layout_of(h, p >= 2);
      DiagSeg s{};
      s.type = DIAG_PANEL; s.net = p; s.is16 = h->fp16 ? 1 : 0; s.rows = h->B; s.cols = l.dims[i];
      s.panel = h->fp16 ? (const void*)h->act16[p][i] : (const void*)h->act[p][i];
      s.pitch = h->fp16 ? h->k16[p >= 2][i] : l.kp[i];
      const int strip = h->fp16 ? 128 : 64;
      if (s.cols % strip) return fail("diagnostics: panel width %d is not a multiple of %d", s.cols, strip);
      add(s, s.cols / strip);
    }
  d->n_panels = 5 * h->L;
  auto alloc = [&](void** p, size_t bytes) -> int { HIPCHK(hipMalloc(p, bytes)); HIPCHK(hipMemsetAsync(*p, 0, bytes, h->stream)); return 0; };
  RC(alloc((void**)&d->segs_dev, d->segs.size() * sizeof(DiagSeg)));
  RC(alloc((void**)&d->items_dev, items.size() * sizeof(DiagItem)));
  RC(alloc((void**)&d->parts, (size_t)d->n_items * sizeof(DiagPart)));
  RC(alloc((void**)&d->out, d->segs.size() * sizeof(DiagPart)));
  RC(alloc((void**)&d->rows, sizeof(DiagRows)));
  HIPCHK(hipMemcpyAsync(d->segs_dev, d->segs.data(), d->segs.size() * sizeof(DiagSeg), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(d->items_dev, items.data(), items.size() * sizeof(DiagItem), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));       // (items is on this stack)
  return 0;
}
static void diag_moments(dqnhip_diag_moments& o, const DiagMomPart& p, int64_t count) {
  o.count = count; o.n_zero = p.n_zero; o.n_nonfinite = p.n_nonfinite; o.sum_abs = p.sum_abs; o.sum_sq = p.sum_sq; o.max_abs = p.max_abs; o.reserved = 0.0f;
}

// ---- replay sweep ----------------------------------------------------------------------

struct SweepHost {
  SweepDev* dev = nullptr; int* idx = nullptr; SweepPart* parts = nullptr; SweepOut* out = nullptr;
  float* rows[4] = {nullptr, nullptr, nullptr, nullptr}; int* match = nullptr;      // q, y, td, q_policy; [chunks x B] each
  DevState* flag_sink = nullptr;        // where a chunk's k_head_q_train raises its flag (the learner's sticky flags belong to updates)
  long long cap = 0;                    // the ring capacity the scratch was sized for (a learner may join another ring later: sweep_ready)
  int chunks = 0;                       // ceil(cap / B): the largest window
};
void sweep_free(H* h) {
  SweepHost* w = h->sweep;
  if (!w) return;
  hipFree(w->dev); hipFree(w->idx); hipFree(w->parts); hipFree(w->out); hipFree(w->match); hipFree(w->flag_sink);
  for (float* r : w->rows) hipFree(r);
  delete w;
  h->sweep = nullptr;
}
static int sweep_build(H* h) {
  SweepHost* w = new SweepHost();
  h->sweep = w;                         // (from here on sweep_free releases whatever was allocated)
  w->cap = RO(h)->ring.cap;
  w->chunks = (int)((w->cap + h->B - 1) / h->B);
  const size_t rows = (size_t)w->chunks * h->B;
  auto alloc = [&](void** p, size_t bytes) -> int { HIPCHK(hipMalloc(p, bytes)); HIPCHK(hipMemsetAsync(*p, 0, bytes, h->stream)); return 0; };
  RC(alloc((void**)&w->dev, sizeof(SweepDev)));
  RC(alloc((void**)&w->idx, (size_t)h->B * sizeof(int)));
  RC(alloc((void**)&w->parts, (size_t)w->chunks * sizeof(SweepPart)));
  RC(alloc((void**)&w->out, sizeof(SweepOut)));
  for (float*& r : w->rows) RC(alloc((void**)&r, rows * sizeof(float)));
  RC(alloc((void**)&w->match, rows * sizeof(int)));
  RC(alloc((void**)&w->flag_sink, sizeof(DevState)));
  return 0;
}
// the scratch, sized for the ring this learner uses NOW: dqnhip_share_replay_memory may have pointed it at a ring of another capacity
// since the last sweep — the window, the chunk slots and the row outputs are counted in that ring's transitions.  The captured chunks
// hold the old addresses: dropped with the scratch, behind everything enqueued
static int sweep_ready(H* h) {
  if (h->sweep && h->sweep->cap != (long long)RO(h)->ring.cap) {
    HIPCHK(hipStreamSynchronize(h->stream));
    for (auto& g : h->sweep_graph) if (g) { hipGraphExecDestroy(g); g = nullptr; }
    sweep_free(h);
  }
  if (!h->sweep && sweep_build(h)) { sweep_free(h); return 1; }
  return 0;
}
// one chunk: [refresh: slots of the chunk's indices] . the forward launches . the row kernel . [refresh: the update's write-back]
template <bool REFRESH>
static int sweep_chunk(H* h, const int*) {
  SweepHost* w = h->sweep;
  if (REFRESH) RC(per_fill_launch(h, w->idx));         // (before the row kernel, which leaves the NEXT chunk's indices in w->idx)
  RC(sweep_forward(h, w->idx, w->flag_sink));
  SweepRowsArgs a{};
  a.sw = w->dev; a.B = h->B;
  a.q = h->q1; a.y = h->y; a.q_policy = h->q2; a.mc = h->mb_mc; a.reward = h->mb_reward; a.term = h->mb_term;
  a.stored = h->Xc_tr + h->S; a.ld_stored = h->lc.kp[0]; a.aout16 = h->aout16;
  a.idx = w->idx; a.parts = w->parts;
  a.o_q = w->rows[0]; a.o_y = w->rows[1]; a.o_td = w->rows[2]; a.o_q_policy = w->rows[3]; a.o_match = w->match;
  a.td_abs = REFRESH ? h->per->td_abs : nullptr;
  HIPCHK(launch(h->stream, k_sweep_rows, dim3(1), dim3(256), 0, a));
  if (REFRESH) RC(per_update_launch(h));
  return 0;
}
// the two bodies a captured chunk is taken from (CaptureSpec::body's signature; a chunk's indices are its own, in device memory)
static int sweep_chunk_eval(H* h, const int* unused) { return sweep_chunk<false>(h, unused); }
static int sweep_chunk_refresh(H* h, const int* unused) { return sweep_chunk<true>(h, unused); }
static void sweep_row(dqnhip_diag_row& o, const SweepMom& m) { o.min = m.mn; o.max = m.mx; o.sum = m.s; o.sum_sq = m.ss; o.n_nonfinite = m.nnf; }

// what: the entry point's name.  rows: an evaluation's per-row outputs (null: none)
static int sweep_run(H* h, const char* what, bool refresh, int32_t first, int32_t n, dqnhip_sweep_report* out, const dqnhip_sweep_rows* rows) {
  if (out && out->struct_size != (int32_t)sizeof(dqnhip_sweep_report))
    return fail("%s: dqnhip_sweep_report.struct_size %d != %zu (ABI mismatch)", what, out->struct_size, sizeof(dqnhip_sweep_report));
  if (rows && rows->struct_size != (int32_t)sizeof(dqnhip_sweep_rows))
    return fail("%s: dqnhip_sweep_rows.struct_size %d != %zu (ABI mismatch)", what, rows->struct_size, sizeof(dqnhip_sweep_rows));
  if (refresh && !h->per) return fail("%s: the replay sweep refreshes priorities, and prioritized replay is not enabled on this learner (dqnhip_per_enable)", what);
  // (the sweep evaluates 1-step targets: on an n-step learner it would report 1-step errors and write 1-step priorities)
  RC(feature_refuse(h, kFeatNstep, what));
  if (h->next_phase != 0) return fail("%s: the replay sweep overwrites the update's panels, and a phased update is in progress (next phase %d)", what, h->next_phase);
  if (dp_grouped(h)) return fail("%s: the replay sweep is not available on a data-parallel learner (dp_world > 1, dqnhip_dp_init) in this version", what);
  if (h->fp16) return fail("%s: the replay sweep is not available with precision = DQNHIP_FP16 in this version", what);
  HIPCHK(hipSetDevice(h->cfg.device));
  RingUse ring_use(h);
  RC(refresh_ring(h));
  const long long size = RO(h)->h_size;
  if (first < 0 || first > size || n < -1 || (n >= 0 && (long long)first + n > size))
    return fail("%s: the replay sweep's window [%d,%lld) lies outside the memory [0,%lld)", what, first, n < 0 ? size : (long long)first + n, size);
  if (n < 0) n = (int32_t)(size - first);
  if (n == 0) {
    // a no-op: nothing is allocated, launched or captured; the report is all zero but for the iteration counters as they stand
    if (!out) return 0;
    int it[2];
    static_assert(offsetof(DevState, critic_iter) == offsetof(DevState, actor_iter) + sizeof(int), "actor_iter, critic_iter are adjacent");
    HIPCHK(hipMemcpyAsync(it, &h->st->actor_iter, sizeof it, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    memset(out, 0, sizeof *out);
    out->struct_size = (int32_t)sizeof *out;
    out->first = first; out->actor_iter = it[0]; out->critic_iter = it[1];
    return 0;
  }
  RC(sweep_ready(h));
  SweepHost* w = h->sweep;
  const int n_chunks = (n + h->B - 1) / h->B;
  if (n_chunks > w->chunks) return fail("internal: %s: %d chunks exceed the scratch's %d", what, n_chunks, w->chunks);
  h->epoch += 1;                         // the panels a dqnhip_update_chained chain left for its next call are about to be overwritten
  if (refresh) RC(per_sync_if_needed(h));
  HIPCHK(launch(h->stream, k_sweep_begin, dim3((h->B + 255) / 256), dim3(256), 0, w->dev, (int)first, (int)n, w->idx, h->B));
  RC(run_chunks(h, &h->sweep_graph[refresh ? 1 : 0], n_chunks, refresh ? sweep_chunk_refresh : sweep_chunk_eval));
  HIPCHK(launch(h->stream, k_sweep_final, dim3(1), dim3(256), 0, (const SweepDev*)w->dev, (const DevState*)h->st, (const SweepPart*)w->parts, h->B, w->out));
  SweepOut res{};
  HIPCHK(hipMemcpyAsync(&res, w->out, sizeof res, hipMemcpyDeviceToHost, h->stream));
  if (rows) {
    float* dst[4] = {rows->q, rows->y, rows->td, rows->q_policy};
    for (int k = 0; k < 4; ++k) if (dst[k]) HIPCHK(hipMemcpyAsync(dst[k], w->rows[k], (size_t)n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (rows->action_match) HIPCHK(hipMemcpyAsync(rows->action_match, w->match, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  if (!out) return 0;
  memset(out, 0, sizeof *out);
  out->struct_size = (int32_t)sizeof *out;
  out->first = first; out->n = res.n; out->n_chunks = res.n_chunks;
  out->n_terminal = res.n_terminal; out->n_action_match = res.n_match;
  dqnhip_diag_row* rr[kSweepQuantities] = {&out->q, &out->y, &out->td, &out->q_policy, &out->mc, &out->q_minus_mc, &out->reward};
  for (int k = 0; k < kSweepQuantities; ++k) sweep_row(*rr[k], res.mom[k]);
  memcpy(out->td_hist, res.hist, sizeof out->td_hist);
  out->actor_iter = res.actor_iter; out->critic_iter = res.critic_iter;
  return 0;
}

}  // namespace dqnhip_host

extern "C" {

int dqnhip_diag_collect(dqnhip_handle h, dqnhip_diag_report* out) {
  if (!out) return fail("dqnhip_diag_collect: null report");
  if (out->struct_size != (int32_t)sizeof(dqnhip_diag_report)) return fail("dqnhip_diag_report.struct_size %d != %zu (ABI mismatch)", out->struct_size, sizeof(dqnhip_diag_report));
  if (!h) return fail("dqnhip_diag_collect: null handle");
  if (h->next_phase != 0) return fail("dqnhip_diag_collect: diagnostics describe a finished update, and a phased update is in progress (next phase %d)", h->next_phase);
  if (h->w_owner) return fail("dqnhip_diag_collect: diagnostics are not available on a learner that reads another learner's parameters "
                              "(dqnhip_share_parameters: the arenas it steps are not all its own); collect on the owner");
  if (h->cfg.solver_type != DQNHIP_SOLVER_ADAM)
    return fail("dqnhip_diag_collect: diagnostics are not available with the %s solver (the step, lag and moment records are defined through Adam's m and v: DESIGN.md 9)",
                dqnhip_solver_name(h->cfg.solver_type));
  RC(feature_refuse(h, kFeatSched, "dqnhip_diag_collect"));      // (k_diag_prep prices the step as lr x adam_correction)
  if (h->dp_shard) return fail("dqnhip_diag_collect: diagnostics are not available with a sharded optimiser (DQNHIP_DP_SHARD_OPT: m and v of foreign slices are stale)");
  HIPCHK(hipSetDevice(h->cfg.device));
  if (!h->diag && diag_build(h)) { diag_free(h); return 1; }
  DiagHost* d = h->diag;
  const dqnhip_config& c = h->cfg;
  DiagPrepArgs pa{h->st, d->rows, {c.actor_lr, c.critic_lr}, c.momentum, c.momentum2};
  HIPCHK(launch(h->stream, k_diag_prep, dim3(1), dim3(64), 0, pa));
  DiagArgs a{};
  a.segs = d->segs_dev; a.items = d->items_dev; a.parts = d->parts; a.rows = d->rows; a.B = h->B; a.delta = c.delta;
  a.q_t = h->q_t; a.y = h->y; a.q1 = h->q1; a.q2 = h->q2; a.term = h->mb_term; a.aout16 = h->aout16; a.dA16 = h->dA16;
  if (h->per) { a.per_w = h->per->w; a.per_prob = h->per->prob; a.per_td = h->per->td_abs; }
  HIPCHK(launch(h->stream, k_diag_reduce, dim3(kDiagRowItems + d->n_items), dim3(256), 0, a));
  HIPCHK(launch(h->stream, k_diag_final, dim3((unsigned)d->segs.size()), dim3(256), 0, (const DiagSeg*)d->segs_dev, (const DiagPart*)d->parts, d->out));
  std::vector<DiagPart> res(d->segs.size());
  DiagRows rows{}; DevState s{};
  HIPCHK(hipMemcpyAsync(res.data(), d->out, res.size() * sizeof(DiagPart), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(&rows, d->rows, sizeof rows, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(&s, h->st, sizeof s, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));

  memset(out, 0, sizeof *out);
  out->struct_size = (int32_t)sizeof *out;
  out->n_blobs = d->n_blobs; out->n_panels = d->n_panels; out->has_per = h->per ? 1 : 0;
  double sumsq[2] = {0.0, 0.0};
  for (int b = 0; b < d->n_blobs; ++b) {
    const DiagSeg& sg = d->segs[b]; const DiagPart& p = res[b];
    dqnhip_diag_blob& o = out->blobs[b];
    o.net = sg.net; o.layer = d->blob_layer[b]; o.is_bias = d->blob_bias[b];
    const int64_t count = (int64_t)sg.rows * sg.cols;
    diag_moments(o.w, p.mom[0], count); diag_moments(o.g, p.mom[1], count); diag_moments(o.lag, p.mom[2], count); diag_moments(o.step, p.mom[3], count);
    memcpy(o.g_hist, p.hist, sizeof o.g_hist);
    sumsq[sg.net] += p.mom[1].sum_sq;
  }
  for (int q = 0; q < d->n_panels; ++q) {
    const DiagSeg& sg = d->segs[d->n_blobs + q]; const DiagPart& p = res[d->n_blobs + q];
    dqnhip_diag_panel& o = out->panels[q];
    o.pass = sg.net; o.layer = q % h->L + 1; o.rows = sg.rows; o.cols = sg.cols;
    o.n_negative = p.n_negative; o.dead_units = p.dead;
    diag_moments(o.a, p.mom[0], (int64_t)sg.rows * sg.cols);
    memcpy(o.hist, p.hist, sizeof o.hist);
  }
  dqnhip_diag_row* rr[5] = {&out->q_target, &out->y, &out->q_train, &out->q_policy, &out->td};
  for (int i = 0; i < 5; ++i) { rr[i]->min = rows.row[i].mn; rr[i]->max = rows.row[i].mx; rr[i]->sum = rows.row[i].sum; rr[i]->sum_sq = rows.row[i].sum_sq; rr[i]->n_nonfinite = rows.row[i].n_nonfinite; }
  out->n_terminal = rows.n_terminal;
  for (int j = 0; j < kNO; ++j) { out->actor_out[j].min = rows.act[j].mn; out->actor_out[j].max = rows.act[j].mx; out->actor_out[j].sum = rows.act[j].sum; out->actor_out[j].n_out_of_bounds = rows.act[j].n_oob; }
  out->dq_da_sum_abs = rows.dqda_sum_abs; out->dq_da_max_abs = rows.dqda_max_abs;
  out->per_w_min = rows.per_w_min; out->per_w_sum = rows.per_w_sum; out->per_prob_min = rows.per_prob_min; out->per_td_abs_max = rows.per_td_abs_max;
  out->actor_iter = s.actor_iter; out->critic_iter = s.critic_iter; out->critic_loss = s.critic_loss; out->avg_q = s.avg_q;
  for (int net = 0; net < 2; ++net) {
    const double norm = std::sqrt(sumsq[net]), clip = (double)c.clip_gradients;
    out->grad_norm[net] = norm;
    out->clip_scale[net] = (c.clip_gradients >= 0.0f && norm > clip) ? clip / norm : 1.0;
  }
  if (h->fp16) {
    out->fp16 = 1; out->loss_scale_mode = c.loss_scale_mode;
    out->loss_scale_critic = h->ls_c; out->loss_scale_dqda = h->ls_q; out->loss_scale_actor = h->ls_a;
    out->mult_critic = h->ls_dynamic ? s.ls_mult[1][0] : 1.0f; out->mult_actor = h->ls_dynamic ? s.ls_mult[0][0] : 1.0f;
  }
  return 0;
}

int dqnhip_evaluate_memory(dqnhip_handle h, int32_t first, int32_t n, dqnhip_sweep_report* out, const dqnhip_sweep_rows* rows) {
  if (!h) return fail("dqnhip_evaluate_memory: null handle");
  if (!out) return fail("dqnhip_evaluate_memory: null report");
  return sweep_run(h, "dqnhip_evaluate_memory", false, first, n, out, rows);
}

int dqnhip_per_refresh(dqnhip_handle h, int32_t first, int32_t n, dqnhip_sweep_report* out) {
  if (!h) return fail("dqnhip_per_refresh: null handle");
  return sweep_run(h, "dqnhip_per_refresh", true, first, n, out, nullptr);
}

}  // extern "C"
