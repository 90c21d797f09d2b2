// learner_create.hip — learner lifetime: the default config, dqnhip_create / dqnhip_destroy (every allocation of a learner and
// its release), and the buffers and graphs that come and go while it lives (host staging, acting scratch, captured launch
// sequences).  Host code only: the kernel attributes a new learner needs are set by prepare_kernels, in the translation unit
// that launches those kernels (learner.hip).
#include "learner_internal.hip.h"

namespace dqnhip_host {

int ensure_stage(H* h, size_t bytes) {
  if (bytes <= h->stage_bytes) return 0;
  if (h->stage_dev) { HIPCHK(hipStreamSynchronize(h->stream)); HIPCHK(hipFree(h->stage_dev)); h->stage_dev = nullptr; }
  bytes = round_up_z(bytes, 1 << 20);
  HIPCHK(hipMalloc(&h->stage_dev, bytes));
  h->stage_bytes = bytes;
  return 0;
}

// acting-time activation scratch for `rows` rows of the widest net
int ensure_act(H* h, int rows) {
  size_t need = 0;
  for (int i = 0; i <= h->L; ++i) need += (size_t)rows * std::max(h->la.kp[i], h->lc.kp[i]);
  need += (size_t)rows * (kAP + 1);
  if (need <= h->act_floats) return 0;
  if (h->act_buf) { HIPCHK(hipStreamSynchronize(h->stream)); HIPCHK(hipFree(h->act_buf)); h->act_buf = nullptr; }
  HIPCHK(hipMalloc(&h->act_buf, need * sizeof(float)));
  h->act_floats = need;
  return 0;
}

// fp16 acting panels for `rows` rows (a multiple of 64) of either net kind, zero-filled on allocation
int ensure_act16(H* h, int rows) {
  if (!h->fp16) return fail("internal: fp16 acting panels on an fp32 learner");
  if (rows < 64 || rows % 64) return fail("internal: fp16 acting panels hold whole 64-row tiles (got %d rows)", rows);
  if (rows <= h->actp16_rows) return 0;
  HIPCHK(hipStreamSynchronize(h->stream));
  for (int i = 0; i <= h->L; ++i) if (h->actp16[i]) { HIPCHK(hipFree(h->actp16[i])); h->actp16[i] = nullptr; }
  if (h->actp16_out) { HIPCHK(hipFree(h->actp16_out)); h->actp16_out = nullptr; }
  h->actp16_rows = 0;
  for (int i = 0; i <= h->L; ++i) {
    const size_t n = (size_t)rows * act16_width(h, i);
    HIPCHK(hipMalloc(&h->actp16[i], n * sizeof(h16)));
    HIPCHK(hipMemsetAsync(h->actp16[i], 0, n * sizeof(h16), h->stream));
  }
  HIPCHK(hipMalloc(&h->actp16_out, (size_t)rows * (kAP + 1) * sizeof(float)));
  HIPCHK(hipMemsetAsync(h->actp16_out, 0, (size_t)rows * (kAP + 1) * sizeof(float), h->stream));
  h->actp16_rows = rows;
  return 0;
}

void drop_graphs(H* h) {
  for (auto& g : h->graph_exec) if (g) { hipGraphExecDestroy(g); g = nullptr; }
  for (auto& g : h->graph_small) if (g) { hipGraphExecDestroy(g); g = nullptr; }
  for (auto& bank : h->ix_graph) for (auto& g : bank) if (g) { hipGraphExecDestroy(g); g = nullptr; }
  for (int& n : h->ix_nodes) n = 0;
  for (auto& g : h->sweep_graph) if (g) { hipGraphExecDestroy(g); g = nullptr; }
  if (h->dp_graph) { hipGraphExecDestroy(h->dp_graph); h->dp_graph = nullptr; }
  if (h->dp_graph_n) { hipGraphExecDestroy(h->dp_graph_n); h->dp_graph_n = nullptr; }
  h->dp_graph_failed = false; h->dp_graph_n_failed = false; h->graph_failed = false;
}

}  // namespace dqnhip_host

extern "C" {

void dqnhip_default_config(dqnhip_config* c, int32_t state_size) {
  memset(c, 0, sizeof *c);
  c->struct_size = (int32_t)sizeof *c;
  c->minibatch = 32;                       // src/dqn.hpp:19
  c->state_size = state_size;
  c->num_hidden = 4;                       // src/dqn.cpp:425,449
  c->hidden[0] = 1024; c->hidden[1] = 512; c->hidden[2] = 256; c->hidden[3] = 128;
  c->replay_capacity = 500000;             // src/dqn.cpp:25
  c->soft_update_freq = 1;                 // :23
  c->gamma = .99; c->beta = .5; c->tau = .001;   // :24, :31, :22
  c->actor_lr = 0.00001f; c->critic_lr = 0.001f; // src/dqn_main.cpp:33-34
  c->momentum = .95f; c->momentum2 = .999f;      // src/dqn_main.cpp:31-32
  c->delta = 1e-8f;                        // Caffe SolverParameter.delta default
  c->clip_gradients = 10.f;                // src/dqn_main.cpp:35
  c->device = 0; c->dp_world = 1; c->dp_rank = 0; c->use_graph = 0; c->seed = 1;
  c->loss_scale_mode = DQNHIP_LOSS_SCALE_STATIC;
  c->loss_scale_growth_interval = 2000;                // the customary value of mixed-precision trainers; not measured here
  c->loss_scale_min_mult = 1.0f / 4096.0f;             // ls_q x 2^-12 = 1: no scaling left
  c->loss_scale_max_mult = 1.0f;                       // never above the built-in scales unless asked
  c->solver_type = DQNHIP_SOLVER_ADAM;                 // FLAGS_solver, src/dqn_main.cpp:30
  c->rms_decay = .99f;                                 // Caffe SolverParameter.rms_decay default
}

const char* dqnhip_solver_name(int32_t solver_type) {
  static const char* const kNames[] = {"Adam", "SGD", "Nesterov", "AdaGrad", "RMSProp", "AdaDelta"};
  return solver_type >= 0 && solver_type <= DQNHIP_SOLVER_ADADELTA ? kNames[solver_type] : nullptr;
}

const char* dqnhip_lr_policy_name(int32_t lr_policy) { return lr_policy_name(lr_policy); }

int dqnhip_get_config(dqnhip_handle h, dqnhip_config* out) {
  if (!h || !out) return fail("null argument");
  *out = h->cfg;
  out->stream = nullptr; out->grad_arena = nullptr; out->grad_arena_bytes = 0;
  return 0;
}

size_t dqnhip_grad_arena_bytes(const dqnhip_config* cfg) {
  dqnhip_config full;
  if (validate(cfg, &full)) return 0;
  NetLayout la, lc;
  layout_init(la, full.state_size, full, true);
  layout_init(lc, full.state_size + kNO, full, false);
  return grad_arena_floats(la, lc) * sizeof(float);
}

static int create_impl(H* h, const dqnhip_config* cfg);

int dqnhip_create(const dqnhip_config* cfg, dqnhip_handle* out) {
  if (!out) return fail("out is null");
  *out = nullptr;
  dqnhip_config full;
  RC(validate(cfg, &full));
  cfg = &full;
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (cfg->device < 0 || cfg->device >= ndev) return fail("device %d not available (%d visible)", cfg->device, ndev);
  HIPCHK(hipSetDevice(cfg->device));
  H* h = new H();
  const int rc = create_impl(h, cfg);
  if (rc) {                                  // free whatever was allocated; keep the first error message
    const std::string msg = g_err;
    dqnhip_destroy(h);
    g_err = msg;
    return rc;
  }
  *out = h;
  return 0;
}

static int create_impl(H* h, const dqnhip_config* cfg) {
  h->cfg = *cfg; h->B = cfg->minibatch; h->S = cfg->state_size; h->L = cfg->num_hidden;
  layout_init(h->la, h->S, *cfg, true);
  layout_init(h->lc, h->S + kNO, *cfg, false);
  if (cfg->stream) h->stream = (hipStream_t)cfg->stream;
  else { HIPCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)); h->own_stream = true; }
  const int B = h->B, L = h->L;
  auto dalloc = [&](float** p, size_t n) -> int {
    HIPCHK(hipMalloc(p, n * sizeof(float)));
    HIPCHK(hipMemsetAsync(*p, 0, n * sizeof(float), h->stream));
    return 0;
  };
  for (int i = 0; i < 4; ++i) RC(dalloc(&h->w[i], layout_of(h, i).arena));
  for (int i = 0; i < 2; ++i) { RC(dalloc(&h->m[i], layout_of(h, i).arena)); RC(dalloc(&h->v[i], layout_of(h, i).arena)); }
  const size_t gfl = grad_arena_floats(h->la, h->lc);
  if (cfg->grad_arena) {
    if (cfg->grad_arena_bytes < gfl * sizeof(float)) return fail("grad_arena too small: %zu < %zu", cfg->grad_arena_bytes, gfl * sizeof(float));
    h->grad_base = (float*)cfg->grad_arena;
    HIPCHK(hipMemsetAsync(h->grad_base, 0, gfl * sizeof(float), h->stream));
  } else { RC(dalloc(&h->grad_base, gfl)); h->own_grad = true; }
  h->g[0] = h->grad_base; h->g[1] = h->grad_base + h->la.arena + 64;
  // replay ring
  Ring& r = h->ring;
  r.cap = cfg->replay_capacity; r.S = h->S; r.SP = round_up(h->S, 64);
  RC(dalloc(&r.state, (size_t)r.cap * r.SP)); RC(dalloc(&r.next, (size_t)r.cap * r.SP));
  RC(dalloc(&r.act, (size_t)r.cap * kAP)); RC(dalloc(&r.reward, r.cap)); RC(dalloc(&r.mc, r.cap));
  HIPCHK(hipMalloc(&r.term, r.cap)); HIPCHK(hipMemsetAsync(r.term, 0, r.cap, h->stream));
  HIPCHK(hipMalloc(&h->st, sizeof(DevState))); HIPCHK(hipMemsetAsync(h->st, 0, sizeof(DevState), h->stream));
  if (has_policy(h)) {      // (a fixed learner allocates nothing and passes null: GatherArgs::sched)
    h->sched = schedule_of(*cfg);
    HIPCHK(hipMalloc(&h->sched_dev, sizeof(LrSchedule)));
    HIPCHK(hipMemcpyAsync(h->sched_dev, &h->sched, sizeof(LrSchedule), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  HIPCHK(hipMalloc(&h->done_counter, sizeof(int))); HIPCHK(hipMemsetAsync(h->done_counter, 0, sizeof(int), h->stream));
  // panels and activations
  RC(dalloc(&h->Xa_s, (size_t)B * h->la.kp[0])); RC(dalloc(&h->Xa_n, (size_t)B * h->la.kp[0]));
  RC(dalloc(&h->Xc_tr, (size_t)B * h->lc.kp[0])); RC(dalloc(&h->Xc_pl, (size_t)B * h->lc.kp[0]));
  h->Xa_s2[0] = h->Xa_s; h->Xc_pl2[0] = h->Xc_pl;
  if (!h->fp16) { RC(dalloc(&h->Xa_s2[1], (size_t)B * h->la.kp[0])); RC(dalloc(&h->Xc_pl2[1], (size_t)B * h->lc.kp[0])); }
  else { h->Xa_s2[1] = nullptr; h->Xc_pl2[1] = nullptr; }
  RC(dalloc(&h->Xc_nx, (size_t)B * h->lc.kp[0]));
  h->act[0][0] = h->Xa_n; h->act[1][0] = h->Xa_s; h->act[2][0] = h->Xc_nx; h->act[3][0] = h->Xc_tr; h->act[4][0] = h->Xc_pl;
  for (int p = 0; p < 5; ++p)
    for (int i = 1; i <= L; ++i) RC(dalloc(&h->act[p][i], (size_t)B * layout_of(h, p >= 2).kp[i]));
  for (int i = 0; i <= L; ++i) { RC(dalloc(&h->dZa[i], (size_t)B * h->la.kp[i])); RC(dalloc(&h->dZc[i], (size_t)B * h->lc.kp[i])); }
  RC(dalloc(&h->U3, (size_t)B * h->lc.kp[L]));        // the training pass's head-seed panel (k_dgrad_qtrain)
  for (int j = 0; j < 2; ++j) RC(dalloc(&h->qdot[j], (size_t)B * (h->lc.kp[L] / 16)));
  RC(dalloc(&h->Wact_t, (size_t)kNO * h->lc.dims[1]));  // critic_target's first-layer action-column weights, transposed (GemmProblem::xcopy_dst)
  RC(dalloc(&h->Zs, (size_t)B * h->lc.kp[1]));   // the state half of critic_target's first layer (first_layers_launch)
  RC(dalloc(&h->mb_reward, B)); RC(dalloc(&h->mb_mc, B)); RC(dalloc(&h->mb_term, B));
  HIPCHK(hipMalloc(&h->mb_idx, B * sizeof(int)));
  HIPCHK(hipHostMalloc((void**)&h->idx_pinned, B * sizeof(int), hipHostMallocMapped));
  // [0, 3) the tick's {loss, avg_q, flags}; [8] dqnhip_skipped_steps; [16, 32) dqnhip_get_loss_scale
  HIPCHK(hipHostMalloc((void**)&h->pinned_stats, 128, hipHostMallocMapped));
  memset(h->pinned_stats, 0, 128);
  { void* d = nullptr; HIPCHK(hipHostGetDevicePointer(&d, h->idx_pinned, 0)); h->idx_pinned_dev = (const int*)d;
    HIPCHK(hipHostGetDevicePointer(&d, h->pinned_stats, 0)); h->stats_dev = (float*)d; }
  RC(dalloc(&h->aout_t16, (size_t)B * kAP)); RC(dalloc(&h->aout16, (size_t)B * kAP)); RC(dalloc(&h->dA16, (size_t)B * kAP));
  RC(dalloc(&h->q_t, B)); RC(dalloc(&h->q1, B)); RC(dalloc(&h->q2, B)); RC(dalloc(&h->y, B)); RC(dalloc(&h->dq, B));
  h->n_head_blocks = (B + 3) / 4;
  RC(dalloc(&h->loss_partial, h->n_head_blocks));
  HIPCHK(hipMalloc(&h->q_partial, B * sizeof(double)));
  HIPCHK(hipMemsetAsync(h->q_partial, 0, B * sizeof(double), h->stream));
  RC(dalloc(&h->part[0], h->la.n_part)); RC(dalloc(&h->part[1], h->lc.n_part));
  h->n_part_dp = 1024; RC(dalloc(&h->part_dp, h->n_part_dp));
  {
    const int Hmax = std::max(h->la.dims[L], h->lc.dims[L]);
    RC(dalloc(&h->head_slab, (size_t)64 * (Hmax / 64) * kNO * 64 + 64 * 16));
    if (B >= 1024 && B % 64 == 0) RC(dalloc(&h->head_slab2, (size_t)(B / 64) * kNO * Hmax + (size_t)(B / 64) * 16));
    HIPCHK(hipMalloc(&h->head_ticket, (Hmax / 64) * sizeof(int)));
    HIPCHK(hipMemsetAsync(h->head_ticket, 0, (Hmax / 64) * sizeof(int), h->stream));
  }
  if (cfg->precision == DQNHIP_FP16) {
    h->fp16 = true;
    const float user = cfg->loss_scale > 0.f ? cfg->loss_scale : 1.0f;
    h->ls_c = 16.0f * (float)(B * cfg->dp_world) * user;   // dq = (q-y)/B_global: back to O(q-y)
    h->ls_q = 4096.0f * user;
    h->ls_a = 16384.0f * user;
    h->ls_dynamic = cfg->loss_scale_mode == DQNHIP_LOSS_SCALE_DYNAMIC;
    if (h->ls_dynamic) {                                   // both multipliers start at 1 (DevState::ls_mult; the rest of it stays zero)
      const float one[2][2] = {{1.0f, 1.0f}, {1.0f, 1.0f}};
      HIPCHK(hipMemcpyAsync(h->st->ls_mult, one, sizeof one, hipMemcpyHostToDevice, h->stream));
      HIPCHK(hipStreamSynchronize(h->stream));
    }
    auto halloc = [&](h16** p, size_t n) -> int {
      HIPCHK(hipMalloc(p, n * sizeof(h16)));
      HIPCHK(hipMemsetAsync(*p, 0, n * sizeof(h16), h->stream));
      h->allocs16.push_back((void*)*p);
      return 0;
    };
    for (int kind = 0; kind < 2; ++kind) {
      const NetLayout& l = kind ? h->lc : h->la;
      for (int i = 0; i <= L; ++i) h->k16[kind][i] = l.kp[i];
    }
    for (int net = 0; net < 4; ++net) {
      const NetLayout& l = layout_of(h, net);
      RC(halloc(&h->w16a[net], l.arena));
      for (int i = 0; i < L; ++i) h->w16[net][i] = h->w16a[net] + l.w_off[i];
    }
    for (int p = 0; p < 5; ++p) {
      const int kind = p >= 2;
      for (int i = 0; i <= L; ++i) RC(halloc(&h->act16[p][i], (size_t)B * h->k16[kind][i]));
    }
    for (int kind = 0; kind < 2; ++kind)
      for (int i = 0; i <= L; ++i) RC(halloc(&h->dZ16[kind][i], (size_t)B * h->k16[kind][i]));
  }
  // weights: gaussian(std 0.01), zero bias (src/dqn.cpp:350-352); targets = hard copy (:660-661)
  {
    std::mt19937_64 rng(cfg->seed * 0x9E3779B97F4A7C15ull + 12345);
    std::normal_distribution<float> nd(0.0f, 0.01f);
    for (int net = 0; net < 2; ++net) {
      const NetLayout& l = layout_of(h, net);
      std::vector<float> dense(l.dense, 0.0f), arena;
      size_t d = 0;
      for (int i = 0; i < l.L; ++i) {
        const size_t nw = (size_t)l.dims[i + 1] * l.dims[i];
        for (size_t e = 0; e < nw; ++e) dense[d + e] = nd(rng);
        d += nw + l.dims[i + 1];
      }
      const int Hh = l.dims[l.L];
      if (net == 0) {
        for (size_t e = 0; e < (size_t)kNA * Hh; ++e) dense[d + e] = nd(rng);
        d += (size_t)kNA * Hh + kNA;
        for (size_t e = 0; e < (size_t)kNP * Hh; ++e) dense[d + e] = nd(rng);
      } else {
        for (size_t e = 0; e < (size_t)Hh; ++e) dense[d + e] = nd(rng);
      }
      dense_to_arena(l, dense.data(), arena);
      HIPCHK(hipMemcpyAsync(h->w[net], arena.data(), l.arena * sizeof(float), hipMemcpyHostToDevice, h->stream));
      HIPCHK(hipStreamSynchronize(h->stream));
      HIPCHK(hipMemcpyAsync(h->w[net + 2], h->w[net], l.arena * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    }
  }
  RC(prepare_kernels(h));
  RC(sync_dirty16(h));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

int dqnhip_destroy(dqnhip_handle h) {
  if (!h) return 0;
  if (h->sharers > 0) return fail("dqnhip_destroy: %d learner(s) still share this learner's layers / replay memory; destroy them first", h->sharers);
  if (h->w_owner) h->w_owner->sharers -= 1;
  if (h->ring_owner) h->ring_owner->sharers -= 1;
  if (h->ring_ev) hipEventDestroy(h->ring_ev);
  hipSetDevice(h->cfg.device);
  state_async_free(h);                  // (a save in flight finishes its file first)
  dp_destroy_impl(h, false);
  hipStreamSynchronize(h->stream);
  for (auto& r : h->recs) { hipEventDestroy(r.a); hipEventDestroy(r.b); }
  drop_graphs(h);
  per_free(h);
  nstep_free(h);
  smooth_free(h);
  diag_free(h);
  sweep_free(h);
  for (int i = 0; i < 2; ++i) {
    if (h->pipe_ev[i]) hipEventDestroy(h->pipe_ev[i]);
    if (h->pipe_idx_pinned[i]) hipHostFree(h->pipe_idx_pinned[i]);
    if (h->pipe_stats[i]) hipHostFree(h->pipe_stats[i]);
  }
  for (int b = 0; b < kIxBanks; ++b) {
    if (h->ix_ev[b]) hipEventDestroy(h->ix_ev[b]);
    if (h->ix_idx[b]) hipHostFree(h->ix_idx[b]);
    if (h->ix_stats[b]) hipHostFree(h->ix_stats[b]);
  }
  for (int i = 0; i < 4; ++i) hipFree(h->w[i]);
  for (int i = 0; i < 2; ++i) { hipFree(h->m[i]); hipFree(h->v[i]); hipFree(h->part[i]); }
  if (h->own_grad) hipFree(h->grad_base);
  hipFree(h->ring.state); hipFree(h->ring.next); hipFree(h->ring.act); hipFree(h->ring.reward);
  hipFree(h->ring.mc); hipFree(h->ring.term); hipFree(h->st); hipFree(h->done_counter);
  hipFree(h->Xa_s2[0]); hipFree(h->Xa_s2[1]); hipFree(h->Xa_n); hipFree(h->Xc_tr); hipFree(h->Xc_pl2[0]); hipFree(h->Xc_pl2[1]); hipFree(h->Xc_nx);
  for (int p = 0; p < 5; ++p) for (int i = 1; i <= h->L; ++i) hipFree(h->act[p][i]);
  for (int i = 0; i <= h->L; ++i) { hipFree(h->dZa[i]); hipFree(h->dZc[i]); }
  hipFree(h->mb_reward); hipFree(h->mb_mc); hipFree(h->mb_term); hipFree(h->mb_idx); hipFree(h->U3); hipFree(h->qdot[0]); hipFree(h->qdot[1]); hipFree(h->Zs); hipFree(h->Wact_t);
  hipHostFree(h->idx_pinned); hipHostFree(h->pinned_stats);
  for (int i = 0; i < 2; ++i) if (h->idx_next_pinned[i]) hipHostFree(h->idx_next_pinned[i]);
  hipFree(h->aout_t16); hipFree(h->aout16); hipFree(h->dA16);
  hipFree(h->q_t); hipFree(h->q1); hipFree(h->q2); hipFree(h->y); hipFree(h->dq);
  hipFree(h->loss_partial); hipFree(h->q_partial); hipFree(h->part_dp); hipFree(h->head_slab); hipFree(h->head_ticket); if (h->head_slab2) hipFree(h->head_slab2);
  for (void* p : h->allocs16) hipFree(p);
  if (h->stage_dev) hipFree(h->stage_dev);
  if (h->shard_total) hipFree(h->shard_total);
  if (h->sched_dev) hipFree(h->sched_dev);
  if (h->act_buf) hipFree(h->act_buf);
  for (int i = 0; i <= h->L; ++i) if (h->actp16[i]) hipFree(h->actp16[i]);
  if (h->actp16_out) hipFree(h->actp16_out);
  if (h->own_stream) hipStreamDestroy(h->stream);
  delete h;
  return 0;
}

}  // extern "C"
