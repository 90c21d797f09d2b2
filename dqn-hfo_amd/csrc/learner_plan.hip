// learner_plan.hip — what is decided before anything is launched: the error channel, the parameter-arena layout and its dense
// (Caffe order) image, config validation, the shape predicates of the launch schedules and the plan (plan_of: which merged forms
// a learner's update takes).  Host code only: this translation unit launches no kernel and embeds no device code.
#include "learner_internal.hip.h"

namespace dqnhip_host {

thread_local std::string g_err;

void layout_init(NetLayout& l, int in_dim, const dqnhip_config& c, bool actor) {
  l.L = c.num_hidden; l.in_dim = in_dim; l.NH = actor ? kNO : 1;
  // fp16 mode: 128-wide first panel so that the fp16 weight arena mirrors this one offset for offset
  l.dims[0] = in_dim; l.kp[0] = round_up(in_dim, c.precision == DQNHIP_FP16 ? 128 : 64);
  for (int i = 0; i < l.L; ++i) { l.dims[i + 1] = c.hidden[i]; l.kp[i + 1] = c.hidden[i]; }
  size_t off = 0, dense = 0;
  int part = 0;
  for (int i = 0; i < l.L; ++i) {
    l.w_off[i] = off; off += (size_t)l.dims[i + 1] * l.kp[i];
    l.b_off[i] = off; off += round_up(l.dims[i + 1], 64);
    dense += (size_t)l.dims[i + 1] * l.dims[i] + l.dims[i + 1];
    // one slot per wgrad tile; the first layer may run the 16-output tiles of wgrad_narrow_body
    l.part_off[i] = part; part += (l.kp[i] / 64) * (l.dims[i + 1] / (i == 0 ? 16 : 64));
  }
  const int H = l.dims[l.L];
  l.hw_off = off; off += round_up_z((size_t)l.NH * H, 64);
  l.hb_off = off; off += 64;
  dense += (size_t)l.NH * H + l.NH;
  l.part_off[l.L] = part; part += std::max((H / 64) * l.NH, H / kRiderCW);    // k_head_bwd uses the first H/64, head_wgrad_rider H/8, k_head_wred one per (head, 64 columns)
  // fp16 learner: the bias gradients come from their own workgroups (k_db16_cols, one per 64 columns): their slots
  l.part_db = part;
  for (int i = 0; i < l.L; ++i) part += l.dims[i + 1] / 64;
  l.arena = round_up_z(off, 64);
  l.dense = dense;
  l.n_part = part;
}

// ---- dense (Caffe order) <-> internal arena ----------------------------------
void dense_to_arena(const NetLayout& l, const float* dense, std::vector<float>& arena) {
  arena.assign(l.arena, 0.0f);
  size_t d = 0;
  for (int i = 0; i < l.L; ++i) {
    const int N = l.dims[i + 1], K = l.dims[i], KP = l.kp[i];
    for (int n = 0; n < N; ++n) memcpy(&arena[l.w_off[i] + (size_t)n * KP], dense + d + (size_t)n * K, K * sizeof(float));
    d += (size_t)N * K;
    memcpy(&arena[l.b_off[i]], dense + d, N * sizeof(float)); d += N;
  }
  const int Hh = l.dims[l.L];
  if (l.NH == kNO) {  // action_layer.W[4,H] .b[4] actionpara_layer.W[6,H] .b[6]
    memcpy(&arena[l.hw_off], dense + d, (size_t)kNA * Hh * sizeof(float)); d += (size_t)kNA * Hh;
    memcpy(&arena[l.hb_off], dense + d, kNA * sizeof(float)); d += kNA;
    memcpy(&arena[l.hw_off + (size_t)kNA * Hh], dense + d, (size_t)kNP * Hh * sizeof(float)); d += (size_t)kNP * Hh;
    memcpy(&arena[l.hb_off + kNA], dense + d, kNP * sizeof(float)); d += kNP;
  } else {
    memcpy(&arena[l.hw_off], dense + d, (size_t)Hh * sizeof(float)); d += Hh;
    arena[l.hb_off] = dense[d]; d += 1;
  }
}
void arena_to_dense(const NetLayout& l, const std::vector<float>& arena, float* dense) {
  size_t d = 0;
  for (int i = 0; i < l.L; ++i) {
    const int N = l.dims[i + 1], K = l.dims[i], KP = l.kp[i];
    for (int n = 0; n < N; ++n) memcpy(dense + d + (size_t)n * K, &arena[l.w_off[i] + (size_t)n * KP], K * sizeof(float));
    d += (size_t)N * K;
    memcpy(dense + d, &arena[l.b_off[i]], N * sizeof(float)); d += N;
  }
  const int Hh = l.dims[l.L];
  if (l.NH == kNO) {
    memcpy(dense + d, &arena[l.hw_off], (size_t)kNA * Hh * sizeof(float)); d += (size_t)kNA * Hh;
    memcpy(dense + d, &arena[l.hb_off], kNA * sizeof(float)); d += kNA;
    memcpy(dense + d, &arena[l.hw_off + (size_t)kNA * Hh], (size_t)kNP * Hh * sizeof(float)); d += (size_t)kNP * Hh;
    memcpy(dense + d, &arena[l.hb_off + kNA], kNP * sizeof(float)); d += kNP;
  } else {
    memcpy(dense + d, &arena[l.hw_off], (size_t)Hh * sizeof(float)); d += Hh;
    dense[d] = arena[l.hb_off]; d += 1;
  }
}


// a positive, normal power of two (a loss-scale multiplier: halving and doubling it, and multiplying by it, are exact)
bool is_pow2(float x) {
  int e = 0;
  return std::isfinite(x) && x >= 1.17549435e-38f && std::frexp(x, &e) == 0.5f;
}

static_assert(kLrFixed == DQNHIP_LR_FIXED && kLrStep == DQNHIP_LR_STEP && kLrExp == DQNHIP_LR_EXP && kLrInv == DQNHIP_LR_INV &&
              kLrMultistep == DQNHIP_LR_MULTISTEP && kLrPoly == DQNHIP_LR_POLY && kLrSigmoid == DQNHIP_LR_SIGMOID &&
              kLrMaxStepvalues == DQNHIP_LR_MAX_STEPVALUES && kRegL2 == DQNHIP_REG_L2 && kRegL1 == DQNHIP_REG_L1, "lr_schedule.hip.h mirrors dqnhip.h");

LrSchedule schedule_of(const dqnhip_config& c) {
  LrSchedule s{};
  s.policy = c.lr_policy; s.base_lr[0] = c.actor_lr; s.base_lr[1] = c.critic_lr; s.gamma = c.lr_gamma; s.power = c.lr_power;
  s.stepsize = c.lr_stepsize; s.max_iter = c.lr_max_iter; s.n_stepvalue = c.lr_n_stepvalue;
  for (int i = 0; i < kLrMaxStepvalues; ++i) s.stepvalue[i] = c.lr_stepvalue[i];
  return s;
}

int validate(const dqnhip_config* in, dqnhip_config* full) {
  if (!in) return fail("config is null");
  // the struct as it is, or as it was before the lr_policy .. regularization_type block was put in behind rms_decay (a caller compiled
  // against that header: its tail — tuning_flags and the loss-scale fields — sits 96 bytes lower; the block reads as zero)
  constexpr size_t kBlock0 = offsetof(dqnhip_config, lr_policy), kBlock1 = offsetof(dqnhip_config, tuning_flags);
  if (in->struct_size == (int32_t)sizeof(dqnhip_config)) *full = *in;
  else if (in->struct_size == (int32_t)(sizeof(dqnhip_config) - (kBlock1 - kBlock0))) {
    memset(full, 0, sizeof *full);
    memcpy(full, in, kBlock0);
    memcpy((char*)full + kBlock1, (const char*)in + kBlock0, sizeof(dqnhip_config) - kBlock1);
    full->struct_size = (int32_t)sizeof(dqnhip_config);
  }
  else return fail("dqnhip_config.struct_size %d != %zu (ABI mismatch)", in->struct_size, sizeof(dqnhip_config));
  const dqnhip_config* c = full;
  if (c->minibatch <= 0 || c->minibatch % 32) return fail("minibatch must be a positive multiple of 32 (got %d)", c->minibatch);
  if (c->state_size < 1) return fail("state_size must be >= 1");
  if (c->num_hidden < 1 || c->num_hidden > kMaxL) return fail("num_hidden out of range");
  for (int i = 0; i < c->num_hidden; ++i)
    if (c->hidden[i] <= 0 || c->hidden[i] % 64) return fail("hidden[%d]=%d must be a positive multiple of 64", i, c->hidden[i]);
  if (c->replay_capacity < 2) return fail("replay_capacity must be >= 2");
  if (c->soft_update_freq < 1) return fail("soft_update_freq must be >= 1");
  if (c->dp_world < 1 || c->dp_rank < 0 || c->dp_rank >= c->dp_world) return fail("bad dp_world/dp_rank");
  if (c->precision != DQNHIP_FP32 && c->precision != DQNHIP_FP16) return fail("precision must be DQNHIP_FP32 or DQNHIP_FP16");
  if (c->precision == DQNHIP_FP16) {
    if (c->minibatch % 128) return fail("fp16 mode: minibatch must be a multiple of 128 (got %d)", c->minibatch);
    for (int i = 0; i < c->num_hidden; ++i)
      if (c->hidden[i] % 128) return fail("fp16 mode: hidden[%d]=%d must be a multiple of 128", i, c->hidden[i]);
  }
  if (c->loss_scale_mode != DQNHIP_LOSS_SCALE_STATIC && c->loss_scale_mode != DQNHIP_LOSS_SCALE_DYNAMIC)
    return fail("loss_scale_mode must be DQNHIP_LOSS_SCALE_STATIC or DQNHIP_LOSS_SCALE_DYNAMIC (got %d)", c->loss_scale_mode);
  if (c->loss_scale_mode == DQNHIP_LOSS_SCALE_DYNAMIC) {      // (static mode reads none of the other three fields)
    if (c->precision != DQNHIP_FP16) return fail("loss_scale_mode = dynamic needs precision = DQNHIP_FP16 (an fp32 learner scales nothing)");
    if (c->dp_world > 1) return fail("loss_scale_mode = dynamic needs dp_world = 1 (got %d): the data-parallel form has never run", c->dp_world);
    if (c->loss_scale_growth_interval < 0) return fail("loss_scale_growth_interval must be >= 0 (0: never grow; got %d)", c->loss_scale_growth_interval);
    if (!is_pow2(c->loss_scale_min_mult)) return fail("loss_scale_min_mult must be a power of two (got %g)", (double)c->loss_scale_min_mult);
    if (!is_pow2(c->loss_scale_max_mult)) return fail("loss_scale_max_mult must be a power of two (got %g)", (double)c->loss_scale_max_mult);
    if (c->loss_scale_min_mult > c->loss_scale_max_mult)
      return fail("loss_scale_min_mult %g > loss_scale_max_mult %g", (double)c->loss_scale_min_mult, (double)c->loss_scale_max_mult);
    if (c->loss_scale_min_mult > 1.0f) return fail("loss_scale_min_mult %g > 1: the multipliers start at 1", (double)c->loss_scale_min_mult);
    if (c->loss_scale_max_mult < 1.0f) return fail("loss_scale_max_mult %g < 1: the multipliers start at 1", (double)c->loss_scale_max_mult);
  }
  // Caffe's solver constructors (adagrad / rmsprop: CHECK_EQ(0, momentum); rmsprop: CHECK_GE(rms_decay, 0), CHECK_LT(rms_decay, 1))
  const char* solver = dqnhip_solver_name(c->solver_type);
  if (!solver) return fail("unknown solver_type %d (DQNHIP_SOLVER_ADAM .. DQNHIP_SOLVER_ADADELTA)", c->solver_type);
  if (c->solver_type == DQNHIP_SOLVER_ADAGRAD && c->momentum != 0.0f) return fail("Momentum cannot be used with AdaGrad. (momentum = %g)", (double)c->momentum);
  if (c->solver_type == DQNHIP_SOLVER_RMSPROP) {
    if (c->momentum != 0.0f) return fail("Momentum cannot be used with RMSProp. (momentum = %g)", (double)c->momentum);
    if (!(c->rms_decay >= 0.0f && c->rms_decay < 1.0f)) return fail("RMSProp: rms_decay must be in [0, 1) (got %g)", (double)c->rms_decay);
  }
  if (c->solver_type != DQNHIP_SOLVER_ADAM && c->dp_world > 1)
    return fail("the %s solver needs dp_world = 1 (got %d): its data-parallel forms do not exist in this version", solver, c->dp_world);
  // SGDSolver::GetLearningRate / Regularize (lr_schedule.hip.h has the refusals)
  char msg[256];
  if (lr_schedule_check(schedule_of(*c), c->weight_decay, c->regularization_type, msg, sizeof msg)) return fail("%s", msg);
  if ((c->lr_policy != DQNHIP_LR_FIXED || c->weight_decay != 0.0f) && c->dp_world > 1)
    return fail("lr_policy %s / weight_decay %g need dp_world = 1 (got %d): their data-parallel forms do not exist in this version",
                dqnhip_lr_policy_name(c->lr_policy), (double)c->weight_decay, c->dp_world);
  return 0;
}

// ---- shape predicates of the launch schedules (learner.hip branches on them, plan_of reports them) -----------------------------
// does layer i's backward (dgrad + wgrad) take the side-by-side pair launch (small minibatches / narrow layers)?
bool bwd_layer_is_pair(const NetLayout& l, int i, int rows) { return dqnhip::bwd_layer_is_pair(l.kp[i], l.dims[i + 1], rows); }     // (gemm_plan.hip.h)
// may the head's weight / bias gradients ride in the first tower layer's wgrad launch (gemm_wgrad_narrow_rider: the last
// launch of a net's backward, input_grad == false)?
bool head_wgrad_can_ride(const NetLayout& l, int rows) {
  const int NH = l.NH, H = l.dims[l.L];
  return H % kRiderCW == 0 && (size_t)(rows * NH + 256 * NH) * sizeof(float) <= (size_t)64 * 1024;
}
// does a weights-wanted, no-input-gradient backward of this tower take the SHIFTED schedule (see tower_backward)?
bool bwd_is_shifted(const H* h, const NetLayout& l, int rows) {
  bool shifted = l.L >= 2 && rows % 16 == 0 && !(h->cfg.tuning_flags & DQNHIP_TUNE_BWD_UNSHIFTED);
  for (int i = 1; i < l.L && shifted; ++i) shifted = !bwd_layer_is_pair(l, i, rows) && l.kp[i] % 64 == 0 && l.dims[i + 1] % 64 == 0;
  return shifted;
}
// rows >= 1024: the heads' backward takes the bandwidth-tiled kernel pair (head_backward_big)
bool head_big_ok(const H* h, int rows, int Hd) { return h->head_slab2 != nullptr && rows >= 1024 && rows % 64 == 0 && Hd % 256 == 0; }
// fp16 learner: does a weights-wanted backward of this net end in a hgemm_group_db launch (the carrier of the head's dW / db riders and of a
// data-parallel learner's tails block)?  Grouped form: always; per-layer form: when the first layer's wgrad takes the 64 x 64 tile.
bool bwd16_has_carrier(const H* h, int net, int rows) {
  const NetLayout& l = layout_of(h, net);
  if (l.L <= kHGemmMax && rows >= kGroupMinRows && !(h->cfg.tuning_flags & DQNHIP_TUNE_FP16_WGRAD_PER_LAYER)) return true;
  HGemm g{}; g.ta = 1; g.tb = 1; g.M = l.dims[1]; g.N = h->k16[net & 1][0]; g.K = rows;
  return hgemm_uses_small_tile(g) && g.K % 128 == 0 && g.M % 64 == 0 && g.N % 64 == 0;
}
// may the first layer of this net run as rider blocks of an optimiser launch (FirstLayerRider, NextL0)?  16-output tiles, and the
// layer's W and b lead the arena back to back: the workgroups that step them are the ones that then use them
bool l0_can_ride(const NetLayout& l) { return l.dims[1] % 16 == 0 && l.w_off[0] == 0 && l.b_off[0] == (size_t)l.dims[1] * l.kp[0]; }
// k_dqda_head_bwd's shapes: 16 columns from the first action column inside a critic panel row of `panel_w`, fewer than 1024 rows
bool dqda_head_shape_ok(const H* h, int panel_w) {
  return h->B % 16 == 0 && h->B < 1024 && h->S + 16 <= panel_w && h->L >= 1 && h->lc.dims[1] % 64 == 0;
}

// ---- the plan: which merged forms this learner's update takes ------------------------------------------------------------------
// ONE place decides (every predicate the launch sequence below branches on), run_phase / run_phase16 read it, and
// dqnhip_get_update_plan reports it together with the launch counts of a captured update: a predicate that silently stops matching at a
// BASELINE shape is a red test (tests/test_gpu_update_plan.py), not a slower bench.  A pure function of the learner's state (shapes,
// tuning flags, sharing, data-parallel mode): evaluated per call, never cached, so there is no stale copy to invalidate.
UpdatePlan plan_of(const H* h) {
  const NetLayout &la = h->la, &lc = h->lc;
  const int B = h->B, L = h->L, Hh = la.dims[L], Hc = lc.dims[L];
  const int tf = h->cfg.tuning_flags;
  UpdatePlan p{};
  p.fp16 = h->fp16;
  p.dp = dp_exchanges(h);     // (a one-rank group with bf16 exchange / a sharded optimiser runs the N-rank code path)
  p.fused_seed = !(tf & DQNHIP_TUNE_SEPARATE_HEAD_SEED);
  p.prioritized = h->per != nullptr;
  p.nstep = h->nstep != nullptr;
  p.smooth = h->tnoise != nullptr;
  if (h->fp16) {
    // fp16 learner: the head's dW / db are column-sum workgroups of the net's last backward launch (hgemm_group_db, HeadWsum)
    // when that launch exists; Step(1)'s k_head_q_train then also writes the scaled fp16 tower-top gradient — no head-backward launch
    // (below 1024 rows: beside the grouped wgrad's 200 one-per-CU tiles at 4096 rows the blocks cost more than the launches they replace)
    p.head_rides_c = bwd16_has_carrier(h, DQNHIP_CRITIC, B) && Hc % 64 == 0 && B < 1024;
    p.head_rides_a = bwd16_has_carrier(h, DQNHIP_ACTOR, B) && Hh % 64 == 0 && B < 1024;
    p.fuse_q = p.head_rides_c;
    p.tails_ride = p.dp && bwd16_has_carrier(h, DQNHIP_CRITIC, B) && bwd16_has_carrier(h, DQNHIP_ACTOR, B);
    // the critic's layer-0 dgrad (only its ten action columns are consumed), the inverting gradients and the actor heads' backward in
    // ONE launch (k_dqda_head_bwd<true>), as on the fp32 path; q(s, mu(s)) rides there
    p.fuse_head = p.head_rides_a && !(tf & DQNHIP_TUNE_SEPARATE_ACTOR_HEAD_BWD) && dqda_head_shape_ok(h, h->k16[1][0]);
    return p;
  }
  p.shifted_c = bwd_is_shifted(h, lc, B); p.shifted_a = bwd_is_shifted(h, la, B);
  p.tails_ride = p.dp && p.shifted_c && p.shifted_a;        // data parallel: the tails block rides in each net's last backward launch
  // the head's own dW / db ride in the net's last backward launch (the first layer's narrow wgrad)
  p.head_rides_c = !head_big_ok(h, B, Hc) && head_wgrad_can_ride(lc, B);
  p.head_rides_a = !head_big_ok(h, B, Hh) && head_wgrad_can_ride(la, B);
  // Step(1)'s head arithmetic inside the critic's top-layer dgrad launch (k_dgrad_qtrain; one 16-column piece per lane: H / 16 <= 64)
  // (prioritized replay: the DQNHIP_TUNE_SEPARATE_Q_TRAIN form, k_head_q_train_w in k_head_q_train's place)
  // (n-step returns: the same form, k_head_q_train_n there)
  p.fuse_q = !p.prioritized && !p.nstep && h->U3 != nullptr && !(tf & DQNHIP_TUNE_SEPARATE_Q_TRAIN) && p.head_rides_c && p.shifted_c && Hc >= 512 && Hc <= 1024 && Hc % 256 == 0;
  // dQ/da's last step, the inverting gradients and the actor heads' backward in ONE launch (k_dqda_head_bwd): 16 columns from the first
  // action column inside the panel row, fewer than 1024 rows, any tower-top width
  p.fuse_head = p.head_rides_a && !(tf & DQNHIP_TUNE_SEPARATE_ACTOR_HEAD_BWD) && dqda_head_shape_ok(h, lc.kp[0]);
  // the first layer of critic(s, mu(s)) rides in the critic's optimiser launch (FirstLayerRider).  Data-parallel learners too:
  // the launch sits behind the critic's exchange point, its norm then comes from k_sumsq's partials; only a SHARDED optimiser — whose
  // pass covers 1/N of the arena — keeps the launch of its own
  p.critic_l0 = !h->dp_shard && h->shared_fl[DQNHIP_CRITIC] == 0 && !(tf & DQNHIP_TUNE_SEPARATE_FIRST_LAYER) &&
                (lc.kp[0] == 64 || lc.kp[0] == 128) && l0_can_ride(lc) && B % 16 == 0 && B <= 512 && L >= 2;
  // Step(1)'s four first layers in one launch, critic_target's action half in the target actor's head kernel (first_layers_launch)
  // (target smoothing: a~ must stand in Xc_nx before the critic-target's first layer reads it — the schedule of
  // DQNHIP_TUNE_SEPARATE_CRITIC_FIRST_LAYERS: no action half inside the head kernel, and with it no early_l0)
  p.first_layers_merged = !p.smooth && h->Zs != nullptr && !(tf & DQNHIP_TUNE_SEPARATE_CRITIC_FIRST_LAYERS) && L >= 2 && B % 32 == 0 && B < 1024 && la.kp[0] < 512 &&
                          lc.kp[0] < 512 && la.dims[1] % 64 == 0 && lc.dims[1] % 64 == 0 && lc.dims[1] <= 1024 && round_up(h->S, 64) <= lc.kp[0];
  // inside a multi-update graph: the next update's gather rides in the critic's optimiser launch and its four first layers in the
  // actor's (k_adam_soft_fwd1_gather / k_adam_soft_l0).  Needs every piece those riders stand on.
  // (prioritized replay: an update's indices do not exist before its predecessor's write-back — no rider gathers ahead)
  // (n-step returns: the riders carry gather_block, not the window walk — v1 gathers in a launch of its own)
  p.early_l0 = !p.prioritized && !p.nstep && h->Xa_s2[1] != nullptr && !(tf & DQNHIP_TUNE_LATE_GATHER) && p.critic_l0 && p.first_layers_merged && h->shared_fl[DQNHIP_ACTOR] == 0 &&
               la.kp[0] == 64 && l0_can_ride(la);
  // the first-layer riders step their slice with Adam's expression (adam_apply4): the other solvers' optimiser launches carry none —
  // the schedule DQNHIP_TUNE_SEPARATE_FIRST_LAYER | DQNHIP_TUNE_LATE_GATHER give an Adam learner
  if (h->cfg.solver_type != DQNHIP_SOLVER_ADAM) { p.critic_l0 = false; p.early_l0 = false; }
  // ... and neither do k_sched_soft<>'s (an lr policy on another solver, a weight decay on any)
  if (sched_family(h)) { p.critic_l0 = false; p.early_l0 = false; }
  return p;
}
// ... while a multi-update graph is being captured (cap_u: the position of the update in it)
bool early_l0(const H* h) { return h->cap_u >= 0 && plan_of(h).early_l0; }

}  // namespace dqnhip_host

extern "C" {

const char* dqnhip_last_error(void) { return g_err.c_str(); }
// used by snapshot.cpp (same library, different translation unit) to report through the same channel
int dqnhip_internal_set_error(const char* msg) { g_err = msg ? msg : ""; return 1; }

// action noise: the literature's values in units of the column's range — not measured on this workload (include/dqnhip.h)
int dqnhip_noise_default_config(dqnhip_noise_config* cfg, int32_t purpose) {
  if (!cfg) return fail("null argument");
  if (purpose != DQNHIP_NOISE_EXPLORE && purpose != DQNHIP_NOISE_TARGET) return fail("dqnhip_noise_default_config: unknown purpose %d", (int)purpose);
  memset(cfg, 0, sizeof *cfg);
  cfg->struct_size = (int32_t)sizeof *cfg;
  cfg->clamp = 1;
  if (purpose == DQNHIP_NOISE_EXPLORE) { cfg->sigma_logits = 0.0f; cfg->sigma_params = 0.1f; cfg->theta = 0.15f; cfg->clip = 0.0f; cfg->seed = 0x6E6F697365ull; }
  else { cfg->sigma_logits = 0.1f; cfg->sigma_params = 0.1f; cfg->theta = 1.0f; cfg->clip = 0.25f; cfg->seed = 0x736D6F6F7468ull; }
  return 0;
}

int dqnhip_noise_explore_host(const dqnhip_noise_config* cfg, uint64_t counter, int32_t row, float* ou_state, float* actor_out) {
  if (!cfg || !ou_state || !actor_out) return fail("null argument");
  if (cfg->struct_size != (int32_t)sizeof(dqnhip_noise_config)) return fail("dqnhip_noise_config.struct_size mismatch");
  if (row < 0) return fail("dqnhip_noise_explore_host: row must be >= 0");
  NoiseCfg c{};
  c.sigma_logits = cfg->sigma_logits; c.sigma_params = cfg->sigma_params; c.theta = cfg->theta; c.clip = cfg->clip;
  c.clamp = cfg->clamp ? 1 : 0; c.seed = cfg->seed;
  char msg[256];
  if (noise_config_check(c, msg, sizeof msg)) return fail("dqnhip_noise_explore_host: %s", msg);
  for (int j = 0; j < kNO; ++j) {
    const float z = noise_normal(c.seed, counter, noise_lane0(row, j));
    ou_state[j] = noise_ou_step(ou_state[j], c.theta, noise_sigma(c, j), z);
    actor_out[j] = noise_apply(actor_out[j], j, ou_state[j], c.clamp);
  }
  return 0;
}

}  // extern "C"
