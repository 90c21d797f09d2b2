// learner.hip — what one update launches.
//
// Host-side orchestration of DQN::UpdateActorCritic (reference src/dqn.cpp:828-972)
// as a fixed sequence of gfx950 kernels on one HIP stream with no host sync:
// nothing crosses PCIe per update except (optionally) B sampled indices in and
// two floats out.  See DESIGN.md for the data layout and the kernel list.
// This translation unit: the forward / backward / optimiser building blocks and the three phases, fp32 (run_phase) and fp16
// (run_phase16), and dqnhip_apply_update*.  Which merged forms they take is decided in learner_plan.hip (plan_of); who calls them —
// capture, replay, the update entry points — is learner_update.hip.  The other units: learner_internal.hip.h.
#include "learner_internal.hip.h"
#include "gemm_direct.hip.h"
#include "hgemm.hip.h"
#include "head_fwd_kernels.hip.h"
#include "head_kernels.hip.h"
#include "small_kernels.hip.h"
#include "solver_kernels.hip.h"

using namespace dqnhip;
using namespace dqnhip_host;

namespace dqnhip_host {

const char* const kFamily[kNumFamily] = {"gemm_fwd_lds_4x2", "gemm_dgrad", "gemm_wgrad", "adam", "gemm_bwd_pair", "gemm_fwd_lds_2x2", "gemm_fwd_direct",
                                         "hgemm_fwd", "hgemm_dgrad", "hgemm_wgrad",
                                         "per_sync", "per_sample", "per_update"};      // by Family
// The timing family of a launch of an fp32 GEMM form (gemm_plan.hip.h) with n problems.  The forward LDS families go by the number
// of problems, not by the tile: a single problem — the 16x16 tile included — files under gemm_fwd_lds_2x2, a grouped launch of any
// tile under gemm_fwd_lds_4x2.
static Family family_of(GemmForm f, int n) {
  switch (kGemmForms[f].kind) {
    case GEMM_KIND_FWD_DIRECT: return kFamFwdDirect;
    case GEMM_KIND_FWD_LDS: return n == 1 ? kFamFwdLds2x2 : kFamFwdLds4x2;
    case GEMM_KIND_DGRAD: case GEMM_KIND_DGRAD_NARROW: return kFamDgrad;
    case GEMM_KIND_BWD: return kFamBwdPair;
    case GEMM_KIND_WGRAD_NARROW: case GEMM_KIND_TAIL: break;
  }
  return kFamWgrad;
}
// a rider launcher (head_kernels.hip.h) is keyed on the form it extends and takes that form's problems: the same precondition
static int form_check(GemmForm f, const GemmBatch& b) {
  return gemm_form_accepts(f, b) ? 0 : fail("internal: the carrier %s of a rider does not accept its problems", kGemmForms[f].name);
}
// one launch of form f (rider / tails: what a tail form carries), timed under its family
static int form_launch(H* h, hipStream_t st, GemmForm f, GemmBatch& b, const HeadWgradRider* rider = nullptr, const TailsArgs* tails = nullptr) {
  HIPCHK(gemm_form_launch(f, b, timed(h, family_of(f, b.n), st), rider, tails));
  return 0;
}

// ---- forward / backward building blocks ----------------------------------------

// One tower layer forward for up to kMaxGroup passes of identical shape.
int layer_forward(H* h, hipStream_t st, const FwdPass* passes, int n, int rows, int i) {
  const NetLayout& l = *passes[0].l;
  GemmBatch b{}; b.n = n;
  for (int j = 0; j < n; ++j) {
    GemmProblem& p = b.prob[j];
    p.P = wat(h, passes[j].net, l.w_off[i]); p.ldp = l.kp[i];
    p.Q = passes[j].act[i]; p.ldq = l.kp[i];
    p.C = passes[j].act[i + 1]; p.ldc = l.kp[i + 1];
    p.Pdim = l.dims[i + 1]; p.Qdim = rows; p.Kred = l.kp[i];
    p.bias = wat(h, passes[j].net, l.b_off[i]); p.relu = 1;
    if (i == l.L - 1 && passes[j].seed_w != nullptr) { p.seed_w = passes[j].seed_w; p.C2 = passes[j].seed_out; }
    if (i == l.L - 1 && passes[j].dot_w != nullptr) { p.dot_w = passes[j].dot_w; p.dot_out = passes[j].dot_out; }
  }
  return form_launch(h, st, fwd_form(l.kp[i], l.dims[i + 1], rows, n), b);
}
int tower_forward(H* h, hipStream_t st, const FwdPass* passes, int n, int rows, int first_layer) {
  for (int i = first_layer; i < passes[0].l->L; ++i) RC(layer_forward(h, st, passes, n, rows, i));
  return 0;
}

// Tower backward from dZ[L] (gradient wrt the last tower pre-activation) down, one launch per layer on `st`.
// want_w: produce dW/db (+sumsq partials) into garena; input_grad: also dZ[0].
// in_lo / in_hi: when only these input columns of dZ[0] are consumed (the critic's action columns), the
// first layer's dgrad computes just the 16-column tiles that cover them.
// fuse: the critic's dQ/da pass — the first layer's action-column tiles, the inverting gradients and the actor heads' backward in
// ONE launch (k_dqda_head_bwd) instead of the narrow dgrad launch here and a head-backward launch after it; carries the q rider.
// qtrain (Step(1)'s backward, shifted schedule): the top layer's dgrad launch also does k_head_q_train's work (k_dgrad_qtrain);
// qtrain_seed = the panel U = (-w_h) lrelu'(x_L) the online critic's top forward layer left (the dgrad's dY operand)
// rider (the head's dW / db) and tails (a data-parallel learner's [loss, q, flag] block) ride in the backward's last launch; qrider
// (q(s, mu(s))) in the first layer's input-gradient launch
struct BwdRiders {
  int in_lo = 0, in_hi = -1;
  const HeadWgradRider* rider = nullptr;
  const QHeadRider* qrider = nullptr;
  DqdaHeadArgs* fuse = nullptr;
  const HeadTrainArgs* qtrain = nullptr; const float* qtrain_seed = nullptr;
  const TailsArgs* tails = nullptr;
};
int tower_backward(H* h, hipStream_t st, const NetLayout& l, int net, float* garena, float* partial,
                   float** act, float** dZ, int rows, bool want_w, bool input_grad, const BwdRiders& r = BwdRiders{}) {
  const QHeadRider* qrider = r.qrider;     // (cleared by the launch that carries it)
  auto dgrad_of = [&](int i) {             // dZ[i] = (dZ[i+1] . W_i) * lrelu'(act[i])
    GemmProblem p{};
    p.mode = GEMM_DGRAD;
    p.P = wat(h, net, l.w_off[i]); p.ldp = l.kp[i];
    p.Q = dZ[i + 1]; p.ldq = l.kp[i + 1];
    p.C = dZ[i]; p.ldc = l.kp[i];
    p.Pdim = l.kp[i]; p.Qdim = rows; p.Kred = l.dims[i + 1];
    p.mask = i > 0 ? act[i] : nullptr; p.ldm = l.kp[i];
    return p;
  };
  auto wgrad_of = [&](int i) {             // dW_i = dZ[i+1]^T . act[i] ; db_i = colsum(dZ[i+1])
    GemmProblem p{};
    p.mode = GEMM_WGRAD;
    p.P = act[i]; p.ldp = l.kp[i];
    p.Q = dZ[i + 1]; p.ldq = l.kp[i + 1];
    p.C = garena + l.w_off[i]; p.ldc = l.kp[i];
    p.Pdim = l.kp[i]; p.Qdim = l.dims[i + 1]; p.Kred = rows;
    p.db = garena + l.b_off[i];
    p.partial = partial ? partial + l.part_off[i] : nullptr;
    return p;
  };
  auto layer_slice = [&](int i) { return (i + 1 < l.L ? l.w_off[i + 1] : l.hw_off) - l.w_off[i]; };
  // SHIFTED schedule (weights wanted, no input gradient, every layer above the first on the one-workgroup-type form):
  //   dgrad(L-1) | wgrad(L-1) + dgrad(L-2) | ... | wgrad(2) + dgrad(1) | wgrad(1) + wgrad(0) + the head's riders
  // instead of  wgrad(i) + dgrad(i) per layer and a last launch with the first layer's narrow wgrad alone.  Same launch
  // count, same workgroups, same arithmetic: the chain's last launch — 64-128 short workgroups, 6 us of launch floor —
  // is absorbed into a full wgrad launch (+~1 us), at the price of splitting one pair (8.3 + 7.9 instead of 14.5 us).
  const bool shifted = want_w && !input_grad && bwd_is_shifted(h, l, rows);
  if (r.qtrain != nullptr && !(shifted && dgrad_form(l.dims[l.L]) == GEMM_FORM_DGRAD_LDS)) return fail("internal: k_dgrad_qtrain needs the shifted schedule and an LDS-staged top layer");
  if (shifted) {
    {
      GemmBatch bd{}; bd.n = 1; bd.prob[0] = dgrad_of(l.L - 1);
      const GemmForm f = dgrad_form(l.dims[l.L]);
      if (r.qtrain != nullptr) {             // (f is GEMM_FORM_DGRAD_LDS: checked above)
        bd.prob[0].Q = r.qtrain_seed;
        RC(form_check(f, bd));
        HIPCHK(dgrad_qtrain_launch(bd, *r.qtrain, timed(h, family_of(f, 1), st)));
      } else RC(form_launch(h, st, f, bd));
    }
    for (int i = l.L - 2; i >= 1; --i) {
      GemmBatch b{}; b.n = 2; b.prob[0] = dgrad_of(i); b.prob[1] = wgrad_of(i + 1);
      RC(form_launch(h, st, bwd_shifted_mid_form(l.dims[i + 1]), b));
      if (h->comm && h->dp_per_layer) RC(dp_reduce_slice(h, st, net, l.w_off[i + 1], layer_slice(i + 1)));
    }
    {
      GemmBatch b{}; b.n = 2; b.prob[0] = wgrad_of(1); b.prob[1] = wgrad_of(0);
      RC(form_launch(h, st, bwd_shifted_tail_form(l.NH), b, r.rider, r.tails));
      if (h->comm && h->dp_per_layer) RC(dp_reduce_slice(h, st, net, l.w_off[0], layer_slice(0) + layer_slice(1)));
    }
    if (qrider) return fail("internal: the q-head rider found no carrier launch");
    return 0;
  }
  if (r.tails != nullptr) return fail("internal: the tails block rides in the shifted schedule's last launch only");
  for (int i = l.L - 1; i >= 0; --i) {
    GemmBatch bd{}, bw{};
    const bool need_dx = (i > 0 || input_grad);
    if (need_dx) bd.prob[bd.n++] = dgrad_of(i);
    if (want_w) bw.prob[bw.n++] = wgrad_of(i);
    if (need_dx && want_w) {
      GemmBatch b{}; b.n = 2; b.prob[0] = bd.prob[0]; b.prob[1] = bw.prob[0];
      RC(form_launch(h, st, bwd_form(l.kp[i], l.dims[i + 1], rows), b));
    } else if (need_dx && i == 0 && r.fuse != nullptr) {
      GemmProblem p = bd.prob[0];
      p.P += r.in_lo; p.C = nullptr; p.Pdim = 16; p.mask = nullptr;
      r.fuse->pr = p;
      const QHeadRider none{};
      HIPCHK(dqda_head_bwd_launch(*r.fuse, qrider ? *qrider : none, timed(h, kFamDgrad, st)));
      qrider = nullptr;
    } else if (need_dx && i == 0 && r.in_hi > r.in_lo && rows % 16 == 0) {
      GemmProblem& p = bd.prob[0];
      const int c0 = (r.in_lo / 16) * 16, c1 = std::min(l.kp[0], (r.in_hi + 15) / 16 * 16);
      p.P += c0; p.C += c0; p.Pdim = c1 - c0;
      if (p.mask) p.mask += c0;
      const GemmForm f = dgrad_form(l.dims[1], true);
      if (qrider) {
        RC(form_check(f, bd));
        HIPCHK(dgrad_narrow_qrider_launch(bd, *qrider, timed(h, family_of(f, 1), st)));
        qrider = nullptr;
      } else RC(form_launch(h, st, f, bd));
    } else if (need_dx) RC(form_launch(h, st, dgrad_form(l.dims[i + 1]), bd));
    else if (r.rider) {                                  // + the head's dW / db as rider blocks (head_wgrad_can_ride)
      const GemmForm f = wgrad_form();
      RC(form_check(f, bw));
      const LaunchOn on = timed(h, family_of(f, 1), st);
      if (l.NH == 1) HIPCHK((wgrad_narrow_rider_launch<1>(bw, *r.rider, on))); else HIPCHK((wgrad_narrow_rider_launch<kNO>(bw, *r.rider, on)));
    } else RC(form_launch(h, st, wgrad_form(), bw));
    // data parallel, bucketed: layer i's dW/db are final once this launch has run -> start their
    // all-reduce on the communication stream while the chain continues with layer i-1
    if (want_w && h->comm && h->dp_per_layer) RC(dp_reduce_slice(h, st, net, l.w_off[i], layer_slice(i)));
  }
  if (qrider) return fail("internal: the q-head rider found no carrier launch");
  return 0;
}

// rows >= 1024: the bandwidth-tiled kernel pair; optionally emits the scaled fp16 panels itself
template <int NH>
constexpr size_t head_bwd_big_lds_bytes() { return (size_t)(64 * NH + 4 * NH * 256) * sizeof(float); }
template <int NH>
int head_backward_big(H* h, hipStream_t st, HeadBwdArgs a, h16* dZ16, float scale16) {
  HeadBwdBigArgs b{}; b.a = a; b.dZ16 = dZ16; b.scale16 = scale16; b.slab2 = h->head_slab2;
  const int chunks = a.rows / 64;
  const int riders = a.q_out != nullptr ? chunks : 0;     // as many rider blocks again: 4 rows per block and round
  b.chunks = riders ? chunks : 0;
  HIPCHK(launch(st, k_head_bwd_big<NH>, dim3(chunks + riders, a.H / 256), dim3(256), head_bwd_big_lds_bytes<NH>(), b));
  if (a.dW != nullptr) HIPCHK(launch(st, k_head_wred<NH>, dim3(a.H / 64, NH), dim3(256), 0, b, chunks));
  return 0;
}

template <int NH>
int head_backward(H* h, hipStream_t st, HeadBwdArgs a) {
  if (head_big_ok(h, a.rows, a.H)) return head_backward_big<NH>(h, st, a, nullptr, 1.0f);
  // row chunks: enough blocks to cover the chip a few times over, <= 64 rows per chunk
  const int RC = std::max(1, std::min(16, a.rows / 64));   // (64 chunks measured slower at B=4096: the last arriver's slab walk)
  const int rows_c = (a.rows + RC - 1) / RC;
  size_t lds = ((size_t)rows_c * NH + 16 * NH * 64 + 16) * sizeof(float);
  a.slab = h->head_slab; a.ticket = h->head_ticket;
  int ry = 0;                                               // extra grid rows for the q rider (16 rows per block)
  if (a.q_out != nullptr) { a.rc_blocks = RC; ry = ((a.rows + 15) / 16 + a.H / 64 - 1) / (a.H / 64); }
  HIPCHK(launch(st, k_head_bwd<NH>, dim3(a.H / 64, RC + ry), dim3(1024), lds, a));
  return 0;
}

// The gather of one update (src/dqn.cpp:846-887).  pos: -1 outside multi-update graphs; else the update's position in the
// graph being captured (0: a launch of its own that also stores DevState::gbase; k >= 1: rides in update k-1's last launch)
GatherArgs gather_args(H* h, const int* idx_dev, int pos) {
  const NetLayout &la = h->la, &lc = h->lc;
  GatherArgs g{};
  g.ring = RO(h)->ring; g.rs = RO(h)->st; g.st = h->st; g.idx_in = idx_dev; g.seed = sample_key(h); g.B = h->B;
  if (h->fp16)
    // the gather writes the five minibatch panels in fp16 (what the GEMMs read: no conversion launch); the action columns
    // of the two critic panels the actor heads fill are zero here — the heads write mu / mu' straight into the panels
    g.o = GatherOut{nullptr, nullptr, la.kp[0], nullptr, nullptr, nullptr, lc.kp[0], h->mb_reward, h->mb_mc, h->mb_term, h->mb_idx,
                    h->act16[1][0], h->act16[0][0], h->act16[3][0], h->act16[4][0], h->act16[2][0]};
  else
    g.o = GatherOut{h->Xa_s2[pos > 0 && early_l0(h) ? (pos & 1) : 0], h->Xa_n, la.kp[0], h->Xc_tr, h->Xc_pl2[pos > 0 && early_l0(h) ? (pos & 1) : 0], h->Xc_nx, lc.kp[0],
                    h->mb_reward, h->mb_mc, h->mb_term, h->mb_idx};
  const int slot = pos > 0 ? (pos & 1) : 0;
  g.corr = h->st->adam_corr[slot]; g.soft_now = &h->st->soft_now[slot];
  g.beta1 = h->cfg.momentum; g.beta2 = h->cfg.momentum2; g.soft_update_freq = h->cfg.soft_update_freq;
  g.ahead = pos > 0 ? pos : -1; g.store_base = pos == 0 ? 1 : 0;
  if (h->chain_cap && pos > 0) { g.idx_in = h->idx_next_dev[pos & 1]; g.ahead = -2; }      // dqnhip_update_chained: the next update's indices, known one call ahead
  // dqnhip_update_indexed_n: every rider form (k_adam_soft_fwd1_gather, k_adam_soft_gather) reads slot `pos` of the graph's index bank;
  // the counters stay gbase + pos, as in a sampled graph
  if (h->cap_idx != nullptr && pos > 0) g.idx_in = h->cap_idx + (size_t)pos * h->B;
  g.blocks = (h->B + 3) / 4 + 1;
  g.sched = h->sched_dev;
  // k_sched_soft<> of a solver without a bias correction reads the slot too: 0 makes the correction exactly 1 (GatherArgs::sched)
  if (sched_family(h) && h->cfg.solver_type != DQNHIP_SOLVER_ADAM) { g.beta1 = 0.0f; g.beta2 = 0.0f; }
  return g;
}

// clip + Adam + Net::Update + soft target update over arena floats [begin, end)
// corr_pre: the update's first launch (k_gather) has left this step's bias correction in DevState::adam_corr
int adam_launch(H* h, hipStream_t st, int net, const float* partial, int n_partial, size_t begin, size_t end, const TickArgs* tick,
                bool corr_pre, const FirstLayerRider* fl, const GatherArgs* early_gather, const NextL0* next_l0) {
  AdamArgs a{};
  const int slot = h->cap_u > 0 ? (h->cap_u & 1) : 0;      // DevState::adam_corr
  a.corr_pre = corr_pre ? &h->st->adam_corr[slot][net] : nullptr; a.soft_pre = corr_pre ? &h->st->soft_now[slot] : nullptr;
  a.w = h->w[net] + begin; a.g = h->g[net] + begin; a.m = h->m[net] + begin; a.v = h->v[net] + begin;
  a.wt = h->w[net + 2] + begin;
  if (h->fp16) { a.w16 = h->w16a[net] + begin; a.wt16 = h->w16a[net + 2] + begin; }
  const size_t sh = h->shared_fl[net];                 // shared prefix of this net's arena (floats)
  if (sh > begin) {
    a.w_sh = h->w_owner->w[net] + begin; a.wt_sh = h->w_owner->w[net + 2] + begin;
    a.n4_sh = (std::min(sh, end) - begin) / 4;
  }
  a.n4 = (end - begin) / 4; a.partial = partial; a.n_partial = n_partial;
  a.lr = net == DQNHIP_ACTOR ? h->cfg.actor_lr : h->cfg.critic_lr;
  a.beta1 = h->cfg.momentum; a.beta2 = h->cfg.momentum2; a.eps = h->cfg.delta;
  a.clip = h->cfg.clip_gradients; a.tau = (float)h->cfg.tau;
  a.soft_update_freq = h->cfg.soft_update_freq; a.which = net; a.st = h->st;
  // dynamic loss scaling moves inside an update only (corr_pre): dqnhip_apply_update* keep the static behaviour — skip and report
  if (h->ls_dynamic && corr_pre) {
    a.ls_dynamic = 1;
    a.ls = LossScaleCfg{h->cfg.loss_scale_growth_interval, h->cfg.loss_scale_min_mult, h->cfg.loss_scale_max_mult};
  }
  if (tick) {
    if (!corr_pre) return fail("adam_launch: the update's bookkeeping needs the scalars k_gather leaves in DevState");
    a.tick_on = 1; a.tick = *tick;
  }
  // k_adam_soft_l0, k_adam_soft_fwd1_gather and k_adam_soft_gather below are launched while a multi-update or chain graph is being
  // captured (cap_u >= 0) and never otherwise; a learner with kernel timing on does not capture, so their LaunchOn carries no events
  if (h->timing && h->cap_u >= 0) return fail("internal: adam_launch inside a graph capture with kernel timing on");
  // A learner whose solver is not Adam reaches k_solver_soft<> / k_solver_soft_gather<> and nothing else (solver_kernels.hip.h): the
  // same arguments (beta2's slot carries rms_decay: solver_hyper), the same grid rule, the same timing family; no first-layer riders
  const int solver = h->cfg.solver_type;
  // A learner with an lr policy: the slot corr_pre points to holds the update's whole step scale (GatherArgs::sched), so the pass
  // multiplies it by 1 — an Adam learner without a decay stays on the tuned kernels below, riders included.  Everything else with a
  // policy or a decay runs k_sched_soft<> / k_sched_soft_gather<> (solver_kernels.hip.h), on the other solvers' schedule.
  if (has_policy(h) || sched_family(h)) {
    if (!corr_pre) return fail("adam_launch: a learner with lr_policy %s / weight_decay %g steps inside an update only (the pass reads the scalars its gather leaves in DevState)",
                               dqnhip_lr_policy_name(h->cfg.lr_policy), (double)h->cfg.weight_decay);
    if (has_policy(h)) a.lr = 1.0f;
  }
  if (sched_family(h)) {
    if (fl != nullptr || early_gather != nullptr || next_l0 != nullptr)
      return fail("internal: adam_launch: the optimiser launches of a learner with lr_policy %s / weight_decay %g carry no first-layer riders",
                  dqnhip_lr_policy_name(h->cfg.lr_policy), (double)h->cfg.weight_decay);
    if (solver != DQNHIP_SOLVER_ADAM) a.beta2 = h->cfg.rms_decay;
    const DecayArgs d{h->cfg.weight_decay, h->cfg.regularization_type == DQNHIP_REG_L1 ? 1 : 0};
    const LaunchOn on = timed(h, kFamAdam, st);
    const int blocks = (int)std::min<size_t>((a.n4 + 255) / 256, (size_t)1536);
    if (tick && h->cap_u >= 0 && h->cap_u + 1 < h->cap_n) {
      const GatherArgs g = gather_args(h, nullptr, h->cap_u + 1);
      const int ablocks = std::min(blocks, std::max(1536 - g.blocks, 1280));
      h->sched_launches[1] += 1;
      HIPCHK(sched_launch(solver, on, ablocks, a, d, &g));
    } else {
      h->sched_launches[0] += 1;
      HIPCHK(sched_launch(solver, on, blocks, a, d, nullptr));
    }
    return 0;
  }
  if (solver != DQNHIP_SOLVER_ADAM) {
    if (fl != nullptr || early_gather != nullptr || next_l0 != nullptr)
      return fail("internal: adam_launch: the %s solver's optimiser launches carry no first-layer riders", dqnhip_solver_name(solver));
    a.beta2 = h->cfg.rms_decay;
    const LaunchOn on = timed(h, kFamAdam, st);
    const int blocks = (int)std::min<size_t>((a.n4 + 255) / 256, (size_t)1536);
    if (tick && h->cap_u >= 0 && h->cap_u + 1 < h->cap_n) {      // (early_l0(h) is false on this learner: the gather rides here, as in k_adam_soft_gather)
      const GatherArgs g = gather_args(h, nullptr, h->cap_u + 1);
      const int ablocks = std::min(blocks, std::max(1536 - g.blocks, 1280));
      h->opt_launches[2] += 1;
      HIPCHK(solver_launch(solver, on, ablocks, a, &g));
    } else {
      h->opt_launches[1] += 1;
      HIPCHK(solver_launch(solver, on, blocks, a, nullptr));
    }
    return 0;
  }
  h->opt_launches[0] += 1;
  const LaunchOn on = timed(h, kFamAdam, st);
  // 1536 blocks = 6 per CU, all resident at once (68 VGPRs: 7 waves per SIMD): with the loads hoisted above the prologue
  // same-box A/B gives 18.4 us per launch against 19.3 at 2048 (a second, short round of blocks), 19.4 at 1792, 18.7 at
  // 1280, 21.5 at 4096 (round 2, before the hoist: 512 .. 8192 within +-3 %, profiles/r02_adam_probe.txt)
  if (fl != nullptr || next_l0 != nullptr) {
    if (begin != 0 || (fl && tick != nullptr) || a.w_sh != nullptr || h->fp16 || !corr_pre) return fail("adam_launch: a first-layer rider needs the whole, unshared fp32 arena inside an update");
    a.skip4 = layout_of(h, net).w_off[1] / 4;
  }
  const int blocks = (int)std::min<size_t>((a.n4 - a.skip4 + 255) / 256 + (fl ? fl->blocks : 0), (size_t)1536);   // riders + the strided pass: what is resident at once
  if (next_l0 != nullptr) {
    // the actor's launch inside a multi-update graph that gathered early: the next update's four first layers ride here (k_adam_soft_l0)
    if (tick == nullptr) return fail("adam_launch: the next update's first layers ride in the update's last launch");
    const int riders = next_l0->a.blocks + next_l0->c.blocks + next_l0->ct.blocks;
    const int ablocks = std::min(blocks, std::max(1536 - riders, 1280));
    HIPCHK(launch(on, k_adam_soft_l0, dim3(riders + ablocks), dim3(256), 0, a, next_l0->a, next_l0->c, next_l0->ct));
  }
  else if (fl != nullptr && early_gather != nullptr) {
    if (blocks <= fl->blocks) return fail("adam_launch: no optimiser workgroups beside the first-layer riders");
    const int ablocks = std::min(blocks, std::max(1536 - early_gather->blocks, 1280));
    if (fl->Kp == 64) HIPCHK(launch(on, k_adam_soft_fwd1_gather<1>, dim3(early_gather->blocks + ablocks), dim3(256), 0, a, *fl, *early_gather));
    else HIPCHK(launch(on, k_adam_soft_fwd1_gather<2>, dim3(early_gather->blocks + ablocks), dim3(256), 0, a, *fl, *early_gather));
  }
  else if (fl != nullptr) {
    if (blocks <= fl->blocks) return fail("adam_launch: no optimiser workgroups beside the first-layer riders");
    if (fl->Kp == 64) HIPCHK(launch(on, k_adam_soft_fwd1<1>, dim3(blocks), dim3(256), 0, a, *fl));
    else HIPCHK(launch(on, k_adam_soft_fwd1<2>, dim3(blocks), dim3(256), 0, a, *fl));
  }
  else if (tick && h->cap_u >= 0 && h->cap_u + 1 < h->cap_n && !early_l0(h)) {
    // inside a multi-update graph: the next update's gather rides in this, the update's last launch (k_adam_soft_gather).
    // At small minibatches the grid stays at what is resident at once; a large minibatch's gather (1025 workgroups at 4096
    // rows) must not thin the optimiser's own grid — its blocks drain within a few us and the rest of the grid moves in
    // (511 optimiser blocks beside it: 35.4 against 27.3 us per launch at 4096 rows)
    const GatherArgs g = gather_args(h, nullptr, h->cap_u + 1);
    const int ablocks = std::min(blocks, std::max(1536 - g.blocks, 1280));
    HIPCHK(launch(on, k_adam_soft_gather, dim3(g.blocks + ablocks), dim3(256), 0, a, g));
  }
  else HIPCHK(launch(on, k_adam_soft, dim3(blocks), dim3(256), 0, a));
  return 0;
}

// clip norm of the REDUCED gradient (data parallel); under DQNHIP_DP_HALF_GRADS the same pass widens the bf16
// transfer image back into the fp32 arena
int sumsq_launch(H* h, int net, size_t begin, size_t end) {
  const NetLayout& l = layout_of(h, net);
  if (end == 0) end = l.arena;
  if (h->dp_half) HIPCHK(launch(h->stream, k_sumsq_bf16, dim3(h->n_part_dp), dim3(256), 0, (const uint16_t*)h->g16[net] + begin, h->g[net] + begin, (end - begin) / 4, h->part_dp));
  else HIPCHK(launch(h->stream, k_sumsq, dim3(h->n_part_dp), dim3(256), 0, h->g[net] + begin, (end - begin) / 4, h->part_dp));
  return 0;
}
// a net's [loss, q, flag, sum of squares] tail: behind its gradient arena (one all-reduce carries both), or in dp_tails
static float* grad_tail(const H* h, int net) {
  if (h->dp_half || h->dp_shard) return h->dp_tails + (net == DQNHIP_ACTOR ? 4 : 0);
  return h->g[net] + layout_of(h, net).arena;
}
// the optimiser step of one net inside an update (phase 1: critic, phase 2: actor + bookkeeping); fl / early_gather / next_l0: the
// riders of adam_launch.  Single learner: the clip norm comes from the partial sums the backward's workgroups left behind.  dp: the
// gradient was reduced since, the norm is taken from the arena (k_sumsq) — or, sharded, the exchange left it in the net's tail
static int optimiser_step(H* h, hipStream_t st, int net, bool dp, const TickArgs* tick, const FirstLayerRider* fl = nullptr,
                          const GatherArgs* early_gather = nullptr, const NextL0* next_l0 = nullptr) {
  const NetLayout& l = layout_of(h, net);
  if (!dp) return adam_launch(h, st, net, h->part[net], l.n_part, 0, l.arena, tick, true, fl, early_gather, next_l0);
  if (h->dp_shard) {
    if (fl || early_gather || next_l0) return fail("internal: riders in a sharded optimiser launch");   // (its pass covers 1/N of the arena)
    // the exchange left this rank's slice of the reduced gradient in place and the group's sum of squares in tail[3]
    size_t lo, hi; shard_range(h, net, lo, hi);
    RC(adam_launch(h, st, net, grad_tail(h, net) + 3, 1, lo, hi, tick));
    return dp_allgather_weights(h, net);
  }
  RC(sumsq_launch(h, net));
  return adam_launch(h, st, net, h->part_dp, h->n_part_dp, 0, l.arena, tick, true, fl, early_gather, next_l0);
}

// ---- mixed-precision building blocks (hgemm.hip.h) --------------------------------------------

int hgemm_timed(H* h, hipStream_t st, const HGemm* gs, int n, Family fam, int force = 0, const HGemmLs* ls = nullptr) {
  HIPCHK(hgemm_launch_batch(gs, n, timed(h, fam, st), force, ls));
  return 0;
}
int hgemm_timed(H* h, hipStream_t st, const HGemm& g, Family fam, const HGemmLs* ls = nullptr) { return hgemm_timed(h, st, &g, 1, fam, 0, ls); }

// fp32 master weights of `net` -> fp16 mirror [N][kp].  The Adam pass keeps the mirrors current by itself; this
// runs after host-side weight changes (w16_dirty).
int sync_w16(H* h, hipStream_t st, int net) {
  const NetLayout& l = layout_of(h, net);
  const int kind = net & 1;
  Cvt16Batch b{};
  for (int i = 0; i < l.L; ++i) {
    cvt16_add(b, h->w[net] + l.w_off[i], l.kp[i], l.dims[i + 1], l.kp[i], h->w16[net][i], h->k16[kind][i], 1.0f);
    if (b.n == 8) { HIPCHK(cvt16_launch(b, st)); b = Cvt16Batch{}; }
  }
  // ... and what lies between the matrices (the biases; behind the last tower layer's, the heads): no GEMM reads those from the mirror,
  // but the optimiser pass writes the WHOLE arena's mirror, the target's only when the soft update is on — without this a target's mirror
  // kept whatever it held there before a host-side change until the next soft update (debug buffer w16_<net>: the mirror is the
  // master's image everywhere)
  for (int i = 0; i < l.L; ++i) {
    const size_t lo = l.b_off[i], hi = i + 1 < l.L ? l.w_off[i + 1] : l.arena;      // (whole 64-float lines: layout_init)
    cvt16_add(b, h->w[net] + lo, (int)(hi - lo), 1, (int)(hi - lo), h->w16a[net] + lo, (int)(hi - lo), 1.0f);
    if (b.n == 8) { HIPCHK(cvt16_launch(b, st)); b = Cvt16Batch{}; }
  }
  HIPCHK(cvt16_launch(b, st));
  h->w16_dirty[net] = false;
  return 0;
}

// layer i of `net` forward on the fp16 panels `panels` ([rows][k16[kind][.]]): the update's act16[p], or acting panels
HGemm fwd16_problem(H* h, h16* const* panels, int net, int rows, int i) {
  const NetLayout& l = layout_of(h, net);
  const int kind = net & 1;
  HGemm g{};
  g.A = panels[i]; g.lda = h->k16[kind][i];
  g.B = h->w16[net][i]; g.ldb = h->k16[kind][i];
  g.M = rows; g.N = l.dims[i + 1]; g.K = h->k16[kind][i];
  g.C16 = panels[i + 1]; g.ldc16 = l.dims[i + 1];
  // (no fp32 copy of the tower top: the head kernels read the fp16 panel, as every tower layer reads its input)
  g.bias = h->w[net] + l.b_off[i]; g.relu = 1; g.scale32 = 1.0f;
  return g;
}
HGemm fwd16_problem(H* h, int p, int net, int rows, int i) { return fwd16_problem(h, h->act16[p], net, rows, i); }
int tower_forward16_on(H* h, hipStream_t st, int net, h16* const* panels, int rows) {
  if (!h->fp16) return fail("internal: fp16 tower forward on an fp32 learner");
  if (rows < 64 || rows % 64) return fail("internal: fp16 tower forward needs whole 64-row tiles (got %d rows)", rows);
  if (h->w16_dirty[net]) RC(sync_w16(h, st, net));
  const NetLayout& l = layout_of(h, net);
  for (int i = 0; i < l.L; ++i) RC(hgemm_timed(h, st, fwd16_problem(h, panels, net, rows, i), kFamHgemmFwd));
  return 0;
}
int tower_forward16(H* h, hipStream_t st, int p, int net, int rows) {
  const NetLayout& l = layout_of(h, net);
  for (int i = 0; i < l.L; ++i) RC(hgemm_timed(h, st, fwd16_problem(h, p, net, rows, i), kFamHgemmFwd));
  return 0;
}
// two independent passes of the same net kind, layer by layer in ONE launch each (the target and
// the online net: same shapes, different weights and inputs)
int tower_forward16_pair(H* h, hipStream_t st, int p0, int net0, int p1, int net1, int rows) {
  const NetLayout& l = layout_of(h, net0);
  for (int i = 0; i < l.L; ++i) {
    const HGemm gs[2] = {fwd16_problem(h, p0, net0, rows, i), fwd16_problem(h, p1, net1, rows, i)};
    RC(hgemm_timed(h, st, gs, 2, kFamHgemmFwd));
  }
  return 0;
}

// Tower backward in fp16 from dZ16[kind][L] (already scaled by `ls`; dynamic loss scaling: by ls x the live multiplier, and ls_mult
// points at the net's {mult, 1 / mult} pair in DevState — null: static).  want_w: dW (fp32, unscaled)
// into garena + bias gradients; input_grad: fp32 dZ32_0[rows][kp0] (unscaled).
// No transposed copy of any panel exists: the dgrad reads the weight mirror W[n][k_in] reduction-major (its rows ARE
// the reduction index), the wgrad reads dY[b][n_out] and X[b][k_in] reduction-major (hgemm.hip.h, HGemm::ta / tb).
// Schedule: the dgrad chain first (one launch per layer), then ALL wgrads of the net + the bias-gradient column
// sums in ONE launch (hgemm_group_db) — at that point every dZ panel is complete and the wgrads are independent.
// cfg.tuning_flags & DQNHIP_TUNE_FP16_WGRAD_PER_LAYER restores the per-layer form (a layer's dgrad + wgrad sharing a
// launch when both take the 64x64 tile; the bias sums riding in the first layer's wgrad launch).
// partial: the clip norm's per-launch partial sums (single learner); rider (the head's dW / db) and tails ride in the last launch
struct Bwd16Riders { float* partial = nullptr; const HeadWsum* rider = nullptr; const TailsArgs* tails = nullptr; };
int tower_backward16(H* h, hipStream_t st, int net, int p, float* garena, float* dZ32_0, int rows,
                     bool want_w, bool input_grad, float ls, const float* ls_mult, const Bwd16Riders& r = Bwd16Riders{}) {
  const NetLayout& l = layout_of(h, net);
  const int kind = net & 1;
  h16** dZ = h->dZ16[kind];
  // dynamic loss scaling: every 1 / ls below times 1 / mult, in the kernel — the launches then take the *_ls kernels (HGemmLs)
  const HGemmLs lsv{nullptr, ls_mult != nullptr ? ls_mult + 1 : nullptr};
  const HGemmLs* lsp = ls_mult != nullptr ? &lsv : nullptr;
  const bool grouped = want_w && l.L <= kHGemmMax && rows >= kGroupMinRows && !(h->cfg.tuning_flags & DQNHIP_TUNE_FP16_WGRAD_PER_LAYER);
  HGemm gws[kMaxL];
  for (int i = l.L - 1; i >= 0; --i) {
    HGemm gd{};
    HGemm& gw = gws[i]; gw = HGemm{};
    const bool need_dx = i > 0 || input_grad;
    if (need_dx) {                         // dZ[i] = (dZ[i+1] . W_i) * lrelu'(act[i])
      HGemm& g = gd;
      g.A = dZ[i + 1]; g.lda = l.dims[i + 1];
      g.B = h->w16[net][i]; g.ldb = h->k16[kind][i]; g.tb = 1;
      g.M = rows; g.N = h->k16[kind][i]; g.K = l.dims[i + 1];
      if (i > 0) {
        // (the ReLU' operand is the whole fp16 activation panel although only its sign is used: a packed sign-bit form was
        // built and measured in round 4 — dgrad traffic 40 -> 33 MB per launch, duration unchanged, the forward's byte
        // stores +1 us per launch: profiles/r04_fp16_sign_mask.txt)
        g.mask = h->act16[p][i]; g.ldm = h->k16[kind][i];
        g.C16 = dZ[i]; g.ldc16 = h->k16[kind][i];
      } else {
        g.C32 = dZ32_0; g.ldc32 = l.kp[0]; g.n_valid32 = l.kp[0]; g.scale32 = 1.0f / ls;
      }
    }
    if (want_w) {                          // dW_i = dZ[i+1]^T . act[i]: both operands batch-major, dY[b][n_out], X[b][k_in]
      HGemm& g = gw;
      g.A = dZ[i + 1]; g.lda = l.dims[i + 1]; g.ta = 1;
      g.B = h->act16[p][i]; g.ldb = h->k16[kind][i]; g.tb = 1;
      g.M = l.dims[i + 1]; g.N = h->k16[kind][i]; g.K = rows;
      g.C32 = garena + l.w_off[i]; g.ldc32 = l.kp[i]; g.n_valid32 = l.kp[i]; g.scale32 = 1.0f / ls;
      if (r.partial) g.sumsq_partial = r.partial + l.part_off[i];      // clip-norm share of this layer's dW (unscaled)
    }
    if (grouped) { if (need_dx) RC(hgemm_timed(h, st, gd, kFamHgemmDgrad, lsp)); continue; }
    // per-layer form: both read dZ[i+1] and neither reads the other's output — at small minibatches (both on the
    // 64x64 split-K tile) they share one launch
    if (need_dx && want_w && hgemm_uses_small_tile(gd) && hgemm_uses_small_tile(gw) && gd.K % 128 == 0 && gw.K % 128 == 0) {
      const HGemm gs[2] = {gd, gw};
      RC(hgemm_timed(h, st, gs, 2, kFamHgemmDgrad, 2, lsp));      // both on the 64x64 tile, as each would be alone
    } else {
      if (need_dx) RC(hgemm_timed(h, st, gd, kFamHgemmDgrad, lsp));
      if (want_w && (i > 0 || need_dx)) RC(hgemm_timed(h, st, gw, kFamHgemmWgrad, lsp));
    }
  }
  if (!want_w) return 0;
  // db_i = column sums of dZ[i+1] [rows][n_out], one workgroup per 64 columns
  Db16Batch db{}; db.scale = 1.0f / ls; db.sumsq_partial = r.partial ? r.partial + l.part_db : nullptr;
  int db_blocks = 0;
  for (int i = 0; i < l.L; ++i) { db.d[db.n++] = Db16{dZ[i + 1], l.dims[i + 1], l.dims[i + 1], rows, garena + l.b_off[i], db_blocks}; db_blocks += l.dims[i + 1] / 64; }
  const LaunchOn on = timed(h, kFamHgemmWgrad, st);
  if (grouped) {
    // 128x128 tiles: a quarter of the operand bytes per FLOP of the 64x64 split-K tile (fp16 mode guarantees
    // hidden % 128 == 0, minibatch % 128 == 0 and a 128-wide first panel, so every wgrad tiles)
    HIPCHK(hgemm_group_db_launch(gws, l.L, true, db, db_blocks, on, r.rider, r.tails, lsp));
  } else if (!input_grad && hgemm_uses_small_tile(gws[0]) && gws[0].K % 128 == 0) {
    // per-layer form: the first layer's wgrad (few tiles, long reduction) carries the column sums
    HIPCHK(hgemm_group_db_launch(gws, 1, false, db, db_blocks, on, r.rider, r.tails, lsp));
  } else {
    if (r.rider != nullptr || r.tails != nullptr) return fail("internal: the fp16 backward found no carrier launch for its riders");
    if (!input_grad) HIPCHK(hgemm_launch(gws[0], on, 0, lsp));
    if (lsp != nullptr) HIPCHK(launch(st, k_db16_cols_ls<0>, dim3(db_blocks), dim3(256), 0, db, lsv.scale32_mult));
    else HIPCHK(launch(st, k_db16_cols<0>, dim3(db_blocks), dim3(256), 0, db));
  }
  return 0;
}

// ---- what both schedules hand their kernels -----------------------------------------------------------------------------------
// The precision-independent fields of the argument structs run_phase (fp32) and run_phase16 (fp16) both build; each adds the
// panels of its own precision after the builder returns.
static float inv_batch_of(const H* h) { return 1.0f / (float)(h->B * h->cfg.dp_world); }
// the head of the actor (mu(s)) or the target actor (mu'(s')); ldxc / xc_col: where it drops its output into a critic input panel
static HeadArgs actor_head_args(const H* h, int net) {
  const NetLayout& la = h->la;
  HeadArgs a{}; a.ldx = la.dims[h->L]; a.H = la.dims[h->L]; a.rows = h->B;
  a.W = wat(h, net, la.hw_off); a.b = wat(h, net, la.hb_off);
  a.out16 = net == DQNHIP_ACTOR ? h->aout16 : h->aout_t16; a.ldxc = h->lc.kp[0]; a.xc_col = h->S;
  return a;
}
// Step(1)'s head arithmetic: q', q, TD target, loss, dq
static HeadTrainArgs q_train_args(const H* h) {
  const NetLayout& lc = h->lc;
  HeadTrainArgs t{};
  t.Wt = wat(h, DQNHIP_CRITIC_TARGET, lc.hw_off); t.bt = wat(h, DQNHIP_CRITIC_TARGET, lc.hb_off);
  t.W = wat(h, DQNHIP_CRITIC, lc.hw_off); t.b = wat(h, DQNHIP_CRITIC, lc.hb_off);
  t.H = lc.dims[h->L]; t.rows = h->B; t.reward = h->mb_reward; t.mc = h->mb_mc; t.term = h->mb_term;
  t.q_target = h->q_t; t.q = h->q1; t.y = h->y; t.dq = h->dq; t.loss_partial = h->loss_partial;
  t.gamma = h->cfg.gamma; t.beta = h->cfg.beta; t.inv_batch = inv_batch_of(h); t.st = h->st;
  return t;
}
// prioritized replay: k_head_q_train's arguments + the sampling probabilities in, the weights and |TD errors| out
static HeadTrainWArgs q_train_w_args(const H* h, const HeadTrainArgs& t) {
  const PerHost* p = h->per;
  return HeadTrainWArgs{t, p->prob, p->w, p->td_abs, p->cfg.beta0, p->cfg.beta_anneal_iters};
}
// data parallel: the [loss, q, flag] tails for the exchange — one more block of a net's last backward launch (UpdatePlan::tails_ride)
// or a launch of its own (tails_launch)
static TailsArgs critic_tails(const H* h) {
  return TailsArgs{(const float*)h->loss_partial, h->n_head_blocks, (const double*)nullptr, 0, inv_batch_of(h), grad_tail(h, DQNHIP_CRITIC), (float*)nullptr, &h->st->flags, 0};
}
static TailsArgs actor_tails(const H* h) {
  return TailsArgs{(const float*)nullptr, 0, (const double*)h->q_partial, h->B, inv_batch_of(h), (float*)nullptr, grad_tail(h, DQNHIP_ACTOR), &h->st->flags, 0};
}
static int tails_launch(hipStream_t st, const TailsArgs& t) {
  HIPCHK(launch(st, k_tails, dim3(1), dim3(256), 0, t));
  return 0;
}
// the bookkeeping block of the update's last launch: publishes (critic_loss, avg_q), advances the iteration / sampling counters
static TickArgs tick_args(const H* h, bool dp) {
  return TickArgs{h->st, grad_tail(h, DQNHIP_CRITIC), grad_tail(h, DQNHIP_ACTOR), (const float*)h->loss_partial, h->n_head_blocks,
                  dp ? (const double*)nullptr : (const double*)h->q_partial, h->B, (float)(h->B * h->cfg.dp_world),
                  // (dqnhip_update_indexed_n: the update's own slot of the graph's stats bank)
                  h->cap_stats ? h->cap_stats + 4 * std::max(h->cap_u, 0) : h->stats_dev};
}
// 1-2: sample + gather (src/dqn.cpp:846-887).  Later updates of a multi-update graph: it rode in the previous update's last launch
// (n-step returns: k_gather_n, the same arguments + the window — always a launch of its own, plan_of: no multi-update riders)
static int gather_launch(H* h, hipStream_t st, const int* idx_dev) {
  if (h->nstep && h->cap_u >= 0) return fail("internal: an n-step update inside a multi-update schedule");
  if (h->cap_u > 0) return 0;
  const GatherArgs g = gather_args(h, idx_dev, h->cap_u);
  if (h->nstep) {
    const GatherNArgs a{g, h->nstep->n, (double)h->cfg.gamma, h->nstep->disc, h->nstep->steps};
    HIPCHK(launch(st, k_gather_n, dim3(g.blocks), dim3(256), 0, a));
    return 0;
  }
  HIPCHK(launch(st, k_gather, dim3(g.blocks), dim3(256), 0, g));
  return 0;
}
// Step(1)'s head arithmetic in a launch of its own: k_head_q_train, its weighted form (prioritized replay), or the per-row-discount
// form of either (n-step returns)
static int q_train_launch(H* h, hipStream_t st, const UpdatePlan& P, const HeadTrainArgs& t) {
  const dim3 grid((h->B + 3) / 4);
  if (P.nstep) {
    const HeadTrainNArgs an{P.prioritized ? q_train_w_args(h, t) : HeadTrainWArgs{t}, h->nstep->disc};
    if (P.prioritized) HIPCHK(launch(st, k_head_q_train_n<true>, grid, dim3(256), 0, an));
    else HIPCHK(launch(st, k_head_q_train_n<false>, grid, dim3(256), 0, an));
  }
  else if (P.prioritized) HIPCHK(launch(st, k_head_q_train_w, grid, dim3(256), 0, q_train_w_args(h, t)));
  else HIPCHK(launch(st, k_head_q_train, grid, dim3(256), 0, t));
  return 0;
}

int run_phase16(H* h, int phase, const int* idx_dev) {
  const int B = h->B, L = h->L;
  const NetLayout &la = h->la, &lc = h->lc;
  const UpdatePlan P = plan_of(h);
  const bool dp = P.dp;
  const int Hh = la.dims[L], Hc = lc.dims[L];
  hipStream_t st = h->stream;
  const bool split = phase == 10;
  // dynamic loss scaling: the {mult, 1 / mult} pairs the kernels read (null: static mode, the immediates alone)
  const float* lsm_c = h->ls_dynamic ? h->st->ls_mult[DQNHIP_CRITIC] : nullptr;
  const float* lsm_a = h->ls_dynamic ? h->st->ls_mult[DQNHIP_ACTOR] : nullptr;
  const bool part16 = !dp;      // the backward leaves the clip norm's partial sums (single learner: optimiser_step)
  // (the heads read the fp16 tower tops and write mu / mu' straight into the critics' fp16 input panels; the fp32 panels are unused)
  HeadArgs hA = actor_head_args(h, DQNHIP_ACTOR); hA.X16 = h->act16[1][L]; hA.xc16 = h->act16[4][0]; hA.ldxc16 = h->k16[1][0];
  if (phase == 11) {
    RC(tower_forward16(h, st, 1, DQNHIP_ACTOR, B));
    RC((head_forward<kNO, HEAD_ACTOR>(h, st, hA)));
    return 0;
  }
  if (phase == 0 || phase == 10) {
    RC(gather_launch(h, st, idx_dev));
    if (split) RC(tower_forward16(h, st, 0, DQNHIP_ACTOR_TARGET, B));
    else RC(tower_forward16_pair(h, st, 0, DQNHIP_ACTOR_TARGET, 1, DQNHIP_ACTOR, B));
    HeadArgs hAT = actor_head_args(h, DQNHIP_ACTOR_TARGET); hAT.X16 = h->act16[0][L]; hAT.xc16 = h->act16[2][0]; hAT.ldxc16 = h->k16[1][0];
    if (split) RC((head_forward<kNO, HEAD_ACTOR>(h, st, hAT)));
    else RC((head_forward<kNO, HEAD_ACTOR>(h, st, hAT, &hA)));
    RC(tower_forward16_pair(h, st, 2, DQNHIP_CRITIC_TARGET, 3, DQNHIP_CRITIC, B));
    {
      HeadTrainArgs t = q_train_args(h);
      t.Xt16 = h->act16[2][L]; t.X16 = h->act16[3][L];
      // with the head's dW / db riding in the net's last backward launch, the scaled fp16 tower-top gradient comes out of
      // this launch too (HeadTrainArgs::dZ16) — Step(1) has no head-backward launch (as on the fp32 path)
      if (P.fuse_q) { t.dZ16 = h->dZ16[1][L]; t.scale16 = h->ls_c; t.ls_mult = lsm_c; }
      RC(q_train_launch(h, st, P, t));
    }
    const TailsArgs tails_c = critic_tails(h);
    {
      HeadBwdArgs a{}; a.dyh = h->dq; a.lddy = 1; a.W = wat(h, DQNHIP_CRITIC, lc.hw_off); a.X416 = h->act16[3][L];
      a.H = Hc; a.rows = B; a.dZ = nullptr; a.dW = h->g[1] + lc.hw_off; a.db = h->g[1] + lc.hb_off;
      a.partial = h->part[1] + lc.part_off[L]; a.ls_mult = lsm_c;
      const HeadWsum r{h->dq, 1, h->act16[3][L], Hc, B, a.dW, a.db, a.partial, 1, Hc / 64};
      if (P.head_rides_c) {}                                       // (dZ16 came out of k_head_q_train, dW / db come from the riders)
      else if (head_big_ok(h, B, Hc)) { a.dZ = nullptr; RC(head_backward_big<1>(h, st, a, h->dZ16[1][L], h->ls_c)); }
      else { a.dZ16 = h->dZ16[1][L]; a.scale16 = h->ls_c; RC(head_backward<1>(h, st, a)); }
      Bwd16Riders br; br.partial = part16 ? h->part[1] : nullptr;
      if (P.head_rides_c) br.rider = &r;
      if (P.tails_ride) br.tails = &tails_c;
      RC(tower_backward16(h, st, DQNHIP_CRITIC, 3, h->g[1], nullptr, B, true, false, h->ls_c, lsm_c, br));
    }
    if (dp && !P.tails_ride) RC(tails_launch(st, tails_c));
    return 0;
  }
  if (phase == 1) {
    // the Adam pass writes the fp16 mirrors of the critic and its target itself
    RC(optimiser_step(h, st, DQNHIP_CRITIC, dp, nullptr));
    // As on the fp32 path: the seed of the dq = -1 pass comes out of the top layer's forward epilogue (HGemm::seed_w, the
    // scaled fp16 panel the dgrad chain reads) and q(s, mu(s)) rides in a later launch-floor launch — here the actor heads'
    // backward (HeadBwdArgs::qr_*).  DQNHIP_TUNE_SEPARATE_HEAD_SEED: the head-backward launch of their own.
    const bool fused_seed = P.fused_seed;
    for (int i = 0; i < L; ++i) {
      HGemm g = fwd16_problem(h, 4, DQNHIP_CRITIC, B, i);
      if (fused_seed && i == L - 1) { g.seed_w = wat(h, DQNHIP_CRITIC, lc.hw_off); g.CS16 = h->dZ16[1][L]; g.ldcs16 = Hc; g.seed_scale = h->ls_q; }
      const HGemmLs seed_ls{lsm_a, nullptr};      // (dynamic loss scaling: the seed panel carries ls_q x the actor's live multiplier)
      RC(hgemm_timed(h, st, g, kFamHgemmFwd, fused_seed && i == L - 1 && lsm_a != nullptr ? &seed_ls : nullptr));
    }
    if (!fused_seed) {
      // q(s, mu(s)) rides in the dq = -1 head launch (rider blocks)
      HeadBwdArgs a{}; a.dyh = nullptr; a.lddy = 1; a.W = wat(h, DQNHIP_CRITIC, lc.hw_off); a.X416 = h->act16[4][L];
      a.H = Hc; a.rows = B; a.dZ = nullptr; a.ls_mult = lsm_a;
      a.q_bias = wat(h, DQNHIP_CRITIC, lc.hb_off); a.q_out = h->q2; a.qsum_partial = h->q_partial;
      if (head_big_ok(h, B, Hc)) { a.dZ = nullptr; RC(head_backward_big<1>(h, st, a, h->dZ16[1][L], h->ls_q)); }
      else { a.dZ16 = h->dZ16[1][L]; a.scale16 = h->ls_q; RC(head_backward<1>(h, st, a)); }
    }
    // DQNHIP_TUNE_SEPARATE_ACTOR_HEAD_BWD where the fused form would apply: the same tile in a launch of its own (k_dqda_head_bwd<true> with
    // DqdaHeadArgs::dxc: dQ/da into the action columns of dZc[0], no head part) + k_head_bwd<10> below — the fused form's arithmetic, cut in
    // two, as on the fp32 path.  Other shapes: the fp16-MFMA layer-0 dgrad launch of tower_backward16
    const bool tile_alone = !P.fuse_head && P.head_rides_a && dqda_head_shape_ok(h, h->k16[1][0]);
    RC(tower_backward16(h, st, DQNHIP_CRITIC, 4, nullptr, h->dZc[0], B, false, !P.fuse_head && !tile_alone, h->ls_q, lsm_a));       // (else: layers L-1 .. 1 only)
    if (P.fuse_head || tile_alone) {
      DqdaHeadArgs fz{};
      if (tile_alone) { fz.dxc = h->dZc[0] + h->S; fz.lddxc = lc.kp[0]; }
      fz.aout16 = h->aout16; fz.dA16 = h->dA16; fz.W = wat(h, DQNHIP_ACTOR, la.hw_off); fz.H = Hh; fz.rows = B;
      fz.t16 = NarrowTile16{h->w16[DQNHIP_CRITIC][0] + h->S, h->k16[1][0], h->dZ16[1][1], lc.dims[1], lc.dims[1]}; fz.inv_ls = 1.0f / h->ls_q;
      fz.X416 = h->act16[1][L]; fz.dZ16 = h->dZ16[0][L]; fz.scale16 = h->ls_a; fz.ls_mult = lsm_a;
      // (DQNHIP_TUNE_SEPARATE_HEAD_SEED: q(s, mu(s)) came out of the dq = -1 head launch — no rider blocks)
      const QHeadRider qr{nullptr, wat(h, DQNHIP_CRITIC, lc.hw_off), wat(h, DQNHIP_CRITIC, lc.hb_off), h->q2, h->q_partial, Hc, B, fused_seed && !tile_alone ? (B + 3) / 4 : 0, h->act16[4][L]};
      HIPCHK(dqda_head_bwd_launch(fz, qr, st));
    }
    {
      HeadBwdArgs a{}; a.dXc = h->dZc[0]; a.ldx = lc.kp[0]; a.S = h->S; a.aout16 = h->aout16; a.dA16 = h->dA16;
      a.W = wat(h, DQNHIP_ACTOR, la.hw_off); a.X416 = h->act16[1][L]; a.H = Hh; a.rows = B; a.dZ = nullptr; a.ls_mult = lsm_a;
      if (fused_seed) {
        a.q_bias = wat(h, DQNHIP_CRITIC, lc.hb_off); a.q_out = h->q2; a.qsum_partial = h->q_partial;
        a.qr_W = wat(h, DQNHIP_CRITIC, lc.hw_off); a.qr_X416 = h->act16[4][L]; a.qr_H = Hc;
      }
      a.dW = h->g[0] + la.hw_off; a.db = h->g[0] + la.hb_off; a.partial = h->part[0] + la.part_off[L];
      const HeadWsum r{h->dA16, kAP, h->act16[1][L], Hh, B, a.dW, a.db, a.partial, kNO, Hh / 64};   // dA16: the post-invert diffs this launch leaves
      if (P.head_rides_a) { a.dW = nullptr; a.db = nullptr; a.partial = nullptr; }
      if (P.fuse_head) {}                                        // (k_dqda_head_bwd<true> above did all of it)
      else if (head_big_ok(h, B, Hh)) { a.dZ = nullptr; RC(head_backward_big<kNO>(h, st, a, h->dZ16[0][L], h->ls_a)); }
      else { a.dZ16 = h->dZ16[0][L]; a.scale16 = h->ls_a; RC(head_backward<kNO>(h, st, a)); }
      const TailsArgs tails_a = actor_tails(h);
      Bwd16Riders br; br.partial = part16 ? h->part[0] : nullptr;
      if (P.head_rides_a) br.rider = &r;
      if (P.tails_ride) br.tails = &tails_a;
      RC(tower_backward16(h, st, DQNHIP_ACTOR, 1, h->g[0], nullptr, B, true, false, h->ls_a, lsm_a, br));
      if (dp && !P.tails_ride) RC(tails_launch(st, tails_a));
    }
    return 0;
  }
  if (phase == 2) {
    const TickArgs tick = tick_args(h, dp);
    RC(optimiser_step(h, st, DQNHIP_ACTOR, dp, &tick));        // + iteration counters / statistics
    h->h_actor_iter += 1; h->h_critic_iter += 1;
    return 0;
  }
  return fail("phase must be 0, 1 or 2 (got %d)", phase);
}

int sync_dirty16(H* h) {
  if (!h->fp16) return 0;
  for (int net = 0; net < 4; ++net) if (h->w16_dirty[net]) RC(sync_w16(h, h->stream, net));
  return 0;
}

// ---- the update, in three phases (see dqnhip.h) ---------------------------------
// Step(1)'s four first tower layers in ONE launch: actor_target(s'), actor(s), critic(s, a) — each exactly what
// layer_forward(…, 0) computes — and the STATE half of critic_target(s', mu'(s'))'s first layer (K = the state columns; no bias, no
// ReLU; into h->Zs).  Its action half is a rank-10 update per row that the target actor's head kernel applies itself
// (HeadArgs::l1_*), so the launch of the critics' first layers between the heads and the critics' second layer is gone.
// with_actor false (the data-parallel overlap form): the online actor's whole forward runs later (phase 11) — three problems.
int first_layers_launch(H* h, hipStream_t st, int rows, bool with_actor) {
  const NetLayout &la = h->la, &lc = h->lc;
  GemmBatch b{}; b.n = with_actor ? 4 : 3;
  auto fill = [&](GemmProblem& p, int net, const NetLayout& l, const float* X, float* Y, int kred, bool finish) {
    p.P = wat(h, net, l.w_off[0]); p.ldp = l.kp[0];
    p.Q = X; p.ldq = l.kp[0];
    p.C = Y; p.ldc = l.kp[1];
    p.Pdim = l.dims[1]; p.Qdim = rows; p.Kred = kred;
    p.bias = finish ? wat(h, net, l.b_off[0]) : nullptr; p.relu = finish ? 1 : 0;
  };
  fill(b.prob[0], DQNHIP_ACTOR_TARGET, la, h->act[0][0], h->act[0][1], la.kp[0], true);
  fill(b.prob[1], DQNHIP_CRITIC, lc, h->act[3][0], h->act[3][1], lc.kp[0], true);
  fill(b.prob[2], DQNHIP_CRITIC_TARGET, lc, h->act[2][0], h->Zs, round_up(h->S, 64), false);
  b.prob[2].xcopy_dst = h->Wact_t; b.prob[2].xcopy_col = h->S; b.prob[2].xcopy_n = kNO;
  if (with_actor) fill(b.prob[3], DQNHIP_ACTOR, la, h->act[1][0], h->act[1][1], la.kp[0], true);
  return form_launch(h, st, first_layers_form(), b);
}
int run_phase(H* h, int phase, const int* idx_dev) {
  const UpdatePlan P = plan_of(h);
  select_panels(h, early_l0(h) ? (h->cap_u & 1) : 0);
  if (h->fp16) return run_phase16(h, phase, idx_dev);
  const int B = h->B, L = h->L;
  const NetLayout &la = h->la, &lc = h->lc;
  const bool dp = P.dp;
  const int Hh = la.dims[L], Hc = lc.dims[L];
  hipStream_t st = h->stream;
  const bool split = phase == 10;          // phase 10 = phase 0 without the online actor's forward, 11 = that forward
  HeadArgs hA = actor_head_args(h, DQNHIP_ACTOR); hA.X = h->act[1][L]; hA.xc = h->Xc_pl;
  if (phase == 11) {
    FwdPass pA{DQNHIP_ACTOR, &la, h->act[1]};
    RC(tower_forward(h, st, &pA, 1, B));
    RC((head_forward<kNO, HEAD_ACTOR>(h, st, hA)));
    return 0;
  }
  if (phase == 0 || phase == 10) {
    RC(gather_launch(h, st, idx_dev));
    FwdPass pAT{DQNHIP_ACTOR_TARGET, &la, h->act[0]}, pA{DQNHIP_ACTOR, &la, h->act[1]};
    FwdPass pCT{DQNHIP_CRITIC_TARGET, &lc, h->act[2]}, pC1{DQNHIP_CRITIC, &lc, h->act[3]};
    HeadArgs hAT = actor_head_args(h, DQNHIP_ACTOR_TARGET); hAT.X = h->act[0][L]; hAT.xc = h->Xc_nx;
    // Step(1)'s head arithmetic (q', q, TD target, loss, dq, dZ_L) inside the critic's top-layer dgrad launch (k_dgrad_qtrain)
    // instead of a launch of its own: the online critic's top forward layer then also leaves U = (-w_h) lrelu'(x_L)
    const bool fuse_q = P.fuse_q;
    if (fuse_q) {
      pC1.seed_w = wat(h, DQNHIP_CRITIC, lc.hw_off); pC1.seed_out = h->U3;
      pC1.dot_w = pC1.seed_w; pC1.dot_out = h->qdot[1];
      pCT.dot_w = wat(h, DQNHIP_CRITIC_TARGET, lc.hw_off); pCT.dot_out = h->qdot[0];
    }
    FwdPass cp[2] = {pCT, pC1};
    // all four first layers of Step(1) in the update's first GEMM launch, critic_target's action half in the head kernel (first_layers_launch);
    // DQNHIP_TUNE_SEPARATE_CRITIC_FIRST_LAYERS: the critics' first layers in a launch of their own behind the heads
    const bool merged_l0 = P.first_layers_merged;
    if (merged_l0) {
      if (!(early_l0(h) && h->cap_u > 0)) RC(first_layers_launch(h, st, B, !split));     // (else: they rode in the previous update's last launch, k_adam_soft_l0)
      hAT.l1_zs = h->Zs; hAT.l1_wt = h->Wact_t;
      hAT.l1_b = wat(h, DQNHIP_CRITIC_TARGET, lc.b_off[0]); hAT.l1_y = h->act[2][1]; hAT.l1_ld = lc.kp[1]; hAT.l1_n = lc.dims[1];
    }
    if (split) {
      // data-parallel overlap form: the online actor's forward (phase 11) is left out so that it can
      // run while the critic gradients are being all-reduced
      RC(tower_forward(h, st, &pAT, 1, B, merged_l0 ? 1 : 0));
      RC((head_forward<kNO, HEAD_ACTOR>(h, st, hAT)));
    } else {
      // actor_target(s') [src/dqn.cpp:889-891] and actor(s) [:910-911, pre-update weights] layer by layer in one
      // launch each, then critic_target(s', mu'(s')) and the critic(s, a) train forward [:904] likewise
      FwdPass ap[2] = {pAT, pA};
      RC(tower_forward(h, st, ap, 2, B, merged_l0 ? 1 : 0));
      RC((head_forward<kNO, HEAD_ACTOR>(h, st, hAT, &hA)));     // both actors' heads in one launch
    }
    if (P.smooth) {
      // target policy smoothing: a~ over the mu'(s') columns the head left in Xc_nx (plan_of: the critics' first layers are behind this)
      const TargetNoiseHost* tn = h->tnoise;
      const TargetSmoothArgs sa{tn->cfg, h->st, h->aout_t16, h->Xc_nx, lc.kp[0], h->S, tn->smoothed16, tn->z16, tn->counter, B};
      HIPCHK(launch(st, k_target_smooth, dim3((B * kAP + 255) / 256), dim3(256), 0, sa));
    }
    RC(tower_forward(h, st, cp, 2, B, merged_l0 ? 1 : 0));
    HeadTrainArgs qt_args = q_train_args(h);
    qt_args.Xt = h->act[2][L]; qt_args.X = h->act[3][L];
    // with the head's dW / db riding in the net's last backward launch, the head's dZ comes out of this launch too
    if (P.head_rides_c) qt_args.dZ = h->dZc[L];
    qt_args.pdt = h->qdot[0]; qt_args.pd = h->qdot[1];
    if (!fuse_q) RC(q_train_launch(h, st, P, qt_args));      // (plan_of: prioritized replay and n-step returns never with fuse_q)
    // critic backward (rest of Step(1)): head (dgrad + ReLU' + wgrad fused), then tower; wgrad
    // writes (beta=0) so ClearParamDiffs/ZeroGradParameters (src/dqn.cpp:63-78, 908-909) vanish
    {
      HeadBwdArgs a{}; a.dyh = h->dq; a.lddy = 1; a.W = wat(h, DQNHIP_CRITIC, lc.hw_off); a.X4 = h->act[3][L];
      a.H = Hc; a.rows = B; a.dZ = h->dZc[L]; a.dW = h->g[1] + lc.hw_off; a.db = h->g[1] + lc.hb_off;
      a.partial = h->part[1] + lc.part_off[L];
      // the head's own gradients ride in the net's last backward launch (the first layer's narrow wgrad)
      const bool ride = P.head_rides_c;
      HeadWgradRider r{h->dq, 1, h->act[3][L], Hc, B, a.dW, a.db, a.partial, Hc / kRiderCW};
      if (!ride) RC(head_backward<1>(h, st, a));          // (riding: dZ came out of k_head_q_train, dW / db come from the rider)
      // data parallel: [loss, q, flag] tails for the exchange — one more block of the backward's last launch, or a launch of its own
      const TailsArgs tails_c = critic_tails(h);
      BwdRiders br;
      if (ride) br.rider = &r;
      if (fuse_q) { br.qtrain = &qt_args; br.qtrain_seed = h->U3; }
      if (P.tails_ride) br.tails = &tails_c;
      RC(tower_backward(h, st, lc, DQNHIP_CRITIC, h->g[1], h->part[1], h->act[3], h->dZc, B, true, false, br));
      if (dp && !P.tails_ride) RC(tails_launch(st, tails_c));
    }
    return 0;
  }
  if (phase == 1) {
    // ClipGradients + Adam + Net::Update of the critic, soft update of critic_target fused (one pass)
    FwdPass pC2{DQNHIP_CRITIC, &lc, h->act[4]};
    h->act[4][0] = h->Xc_pl;
    // the first layer of critic(s, mu(s)) rides in the critic's optimiser launch (FirstLayerRider: the workgroups that own W1 run it
    // on the weights they have just stepped); DQNHIP_TUNE_SEPARATE_FIRST_LAYER: a launch of its own (same bits)
    const bool ride_l0 = P.critic_l0;
    const FirstLayerRider fl{h->Xc_pl, lc.kp[0], h->act[4][1], lc.kp[1], B, lc.kp[0], lc.dims[1], lc.dims[1] / 16};
    // inside a multi-update graph the NEXT update's gather rides here too (its panels: the other parity), so that its first layers
    // can ride in the actor's launch
    const bool eg = ride_l0 && early_l0(h) && h->cap_u + 1 < h->cap_n;
    const GatherArgs g = eg ? gather_args(h, nullptr, h->cap_u + 1) : GatherArgs{};
    RC(optimiser_step(h, st, DQNHIP_CRITIC, dp, nullptr, ride_l0 ? &fl : nullptr, eg ? &g : nullptr));
    // The seed of BackwardFrom(q_values_layer) [:918-923] — q diff = -1 per row, taken through the head and the top
    // layer's ReLU, input gradient only (the reference's discarded critic dW, SURVEY a11, is never computed) — does not
    // depend on q: it comes out of the top tower layer's forward epilogue, and q(s, mu(s)) itself [:913-916], which only
    // the statistics read, rides in the chain's last launch.  DQNHIP_TUNE_SEPARATE_HEAD_SEED: a head-backward launch
    // between the forward and the backward chain (same arithmetic, one launch more).
    const bool fused_seed = P.fused_seed;
    if (fused_seed) { pC2.seed_w = wat(h, DQNHIP_CRITIC, lc.hw_off); pC2.seed_out = h->dZc[L]; }
    RC(tower_forward(h, st, &pC2, 1, B, ride_l0 ? 1 : 0));   // critic(s, mu(s)), UPDATED weights [:913-916]
    const QHeadRider qr{h->act[4][L], wat(h, DQNHIP_CRITIC, lc.hw_off), wat(h, DQNHIP_CRITIC, lc.hb_off), h->q2, h->q_partial, Hc, B, (B + 3) / 4};
    if (!fused_seed) {
      HeadBwdArgs a{}; a.dyh = nullptr; a.lddy = 1; a.W = wat(h, DQNHIP_CRITIC, lc.hw_off); a.X4 = h->act[4][L];
      a.H = Hc; a.rows = B; a.dZ = h->dZc[L];
      a.q_bias = wat(h, DQNHIP_CRITIC, lc.hb_off); a.q_out = h->q2; a.qsum_partial = h->q_partial;
      RC(head_backward<1>(h, st, a));
    }
    // dQ/da's last step, the inverting gradients (src/dqn.cpp:924-957) and the actor heads' backward (src/dqn.cpp:960-963) share
    // ONE launch (k_dqda_head_bwd) when the actor head's own gradients ride in the actor's last backward launch and the shapes
    // allow it (16 columns from the first action column inside the panel row, fewer than 1024 rows: dqda_head_shape_ok);
    // DQNHIP_TUNE_SEPARATE_ACTOR_HEAD_BWD: the narrow dgrad launch + k_head_bwd<10> (same arithmetic, one launch more)
    const bool ride_a = P.head_rides_a;
    const bool fuse_head = P.fuse_head;
    DqdaHeadArgs fz{};
    fz.aout16 = h->aout16; fz.dA16 = h->dA16; fz.W = wat(h, DQNHIP_ACTOR, la.hw_off); fz.X4 = h->act[1][L]; fz.dZ = h->dZa[L]; fz.H = Hh; fz.rows = B;
    {
      BwdRiders br; br.in_lo = h->S; br.in_hi = h->S + kNO;      // only the action columns of the input gradient are consumed
      if (fused_seed) br.qrider = &qr;
      if (fuse_head) br.fuse = &fz;
      RC(tower_backward(h, st, lc, DQNHIP_CRITIC, nullptr, nullptr, h->act[4], h->dZc, B, false, true, br));
    }
    // inverting gradients (src/dqn.cpp:924-957) + actor heads backward (src/dqn.cpp:960-963)
    {
      HeadBwdArgs a{}; a.dXc = h->dZc[0]; a.ldx = lc.kp[0]; a.S = h->S; a.aout16 = h->aout16; a.dA16 = h->dA16;
      a.W = wat(h, DQNHIP_ACTOR, la.hw_off); a.X4 = h->act[1][L]; a.H = Hh; a.rows = B; a.dZ = h->dZa[L];
      a.dW = h->g[0] + la.hw_off; a.db = h->g[0] + la.hb_off; a.partial = h->part[0] + la.part_off[L];
      HeadWgradRider r{h->dA16, kAP, h->act[1][L], Hh, B, a.dW, a.db, a.partial, Hh / kRiderCW};   // dA16: the post-invert diffs this launch leaves
      if (ride_a) { a.dW = nullptr; a.db = nullptr; a.partial = nullptr; }
      if (!fuse_head) RC(head_backward<kNO>(h, st, a));
      const TailsArgs tails_a = actor_tails(h);
      BwdRiders br;
      if (ride_a) br.rider = &r;
      if (P.tails_ride) br.tails = &tails_a;
      RC(tower_backward(h, st, la, DQNHIP_ACTOR, h->g[0], h->part[0], h->act[1], h->dZa, B, true, false, br));
      if (dp && !P.tails_ride) RC(tails_launch(st, tails_a));
    }
    return 0;
  }
  if (phase == 2) {
    // the actor's optimiser pass is the update's last launch: its block 0 also publishes
    // (critic_loss, avg_q) and advances the iteration / sampling counters
    const TickArgs tick = tick_args(h, dp);
    NextL0 n{};
    const bool next = early_l0(h) && h->cap_u + 1 < h->cap_n;
    if (next) {
      // the next update's first layers ride here: its panels (gathered in this update's critic launch) are those of the other parity
      const int pn = (h->cap_u + 1) & 1;
      n.a = ActorL0{h->Xa_s2[pn], h->Xa_n, la.kp[0], h->act[1][1], h->act[0][1], la.kp[1], B, la.dims[1], la.dims[1] / 16};
      n.c = PlainL0{h->w[DQNHIP_CRITIC] + lc.w_off[0], lc.kp[0], h->w[DQNHIP_CRITIC] + lc.b_off[0], h->Xc_tr, lc.kp[0], h->act[3][1], lc.kp[1],
                    B, lc.kp[0], lc.dims[1], nullptr, 0, 0, lc.dims[1] / 16};
      n.ct = PlainL0{h->w[DQNHIP_CRITIC_TARGET] + lc.w_off[0], lc.kp[0], nullptr, h->Xc_nx, lc.kp[0], h->Zs, lc.kp[1],
                     B, round_up(h->S, 64), lc.dims[1], h->Wact_t, h->S, kNO, lc.dims[1] / 16};
    }
    RC(optimiser_step(h, st, DQNHIP_ACTOR, dp, &tick, nullptr, nullptr, next ? &n : nullptr));
    h->h_actor_iter += 1; h->h_critic_iter += 1;
    return 0;
  }
  return fail("phase must be 0, 1, 2, 10 or 11 (got %d)", phase);
}

// ---- one chunk of a replay sweep, up to its row kernel (dqnhip_evaluate_memory / dqnhip_per_refresh) --------------------------
// Phase 0's gather and forward launches as the stand-alone update issues them (the first layers merged where the plan merges them),
// Step(1)'s head arithmetic in the launch of its own (k_head_q_train: the DQNHIP_TUNE_SEPARATE_Q_TRAIN form, whatever the plan says —
// there is no dgrad launch to carry it), then critic(s, mu(s)) on the critic AS IT STANDS, every layer from its launcher (no optimiser
// launch carries its first layer), and its q head.  Leaves q_t, q1, y, q2, aout16, the gathered reward / mc / term and the panels.
int sweep_forward(H* h, const int* idx_dev, DevState* flag_sink) {
  if (h->fp16) return fail("internal: sweep_forward on an fp16 learner");
  const UpdatePlan P = plan_of(h);
  select_panels(h, 0);
  const int B = h->B, L = h->L;
  const NetLayout &la = h->la, &lc = h->lc;
  hipStream_t st = h->stream;
  {
    // the gather's row blocks alone: its last block — this update's Adam corrections and soft-update switch into DevState — is not launched
    const GatherArgs g = gather_args(h, idx_dev, -1);
    HIPCHK(launch(st, k_gather, dim3(g.blocks - 1), dim3(256), 0, g));
  }
  HeadArgs hA = actor_head_args(h, DQNHIP_ACTOR); hA.X = h->act[1][L]; hA.xc = h->Xc_pl;
  HeadArgs hAT = actor_head_args(h, DQNHIP_ACTOR_TARGET); hAT.X = h->act[0][L]; hAT.xc = h->Xc_nx;
  FwdPass pAT{DQNHIP_ACTOR_TARGET, &la, h->act[0]}, pA{DQNHIP_ACTOR, &la, h->act[1]};
  FwdPass pCT{DQNHIP_CRITIC_TARGET, &lc, h->act[2]}, pC1{DQNHIP_CRITIC, &lc, h->act[3]};
  const bool merged_l0 = P.first_layers_merged;
  if (merged_l0) {
    RC(first_layers_launch(h, st, B, true));
    hAT.l1_zs = h->Zs; hAT.l1_wt = h->Wact_t;
    hAT.l1_b = wat(h, DQNHIP_CRITIC_TARGET, lc.b_off[0]); hAT.l1_y = h->act[2][1]; hAT.l1_ld = lc.kp[1]; hAT.l1_n = lc.dims[1];
  }
  const FwdPass ap[2] = {pAT, pA}, cp[2] = {pCT, pC1};
  RC(tower_forward(h, st, ap, 2, B, merged_l0 ? 1 : 0));
  RC((head_forward<kNO, HEAD_ACTOR>(h, st, hAT, &hA)));
  RC(tower_forward(h, st, cp, 2, B, merged_l0 ? 1 : 0));
  HeadTrainArgs t = q_train_args(h);
  t.Xt = h->act[2][L]; t.X = h->act[3][L]; t.st = flag_sink;
  HIPCHK(launch(st, k_head_q_train, dim3((B + 3) / 4), dim3(256), 0, t));
  FwdPass pC2{DQNHIP_CRITIC, &lc, h->act[4]};
  RC(tower_forward(h, st, &pC2, 1, B));
  HeadArgs hq{}; hq.X = h->act[4][L]; hq.ldx = lc.dims[L]; hq.H = lc.dims[L]; hq.rows = B;
  hq.W = wat(h, DQNHIP_CRITIC, lc.hw_off); hq.b = wat(h, DQNHIP_CRITIC, lc.hb_off); hq.q = h->q2;
  RC((head_forward<1, HEAD_Q>(h, st, hq)));
  return 0;
}

int to_bf16_launch(H* h, int net) {
  HIPCHK(launch(h->stream, k_to_bf16, dim3(1024), dim3(256), 0, (const float*)h->g[net], layout_of(h, net).arena / 4, h->g16[net]));
  return 0;
}
int shard_scal_launch(H* h, float* tail) {
  HIPCHK(launch(h->stream, k_shard_scal, dim3(1), dim3(256), 0, (const float*)h->part_dp, h->n_part_dp, tail));
  return 0;
}
// dynamic-LDS limits, for THIS unit's copies of the kernels (it launches every kernel of the update)
int prepare_kernels(const H* h) {
  if (h->fp16) HIPCHK(hgemm_prepare_all());
  HIPCHK(direct_prepare_all());
  if (h->head_slab2 != nullptr) {                          // head_big_ok
    HIPCHK(direct_prepare(k_head_bwd_big<1>, (int)head_bwd_big_lds_bytes<1>()));
    HIPCHK(direct_prepare(k_head_bwd_big<kNO>, (int)head_bwd_big_lds_bytes<kNO>()));
  }
  return 0;
}

}  // namespace dqnhip_host

extern "C" {

// Solver::ApplyUpdate() of one net in isolation (actor_solver_->ApplyUpdate(), src/dqn.cpp:964; the tail of
// critic_solver_->Step(1), :904) on the gradient currently in the net's arena (e.g. dqnhip_set_params(KIND_G)):
// ClipGradients + Adam + Net::Update + the soft update of that net's target under the condition of :967, then
// set_iter(iter + 1) of that solver (:965).  The clip norm is taken from the arena itself (k_sumsq), as after an
// all-reduce; the same k_adam_soft pass as inside an update.
int dqnhip_apply_update(dqnhip_handle h, int32_t net) {
  if (!h) return fail("null handle");
  h->epoch += 1;
  if (net != DQNHIP_ACTOR && net != DQNHIP_CRITIC) return fail("net must be ACTOR or CRITIC");
  if (h->next_phase != 0) return fail("dqnhip_apply_update: a phased update is in progress (next phase %d)", h->next_phase);
  RC(feature_refuse(h, kFeatSched, "dqnhip_apply_update"));
  HIPCHK(hipSetDevice(h->cfg.device));
  RC(sync_dirty16(h));
  const NetLayout& l = layout_of(h, net);
  HIPCHK(launch(h->stream, k_sumsq, dim3(h->n_part_dp), dim3(256), 0, h->g[net], l.arena / 4, h->part_dp));
  RC(adam_launch(h, h->stream, net, h->part_dp, h->n_part_dp, 0, l.arena, nullptr, false));   // no gather ran: the pass evaluates its own correction
  HIPCHK(launch(h->stream, k_advance_iter, dim3(1), dim3(1), 0, h->st, (int)net, h->stats_dev));
  if (net == DQNHIP_ACTOR) h->h_actor_iter += 1; else h->h_critic_iter += 1;
  return 0;
}

// Solver::ApplyUpdate() of one net evaluated the way a `world`-rank group with a SHARDED optimiser evaluates it
// (DQNHIP_DP_SHARD_OPT), by this one learner standing in for every rank in turn: per slice r the sum of squares of the
// gradient's floats [r, r + 1) * arena / world (k_sumsq + k_shard_scal — each rank's share of the clip norm), their sum in
// rank order (what the 4-float all-reduce leaves on every rank), then clip + Adam + Net::Update + soft update on slice r with
// that norm (k_adam_soft on the sub-range), then set_iter(iter + 1).  No exchange is needed because the gradient in the
// arena already IS the reduced one.  world = 1 is dqnhip_apply_update bit for bit; world > 1 differs from it only through
// the order in which the clip norm is summed (identical bits whenever the clip is inactive).
int dqnhip_apply_update_sharded(dqnhip_handle h, int32_t net, int32_t world) {
  if (!h) return fail("null handle");
  h->epoch += 1;
  if (net != DQNHIP_ACTOR && net != DQNHIP_CRITIC) return fail("net must be ACTOR or CRITIC");
  if (h->next_phase != 0) return fail("dqnhip_apply_update_sharded: a phased update is in progress (next phase %d)", h->next_phase);
  RC(feature_refuse(h, kFeatSched, "dqnhip_apply_update_sharded"));
  if (h->cfg.solver_type != DQNHIP_SOLVER_ADAM)
    return fail("dqnhip_apply_update_sharded: the %s solver has no sharded form in this version (DESIGN.md 9); use dqnhip_apply_update", dqnhip_solver_name(h->cfg.solver_type));
  const NetLayout& l = layout_of(h, net);
  if (world < 1 || l.arena % ((size_t)4 * world)) return fail("apply_update_sharded: the arena (%zu floats) must be divisible by 4 x world = %d", l.arena, 4 * world);
  HIPCHK(hipSetDevice(h->cfg.device));
  RC(sync_dirty16(h));
  if (!h->shard_total) HIPCHK(hipMalloc(&h->shard_total, 8 * sizeof(float)));
  const size_t slice = l.arena / (size_t)world;
  float* tail = h->shard_total + 4;
  for (int r = 0; r < world; ++r) {
    HIPCHK(launch(h->stream, k_sumsq, dim3(h->n_part_dp), dim3(256), 0, h->g[net] + r * slice, slice / 4, h->part_dp));
    HIPCHK(launch(h->stream, k_shard_scal, dim3(1), dim3(256), 0, (const float*)h->part_dp, h->n_part_dp, tail));
    HIPCHK(launch(h->stream, k_shard_accumulate, dim3(1), dim3(1), 0, h->shard_total, (const float*)tail, r == 0 ? 1 : 0));
  }
  for (int r = 0; r < world; ++r) RC(adam_launch(h, h->stream, net, h->shard_total, 1, r * slice, (r + 1) * slice, nullptr, false));
  HIPCHK(launch(h->stream, k_advance_iter, dim3(1), dim3(1), 0, h->st, (int)net, h->stats_dev));
  if (net == DQNHIP_ACTOR) h->h_actor_iter += 1; else h->h_critic_iter += 1;
  return 0;
}

int dqnhip_grad_buffer(dqnhip_handle h, int32_t net, void** dptr, size_t* nfloats) {
  if (!h) return fail("null handle");
  if (net != DQNHIP_ACTOR && net != DQNHIP_CRITIC) return fail("net must be ACTOR or CRITIC");
  if (dptr) *dptr = h->g[net];
  if (nfloats) *nfloats = layout_of(h, net).arena + 4;
  return 0;
}

}  // extern "C"
