// learner_args.hip.h — the ARGUMENT layer: the plain structs and constants that host code and kernels share.  No __global__,
// no launcher, nothing that instantiates a kernel: a host-only translation unit includes this (through learner_internal.hip.h)
// and embeds no device code.  Layers, includes pointing downwards only:
//   arguments   gemm_common.hip.h (GEMM problems, LaunchOn / launch, tails, flags), this header, lr_schedule.hip.h (Caffe's lr policies:
//               one function for the host and the device), gemm_plan.hip.h (the fp32 family's
//               launch forms: table, preconditions, choosers), hgemm_plan.hip.h (the fp16 family's problem description and tile choice)
//   bodies      gemm_bodies.hip.h, update_bodies.hip.h, solver_bodies.hip.h (the optimiser pass of the solvers other than Adam):
//               __device__ functions only; noise_bodies.hip.h (exploration noise: __host__ __device__, one text for both sides)
//   kernels     gemm_direct.hip.h, hgemm.hip.h, head_fwd_kernels.hip.h, head_kernels.hip.h, small_kernels.hip.h (gather, optimiser),
//               solver_kernels.hip.h (the optimiser launches of the solvers other than Adam; learner.hip),
//               io_kernels.hip.h (learner_io.hip), per_kernels.hip.h (prioritized replay; learner_per.hip), diag_kernels.hip.h,
//               sweep_kernels.hip.h (update diagnostics, replay sweep; learner_eval.hip), state_kernels.hip.h, snapshot_kernels.hip.h
//               (asynchronous state save / Caffe snapshot; learner_save_async.hip), env.hip.h (learner_env.hip): __global__ functions
//               and their launchers, grouped by the unit that launches them
// One include points upwards: head_fwd_kernels.hip.h holds the launcher head_forward<>, which takes the learner and reports through
// HIPCHK, and so includes learner_internal.hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gemm_common.hip.h"
#include "lr_schedule.hip.h"      // LrSchedule, lr_rate: one text for the host and the scalars block of the gather

namespace dqnhip {

constexpr int kNA = 4;    // kActionSize       src/dqn.hpp:20
constexpr int kNP = 6;    // kActionParamSize  src/dqn.hpp:21
constexpr int kNO = 10;   // ActorOutput       src/dqn.hpp:28
constexpr int kAP = 16;   // padded ActorOutput row (64 B)

// The bounds the inverting gradients push ActorOutput column j against (src/dqn.cpp:927-957): the four action logits in [-1, 1], the
// two powers (parameters 0 and 4) in [0, 100], the four angles in [-180, 180].  One definition: the head-backward kernels
// (head_kernels.hip.h) and the diagnostics' out-of-bounds counts (diag_kernels.hip.h) read it.
__host__ __device__ __forceinline__ void inverting_bounds(int j, float& mn, float& mx) {
  if (j < kNA) { mn = -1.0f; mx = 1.0f; }
  else { const int p = j - kNA; if (p == 0 || p == 4) { mn = 0.0f; mx = 100.0f; } else { mn = -180.0f; mx = 180.0f; } }
}

// Device-resident scalars of one learner (graph-replayable: nothing that
// changes per update is a kernel argument).
struct DevState {
  int ring_head;        // physical slot of logical transition 0
  int ring_size;        // std::deque::size()
  int actor_iter;       // actor_solver_->iter()
  int critic_iter;      // critic_solver_->iter()
  unsigned long long update_counter;  // Philox counter for on-device sampling
  float critic_loss;    // last update's return value .first
  float avg_q;          // .second
  // sticky until dqnhip_read_stats reports and clears them (the reference aborts instead:
  // CHECK(std::isfinite(target)) src/dqn.cpp:898, CHECK(std::isfinite(critic_loss)) :906)
  int flags;            // kFlagTarget | kFlagGradNorm
  int skipped_steps;    // optimiser steps skipped because the gradient norm was not finite
  // Adam's bias correction sqrt(1 - beta2^t) / (1 - beta1^t) of THIS update's actor / critic step, evaluated by a spare
  // block of the update's first launch (k_gather): two double pow() are a ~2 us dependent chain, which every block of
  // k_adam_soft otherwise sits through before its first load (measured: 23.2 -> 21.3 us per launch without it)
  // Two slots: inside a multi-update graph (dqnhip_update_async_n) update u uses slot u & 1, because the gather of
  // update u + 1 — which writes that update's scalars — rides in update u's LAST launch, the optimiser pass that still
  // reads update u's.  Everything else uses slot 0.
  float adam_corr[2][2];   // [slot][actor, critic]
  // ... and the soft-update switch of this update (max_iter() % soft_update_freq == 0 AFTER both increments,
  // src/dqn.cpp:967), from the same block: with both in DevState no block of k_adam_soft reads an iteration counter,
  // so the update's bookkeeping (tick_body) no longer has to wait for the last block of the last launch
  int soft_now[2];
  // multi-update graphs: (update_counter, actor_iter, critic_iter) as the graph's FIRST gather found them.  A gather
  // that rides ahead in the previous update's last launch runs beside the block that advances the live counters, so it
  // takes its own from here: base + its position in the graph (a capture-time constant).
  unsigned long long gbase_counter;
  int gbase_it[2];
  // Dynamic loss scaling (cfg.loss_scale_mode = DQNHIP_LOSS_SCALE_DYNAMIC, fp16 learner), indexed [actor, critic] like adam_corr: the
  // live power-of-two multiplier of the net's static scales and its reciprocal, side by side (ls_mult[1] multiplies ls_c, ls_mult[0]
  // both ls_q and ls_a), the finite steps in a row since the multiplier last moved, and how often it was halved / doubled.
  // WRITER: lane 0 of block 0 of the strided pass of that net's optimiser launch inside an update (adam_scalars), and nobody else on
  // the device.  READERS: the backward kernels of the update — ls_mult[1] between the update's gather and the critic's optimiser
  // launch, ls_mult[0] between the critic's optimiser launch and the actor's — always a kernel boundary away from the writer on the
  // one stream.  No block of an optimiser launch reads a multiplier: the other optimiser blocks only need "finite or not", the
  // riders that share those launches are the next update's gather (counters and indices) and, on fp32 learners only, first tower
  // layers.  So one slot is enough (adam_corr needs two because a rider WRITES the next update's value beside its reader).
  float ls_mult[2][2];     // [net][mult, 1 / mult]; {1, 1} in static mode (never read there)
  int ls_good[2];
  int ls_backoffs[2], ls_growths[2];
};
// (kFlagTarget / kFlagGradNorm: gemm_common.hip.h)

// ---- dynamic loss scaling: the decision, once per net per update (adam_scalars; tests/cpp/loss_scale_host.cpp runs it on the host) ----
struct LossScaleCfg { int growth_interval; float min_mult, max_mult; };      // growth_interval 0: never grow
struct LossScaleState { float mult; int good; };
struct LossScaleStep { LossScaleState st; int raise_flag, backed_off, grew; };
// finite: the net's gradient norm of this update.  Not finite: the step is skipped (the caller's business); the multiplier is halved
// and the update stays silent — unless the multiplier is at its floor already, where no backoff is left: raise kFlagGradNorm as the
// static mode does (a NaN weight, a hopeless scale).  Finite: after growth_interval such steps in a row the multiplier doubles, up to
// max_mult.  Multipliers are powers of two: halving and doubling are exact.
__host__ __device__ inline LossScaleStep loss_scale_step(LossScaleState s, bool finite, const LossScaleCfg& c) {
  LossScaleStep r{s, 0, 0, 0};
  if (!finite) {
    r.st.good = 0;
    if (s.mult <= c.min_mult) r.raise_flag = 1;
    else { r.st.mult = s.mult * 0.5f; r.backed_off = 1; }
    return r;
  }
  r.st.good = s.good + 1;
  if (c.growth_interval > 0 && r.st.good == c.growth_interval) {
    const float up = s.mult * 2.0f < c.max_mult ? s.mult * 2.0f : c.max_mult;
    r.grew = up > s.mult ? 1 : 0;
    r.st.mult = up > s.mult ? up : s.mult;
    r.st.good = 0;
  }
  return r;
}
// (the readers take the multiplier through ls_live, gemm_common.hip.h)

// ---- replay ring -------------------------------------------------------------
// SoA ring in HBM: state[cap][SP], next[cap][SP] (rows padded to SP = roundup(S,64)
// floats so every row is whole 256-B lines), act[cap][16], reward[cap], mc[cap],
// term[cap].  Logical index i (what the reference's deque exposes) lives in
// physical slot (head + i) % cap.
struct Ring {
  float* state; float* next; float* act; float* reward; float* mc; uint8_t* term;
  int cap, S, SP;
};

// Minibatch gather (src/dqn.cpp:846-887): one wave per sampled transition; each
// row of the ring is whole 256-B lines so the reads are fully coalesced.  Writes
// the five network input panels directly (Concat layer, src/dqn.cpp:446-448,
// folded in):  Xa_s=[s|0]  Xa_n=[s'|0]  Xc_tr=[s|a|0]  Xc_pl=[s|0..]  Xc_nx=[s'|0..]
struct GatherOut {
  float* Xa_s; float* Xa_n; int KaP;
  float* Xc_tr; float* Xc_pl; float* Xc_nx; int KcP;
  float* reward; float* mc; float* term; int* idx;
  // fp16 learner: the same five panels as fp16 (what its GEMMs read), written here instead of by a conversion launch
  // (null: fp32 learner).  Row strides = KaP / KcP (the fp16 learner pads both to 128).
  _Float16* Ha_s; _Float16* Ha_n; _Float16* Hc_tr; _Float16* Hc_pl; _Float16* Hc_nx;
};
// rs: the DevState that holds the ring's (head,size) — another learner's under
// ShareReplayMemory; st: this learner's (sampling counter)
// One gather: `blocks` - 1 row blocks (4 transitions each) + ONE scalars block (the last) whose first lanes evaluate this
// update's Adam corrections (t = iter + 1 of the actor / the critic: the counters only move in the update's last block)
// and its soft-update switch.
struct GatherArgs {
  Ring ring; const DevState* rs; DevState* st; const int* idx_in; uint64_t seed; GatherOut o; int B;
  float* corr; int* soft_now;       // DevState::adam_corr[slot], &DevState::soft_now[slot]
  float beta1, beta2; int soft_update_freq;
  // -1: a launch of its own — the live counters are this update's.  k >= 1: the gather of the k-th update of a
  // multi-update graph riding in update k-1's last launch — counters = DevState::gbase + k (see DevState).
  // -2: explicit indices, riding in the previous update's CRITIC optimiser launch (a kernel boundary before that update's tick):
  // counters = live + 1.
  int ahead;
  int store_base;                   // 1 (first update of a multi-update graph): also store the live counters to gbase
  int blocks;
  // A learner with an lr policy (device-resident, allocated at create; null: a fixed learner — the scalars block is the code it was):
  // corr[net] then carries the update's whole step scale, lr_rate(iter) x the bias correction in one float32 multiply (Caffe's
  // local_rate * correction), and the optimiser pass multiplies it by a.lr = 1.  A solver without a correction passes beta1 = beta2 = 0:
  // sqrt(1 - 0) / (1 - 0) is exactly 1.  Last member: nothing before it moves.
  const LrSchedule* sched;
};

// n-step returns (dqnhip_nstep_enable; k_gather_n): the gather's arguments + the window.  Row `row` of the minibatch starts at logical
// index li and covers m <= n transitions: up to the first terminal one, the ring's last one, or n.  reward[row] becomes the discounted
// sum R of the window's rewards, term / the next-state panels come from the window's last transition, disc[row] = gamma^m.
constexpr int kNstepMax = 64;    // one lane per transition of a window
struct GatherNArgs {
  GatherArgs g;
  int n;                               // 1 .. kNstepMax
  double gamma;                        // cfg.gamma as the head kernel reads it
  double* disc; int* steps;            // [B] out: gamma^m, m
};
// k_nstep_validate: the contiguity invariant n-step windows stand on, over the logical range [first, first + n)
struct NstepValidateArgs {
  Ring ring; const DevState* rs; int first, n;
  unsigned long long* violations; int* first_bad;      // += the non-terminal transitions whose stored next state is not their successor's state; min= their logical index
};

// ---- head layers (head_fwd_kernels.hip.h, head_kernels.hip.h) ----------------------------------------------------------------
enum HeadMode { HEAD_ACTOR = 0, HEAD_Q = 1, HEAD_Q_TRAIN = 2, HEAD_Q_POLICY = 3 };      // the MODE of k_head_fwd* / head_forward<>
struct HeadArgs {
  const float* X; int ldx; int H;      // [rows][H] tower top
  const _Float16* X16;                 // fp16 learner: the same panel in fp16 (then X is null)
  const float* W; const float* b;      // [NH][H], [NH]
  int rows;
  // HEAD_ACTOR
  float* out16;                        // [rows][16]
  float* xc; int ldxc; int xc_col;     // also written into a critic input panel (may be null)
  _Float16* xc16; int ldxc16;          // fp16 learner: and into that panel's fp16 copy (may be null)
  // HEAD_ACTOR, the target actor's head inside Step(1) (round 5; null: off): the block that has just formed mu'(s') of a row also
  // FINISHES the first tower layer of critic_target(s', mu'(s')) for that row.  The layer's state half
  // l1_zs[row][n] = sum_{k < S} W1[n][k] s'[k] came out of the update's first GEMM launch (no bias, no ReLU); here
  // l1_y[row][n] = lrelu((l1_zs[row][n] + sum_a W1[n][S + a] mu'[a]) + b1[n]), a in action order (an fma chain on l1_zs).
  // (With the action-column weights read in place — 40 dwords 512 B apart per thread — this kernel took 6.8 instead of 4.9 us.)
  const float* l1_zs; const float* l1_wt; const float* l1_b; float* l1_y; int l1_ld; int l1_n;   // l1_wt[a][n] = W1[n][S + a] (GemmProblem::xcopy_dst); l1_n <= 1024, % 4 == 0
  // HEAD_Q*
  float* q;                            // [rows]
  // HEAD_Q_TRAIN: TD target + Euclidean loss
  const float* q_target; const float* reward; const float* mc; const float* term;
  float* y; float* dq; float* loss_partial;   // loss_partial[gridDim.x]
  double gamma, beta; float inv_batch;
  // HEAD_Q_POLICY
  double* qsum_partial;                // [gridDim.x]
};

struct HeadArgs2 { HeadArgs p[2]; };

// k_head_q_train / k_dgrad_qtrain
struct HeadTrainArgs {
  const float* Xt; const float* Wt; const float* bt;   // target critic top / head
  const float* X; const float* W; const float* b;      // online critic top / head
  const _Float16* Xt16; const _Float16* X16;           // fp16 learner: the tower tops in fp16 (then Xt / X are null)
  int H, rows;
  const float* reward; const float* mc; const float* term;
  float* q_target; float* q; float* y; float* dq; float* loss_partial;
  double gamma, beta; float inv_batch;
  DevState* st;                                         // non-finite target flag (src/dqn.cpp:898)
  // not null: this launch also writes the online critic's tower-top gradient dZ[row][k] = (dq[row] * W[k]) * lrelu'(X[row][k])
  // — what k_head_bwd<1> computed from dq in a launch of its own.  The wave that forms a row's dq has just streamed that
  // row of X and W through its registers; the head's own dW / db ride elsewhere (head_wgrad_rider), so with this the
  // critic's head-backward launch of Step(1) is gone.
  float* dZ;
  // fp16 learner (round 6): the same gradient as the scaled fp16 panel its GEMMs read, dZ16[row][k] = (h16)(dZ * scale16) — with it
  // the fp16 learner's k_head_bwd<1> / k_head_bwd_big<1> + k_head_wred<1> launches of Step(1) are gone as well
  _Float16* dZ16; float scale16;
  // k_dgrad_qtrain: the two head dot products in 16-column pieces, [rows][H / 16], left by the top forward layers (GemmProblem::dot_w)
  const float* pdt; const float* pd;
  const float* ls_mult;                                 // dynamic loss scaling: scale16 is multiplied by *ls_mult (DevState::ls_mult[1]; null: static)
};

// k_head_q_train_w (prioritized replay): k_head_q_train's arguments + the importance weights' inputs and outputs
struct HeadTrainWArgs {
  HeadTrainArgs t;
  const float* prob;                   // [rows]: the sampling probability of each row's transition (k_per_sample / k_per_fill)
  float* w; float* td_abs;             // [rows] out: the row's weight, |q - target|
  float beta0; int beta_anneal_iters;  // beta = min(1, beta0 + (1 - beta0) critic_iter / beta_anneal_iters); 0 iterations: constant
};

// k_head_q_train_n<WEIGHTED> (n-step returns): k_head_q_train's (WEIGHTED: k_head_q_train_w's) arguments + each row's discount, which
// takes t.gamma's place; t.reward holds the window's discounted reward sum (k_gather_n).  Not WEIGHTED: prob / w / td_abs are unused
struct HeadTrainNArgs {
  HeadTrainWArgs w;
  const double* disc;                  // [rows]: gamma^m of each row's window
};

// k_head_bwd
struct HeadBwdArgs {
  const float* dyh; int lddy;          // NH==1: dq[rows] (null: -1 per row, no wgrad)
  const float* dXc; int ldx; int S;    // actor: critic input gradient (invert source)
  const float* aout16;                 // actor: mu(s) for the inverting bounds
  float* dA16;                         // actor: post-invert head diffs (debug / parity)
  const float* W; const float* X4; int H; int rows;
  const _Float16* X416;                // fp16 learner: the tower top in fp16 (then X4 is null)
  float* dZ; float* dW; float* db; float* partial;
  float* slab;                         // [RC][H/64][NH][64] per-row-chunk partial dW
  int* ticket;                         // [H/64] arrival counters, zero before and after every launch
  // rider (NH == 1, dq = -1 pass): the y-rows >= rc_blocks of the grid compute q = head(X4) + avg-Q partials
  // — the critic(s, mu(s)) head forward (src/dqn.cpp:913-916).  The -1 seed does not depend on q, so the
  // two used to be separate dependent launches for no reason.
  int rc_blocks;                       // row chunks of the backward part (0: gridDim.y)
  const float* q_bias; float* q_out; double* qsum_partial;
  // the rider's own head (fp16 learner: the critic(s, mu(s)) head rides in the ACTOR heads' backward launch — its seed comes
  // out of the critic's top forward layer, HGemm::seed_w); null: the launch's own W / X4 / X416 / H (the dq = -1 launch)
  const float* qr_W; const float* qr_X4; const _Float16* qr_X416; int qr_H;
  // fp16 learner: also emit the tower-top gradient as the scaled fp16 panel the fp16 GEMMs read (dZ16 [rows][H])
  // instead of a separate conversion launch
  _Float16* dZ16; float scale16;
  const float* ls_mult;                // dynamic loss scaling: scale16 is multiplied by *ls_mult (null: static)
};

// the fp16 operands of a narrow dgrad tile (dgrad_narrow_tile16, gemm_bodies.hip.h)
struct NarrowTile16 { const _Float16* P; int ldp; const _Float16* Q; int ldq; int Kred; };
// k_dqda_head_bwd
struct DqdaHeadArgs {
  GemmProblem pr;                          // critic first layer's narrow dgrad: P = W_0 + S (16 columns from the first action column), Q = dZ_1, Kred = width of layer 1
  const float* aout16; float* dA16;        // mu(s) [rows][16]; post-invert diffs [rows][16] (column chunk 0 writes them)
  const float* W; const float* X4;         // actor head weights [10][H], actor tower top [rows][H]
  float* dZ;                               // actor tower-top gradient [rows][H]
  int H, rows, row_tiles;                  // row_tiles = rows / 16
  // fp16 learner (F16 = true, round 6: its layer-0 dgrad launch + k_head_bwd<10> in one): the tile from the fp16 operands
  // (dgrad_narrow_tile16; t16.P = W16_0 + S, t16.Q = the scaled dZ16_1), times inv_ls; the tower top read as fp16 (X416), the
  // tower-top gradient written as the scaled fp16 panel dZ16 = (h16)(dZ * scale16)
  NarrowTile16 t16; float inv_ls;
  const _Float16* X416; _Float16* dZ16; float scale16;
  // dynamic loss scaling: {mult, 1 / mult} of the actor (DevState::ls_mult[0]) — inv_ls is multiplied by ls_mult[1] (the incoming panel
  // carries ls_q x mult), scale16 by ls_mult[0] (the outgoing one carries ls_a x mult); null: static
  const float* ls_mult;
  // DQNHIP_TUNE_SEPARATE_ACTOR_HEAD_BWD on the fp16 learner: the launch only forms the tile and leaves its ten action columns, times
  // inv_ls, at dxc[row * lddxc + j] (the critic's first-layer input gradient panel at its first action column) for k_head_bwd<10>;
  // one workgroup per row tile, no head part.  Null: the fused form
  float* dxc; int lddxc;
};

// k_head_bwd_big / k_head_wred
struct HeadBwdBigArgs {
  HeadBwdArgs a;
  _Float16* dZ16; float scale16;                             // fp16 output (null: fp32 a.dZ only); dynamic loss scaling: times *a.ls_mult
  float* slab2;                                              // [rows/64][NH][H] then [rows/64][16]
  // rider (NH == 1, dq = -1 pass; a.q_out != null): blocks with blockIdx.x >= chunks compute q = head(X4) + the avg-Q
  // partials (critic(s, mu(s)) head forward, src/dqn.cpp:913-916), one wave per row — as in k_head_bwd
  int chunks;
};

// ---- rider blocks of GEMM launches (q_head_rider, head_wgrad_rider: gemm_bodies.hip.h) ------------------------------------------
struct QHeadRider {
  const float* X4; const float* W; const float* bias;   // tower top [rows][H], head weights [H], head bias [1]
  float* q_out; double* qsum_partial;                   // [rows] each
  int H, rows, blocks;                                  // blocks = ceil(rows / 4) (0: none)
  const _Float16* X416;                                 // fp16 learner: the tower top in fp16 (then X4 is null); last member (aggregate initialisers of the fp32 call sites leave it null)
};
struct HeadWgradRider {
  const float* dy; int lddy;
  const float* X4; int H, rows;
  float* dW; float* db; float* partial;     // [NH][H], [NH], one sum-of-squares slot per rider block (H / 16)
  int blocks;                               // H / kRiderCW rider blocks, FIRST in the grid (0: none)
};
constexpr int kRiderCW = 8;                    // columns per rider block (x 32 row groups)

// ---- optimiser (small_kernels.hip.h; the pass itself: update_bodies.hip.h) -----------------------------------------------------
struct TickArgs {
  DevState* st; float* critic_tail; float* actor_tail;
  const float* loss_partial; int n_loss; const double* q_partial; int n_q; float batch;
  // host-mapped (pinned) copy of {critic_loss, avg_q, flags}: written by the update's last block, so
  // that dqnhip_read_stats needs a stream sync but no device-to-host copy (null: none)
  float* host_stats;
};
struct AdamArgs {
  float* w; float* g; float* m; float* v; float* wt;
  _Float16* w16; _Float16* wt16;             // fp16 mode: fp16 mirrors of w / wt, same offsets (null otherwise)
  float* w_sh; float* wt_sh; size_t n4_sh;   // float4 [0, n4_sh) of w / wt live in another learner's arena (ShareParameters)
  size_t n4;                      // arena length / 4
  size_t skip4;                   // the strided pass starts here: float4 [0, skip4) belong to the launch's first-layer riders (0: none)
  const float* partial; int n_partial;
  const float* corr_pre;          // this step's bias correction, evaluated earlier in the update (DevState::adam_corr); null: here
  const int* soft_pre;            // with corr_pre: this update's soft-update switch (DevState::soft_now)
  float lr, beta1, beta2, eps, clip, tau;
  int soft_update_freq;
  int which;                      // 0 actor, 1 critic (selects the iter counter)
  DevState* st;
  // the update's last launch also does k_tick's work: the block that finishes last (arrival
  // ticket; no fence needed — it consumes nothing the other blocks of THIS launch produced, and
  // by then every block has read the iteration counters it is about to advance) runs tick_body
  int tick_on;                    // 1: block 0 also runs tick_body (requires corr_pre / soft_pre)
  TickArgs tick;
  // dynamic loss scaling (an optimiser pass INSIDE an update of a dynamic learner; else 0 and the static behaviour): block 0 of the
  // strided pass runs loss_scale_step on DevState::ls_mult[which] / ls_good[which]
  int ls_dynamic; LossScaleCfg ls;
};

// the first-layer riders of the optimiser launches (k_adam_soft_fwd1*, k_adam_soft_l0)
struct FirstLayerRider {
  const float* X; int ldx;      // [rows][Kp]: the layer's input panel, complete before this launch
  float* Y; int ldy;            // [rows][N] out
  int rows, Kp, N;              // Kp = 64 G, rows % 16 == 0, N % 16 == 0; W1 = arena float4 [0, N Kp / 4), b1 behind it
  int blocks;                   // N / 16
};
struct ActorL0 {
  const float* Xs; const float* Xn; int ldx;   // the next update's state / next-state panels [rows][64]
  float* Ys; float* Yn; int ldy;               // actor(s), actor_target(s') first-layer activations
  int rows, N;                                 // Kp = 64 (one float4 of W1 per rider thread)
  int blocks;                                  // N / 16
};
struct PlainL0 {
  const float* W; int ldw; const float* bias;  // [N][ldw]; bias null: none (and no ReLU: a partial pre-activation)
  const float* X; int ldx; float* Y; int ldy;
  int rows, Kred, N;                           // Kred = 64 or 128 (<= ldw)
  float* xcopy_dst; int xcopy_col, xcopy_n;    // GemmProblem::xcopy_dst (null: none)
  int blocks;                                  // N / 16
};

// k_local_reduce
struct LocalReduce { float* g[8]; int n; size_t n4; };

}  // namespace dqnhip
