/*
 * dqnhip.h — C-ABI of the MI355X-native (gfx950) actor-critic learner.
 *
 * This is the drop-in boundary for ONE hot path of mhauskn/dqn-hfo: the
 * dqn::DQN Update()/SelectAction(s)/AddTransition(s) surface declared in the
 * reference's src/dqn.hpp:56-134.  The reference has no FFI of its own (it is
 * a C++ class linked statically into bin/dqn, CMakeLists.txt:32-33); the
 * entry points below are what a `dqn::DQN` adaptor class binds to (see
 * INTEGRATION.md, include/dqn.hpp and dqn-hfo_amd/csrc/dqn_dropin.cpp).  Every function cites
 * the reference method it replaces.
 *
 * Conventions
 *   - plain C types only: pointers, sizes, ints, floats.  No torch, no HIP
 *     types in signatures (streams / device memory travel as void*).
 *   - every function returns 0 on success, non-zero on failure; the message is
 *     available from dqnhip_last_error() (thread-local).  The adaptor turns a
 *     non-zero status into LOG(FATAL), which is the reference's error
 *     convention (glog CHECK/abort, src/dqn.cpp:898,906 ...).
 *   - one handle == one learner == one HIP stream on one device.  Handles are
 *     not thread-safe (the reference uses one DQN per agent thread,
 *     src/dqn_main.cpp:264).
 *   - "host" pointers are ordinary CPU memory; "_device" variants take
 *     pointers to HBM on the handle's device.
 *   - ActorOutput layout (src/dqn.hpp:28, src/dqn.cpp:210-216): 10 floats
 *     [dash, turn, tackle, kick | dashPow, dashAng, turnAng, tackleAng,
 *      kickPow, kickAng].
 *   - dense parameter order (Caffe learnable_params order):
 *       actor : ip1.W[h1,S] ip1.b[h1] ... ip4.W ip4.b
 *               action_layer.W[4,h4] .b[4]  actionpara_layer.W[6,h4] .b[6]
 *       critic: ip1.W[h1,S+10] ip1.b ... ip4.W ip4.b  q_values_layer.W[1,h4] .b[1]
 *     all weights row-major [num_output, K] as in Caffe InnerProduct.
 */
#ifndef DQNHIP_H_
#define DQNHIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DQNHIP_ACTION_SIZE 4        /* kActionSize       src/dqn.hpp:20 */
#define DQNHIP_ACTION_PARAM_SIZE 6  /* kActionParamSize  src/dqn.hpp:21 */
#define DQNHIP_ACTOR_OUT 10         /* ActorOutput       src/dqn.hpp:28 */
#define DQNHIP_MAX_HIDDEN 8

/* which network a call refers to */
enum dqnhip_net {
  DQNHIP_ACTOR = 0,         /* actor_net_          src/dqn.hpp:189 */
  DQNHIP_CRITIC = 1,        /* critic_net_         src/dqn.hpp:191 */
  DQNHIP_ACTOR_TARGET = 2,  /* actor_target_net_   src/dqn.hpp:193 */
  DQNHIP_CRITIC_TARGET = 3  /* critic_target_net_  src/dqn.hpp:192 */
};

/* which per-parameter array: data, or solver history (Caffe SolverState
 * history = [h1_0..h1_P-1, h2_0..h2_P-1]), or last gradient.
 * KIND_M is history 1 (Adam's m; the momentum / accumulated-square history of the other solvers), KIND_V is history 2
 * (Adam's v, AdaDelta's update history; all zero and never touched under SGD, Nesterov, AdaGrad and RMSProp). */
enum dqnhip_param_kind {
  DQNHIP_KIND_W = 0,
  DQNHIP_KIND_M = 1,        /* history 1 */
  DQNHIP_KIND_V = 2,        /* history 2 */
  DQNHIP_KIND_G = 3
};

/* dqnhip_config.solver_type: Caffe's solvers (SolverParameter.type, the reference driver's -solver flag: src/dqn_main.cpp:30,
 * src/dqn.cpp:628-629).  0 — what a zero-filled field means — is Adam, the reference's default.  One type for both nets.
 * With gs = g * clip_scale (SGDSolver::ClipGradients), lr = actor_lr / critic_lr, mom = momentum, d = delta, rho = rms_decay,
 * float32 in this order (no bias correction, no use of the iteration):
 *   SGD       h1 = fmaf(lr, gs, mom*h0);  w1 = w0 - h1
 *   Nesterov  h1 = fmaf(lr, gs, mom*h0);  u = fmaf(1 + mom, h1, -(mom*h0));  w1 = w0 - u
 *   AdaGrad   h1 = fmaf(gs, gs, h0);  w1 = w0 - lr * (gs / (sqrtf(h1) + d))                      needs momentum == 0
 *   RMSProp   h1 = fmaf(1 - rho, gs*gs, rho*h0);  w1 = w0 - lr * (gs / (sqrtf(h1) + d))          needs momentum == 0, 0 <= rho < 1
 *   AdaDelta  h1 = fmaf(1 - mom, gs*gs, mom*h0);  u = gs * sqrtf((h2_0 + d) / (h1 + d));
 *             h2_1 = fmaf(1 - mom, u*u, mom*h2_0);  w1 = w0 - lr*u
 * The soft target update, the skipped step on a non-finite norm and loss scaling are the Adam learner's.
 * v1 limits of the five: no data parallelism (dp_world > 1, dqnhip_dp_init*, dqnhip_apply_update_sharded), no dqnhip_diag_collect,
 * no first-layer riders in the optimiser launches (the schedule is the one DQNHIP_TUNE_SEPARATE_FIRST_LAYER |
 * DQNHIP_TUNE_LATE_GATHER give an Adam learner). */
enum dqnhip_solver {
  DQNHIP_SOLVER_ADAM = 0,
  DQNHIP_SOLVER_SGD = 1,
  DQNHIP_SOLVER_NESTEROV = 2,
  DQNHIP_SOLVER_ADAGRAD = 3,
  DQNHIP_SOLVER_RMSPROP = 4,
  DQNHIP_SOLVER_ADADELTA = 5
};

/* Learner configuration.  Defaults in comments are the reference's.
 * Replaces: the compile-time constants of src/dqn.hpp:18-21, the Tower()
 * size list of src/dqn.cpp:425,449, the 11 learner gflags of
 * src/dqn.cpp:21-31 and the solver fields set in src/dqn_main.cpp:249-262. */
#define DQNHIP_FP32 0
#define DQNHIP_FP16 1
/* dqnhip_config.loss_scale_mode (fp16 learner) */
#define DQNHIP_LOSS_SCALE_STATIC 0   /* the built-in scales x loss_scale, fixed at create time (default)                 */
#define DQNHIP_LOSS_SCALE_DYNAMIC 1  /* ... x a power-of-two multiplier per net that the optimiser launch adjusts itself */

/* dqnhip_config.lr_policy: Caffe's learning-rate policies (SolverParameter.lr_policy, the reference driver's -lr_policy flag:
 * src/dqn_main.cpp:36, 255-256; SGDSolver::GetLearningRate).  0 — a zero-filled field — is "fixed", every learner
 * there was before the field existed.  With base = actor_lr / critic_lr and iter the net's solver iteration before its increment:
 *   fixed      base
 *   step       base * gamma^(iter / stepsize)                  (integer division)         stepsize > 0, gamma > 0
 *   exp        base * gamma^iter                                                          gamma > 0
 *   inv        base * (1 + gamma * iter)^(-power)                                         gamma >= 0
 *   multistep  base * gamma^k, k = number of stepvalues <= iter                           1..16 strictly increasing positive values, gamma > 0
 *   poly       base * max(0, 1 - iter / max_iter)^power        (0 from max_iter on)       max_iter > 0, power >= 0
 *   sigmoid    base / (1 + exp(-gamma * (iter - stepsize)))                               stepsize >= 0
 * Evaluated in double from the float32 fields and rounded once (Caffe: float powf) — ON THE DEVICE, per update, from the iteration
 * counters (a captured graph replays sixteen updates with sixteen different rates).  One schedule serves both nets.
 * weight_decay / regularization_type: SGDSolver::Regularize inside the optimiser pass, after the clip, decay_mult 1 on
 * weights and biases alike: gd = fmaf(weight_decay, r, g * clip_scale) with r = w (L2) or sign(w), sign(0) = 0 (L1); the solver's
 * rule then runs on gd.  The clip norm is the unregularised gradient's.
 * A learner with a policy or a decay (v1): single learner only (no dp_world > 1, dqnhip_dp_init*, dqnhip_apply_update*), no
 * dqnhip_diag_collect.  An Adam learner with a policy and no decay keeps its kernels (the rate reaches them through
 * DevState::adam_corr); every other such learner runs k_sched_soft<> and takes the schedule without first-layer riders. */
#define DQNHIP_LR_FIXED 0
#define DQNHIP_LR_STEP 1
#define DQNHIP_LR_EXP 2
#define DQNHIP_LR_INV 3
#define DQNHIP_LR_MULTISTEP 4
#define DQNHIP_LR_POLY 5
#define DQNHIP_LR_SIGMOID 6
#define DQNHIP_LR_MAX_STEPVALUES 16
#define DQNHIP_REG_L2 0
#define DQNHIP_REG_L1 1

typedef struct dqnhip_config {
  int32_t struct_size;       /* = sizeof(dqnhip_config); ABI check (or that size less the 96 bytes of the lr_policy ..
                                regularization_type block: a caller compiled before it existed — a fixed learner without decay) */
  int32_t minibatch;         /* kMinibatchSize (32); multiple of 32           */
  int32_t state_size;        /* num_features = 50 + 9*players; >= 1           */
  int32_t num_hidden;        /* tower depth (4); 1..DQNHIP_MAX_HIDDEN         */
  int32_t hidden[DQNHIP_MAX_HIDDEN]; /* {1024,512,256,128}; multiples of 64   */
  int32_t replay_capacity;   /* FLAGS_memory (500000)                         */
  int32_t soft_update_freq;  /* FLAGS_soft_update_freq (1)                    */
  double gamma;              /* FLAGS_gamma (.99) — double, as the reference  */
  double beta;               /* FLAGS_beta  (.5)                              */
  double tau;                /* FLAGS_tau   (.001); applied as float          */
  float actor_lr;            /* FLAGS_actor_lr  (1e-5)                        */
  float critic_lr;           /* FLAGS_critic_lr (1e-3)                        */
  float momentum;            /* FLAGS_momentum (.95): Adam beta1; SGD / Nesterov momentum; AdaDelta decay;
                                must be 0 for AdaGrad and RMSProp               */
  float momentum2;           /* FLAGS_momentum2 (.999): Adam beta2; read by no other solver */
  float delta;               /* Caffe SolverParameter.delta (1e-8): Adam eps; AdaGrad / RMSProp: added to the root;
                                AdaDelta: inside both roots; SGD / Nesterov: not read */
  float clip_gradients;      /* FLAGS_clip_grad (10); < 0 disables            */
  int32_t device;            /* HIP device ordinal                            */
  int32_t dp_world;          /* data-parallel world size (1 = single GPU)     */
  int32_t dp_rank;           /* this learner's rank in the DP group           */
  int32_t use_graph;         /* 1: replay the update as a captured hipGraph   */
  uint64_t seed;             /* counter-based RNG key for on-device sampling  */
  void* stream;              /* optional hipStream_t to run on (NULL: own)    */
  void* grad_arena;          /* optional caller-owned device memory that will
                                hold both gradient arenas (so torch.distributed
                                can all-reduce it in place); NULL: library
                                allocates.  Size: dqnhip_grad_arena_bytes().  */
  size_t grad_arena_bytes;
  int32_t precision;         /* DQNHIP_FP32 (default): exact-fp32 MFMA, the parity path.
                                DQNHIP_FP16: tower GEMMs take fp16 operands with fp32
                                accumulation (BASELINE.json config #5); master weights,
                                Adam, heads, TD target and losses stay fp32.  Needs
                                minibatch % 128 == 0 and hidden[i] % 128 == 0.       */
  float loss_scale;          /* FP16 only: multiplies the built-in static scales of the
                                back-propagated gradients (0 or 1: defaults).  An fp16
                                gradient panel that overflows makes the net's gradient
                                norm non-finite: the step is skipped and the next
                                dqnhip_read_stats fails ("Gradient norm not finite") —
                                unless loss_scale_mode is dynamic.                     */
  int32_t solver_type;       /* FLAGS_solver: DQNHIP_SOLVER_* (0 = Adam, the default, and what a zero-filled field means) */
  float rms_decay;           /* RMSProp's decay, Caffe SolverParameter.rms_decay (.99); read by no other solver.
                                Every field above these two keeps the offset it had before they existed — a caller compiled
                                against that header and run on this library (which fills the struct through
                                dqnhip_default_config) still sets what it means to set; from here on the offsets grew by 8. */
  int32_t lr_policy;         /* FLAGS_lr_policy: DQNHIP_LR_* (0 = fixed, the default)                              */
  float lr_gamma;            /* SolverParameter.gamma (NOT the discount, which is `gamma` above)                   */
  float lr_power;            /* SolverParameter.power                                                              */
  int32_t lr_stepsize;       /* SolverParameter.stepsize                                                           */
  int32_t lr_max_iter;       /* SolverParameter.max_iter (read by poly alone)                                      */
  int32_t lr_n_stepvalue;    /* number of lr_stepvalue entries in use (multistep)                                  */
  int32_t lr_stepvalue[DQNHIP_LR_MAX_STEPVALUES];   /* SolverParameter.stepvalue                                   */
  float weight_decay;        /* SolverParameter.weight_decay (0: none, the default)                                */
  int32_t regularization_type;   /* DQNHIP_REG_L2 (default) / DQNHIP_REG_L1.  These 24 words sit where they do for the reason
                                solver_type does; from here on the offsets grew by another 96. */
  int32_t tuning_flags;      /* DQNHIP_TUNE_* bits: A/B switches that select an alternative
                                SCHEDULE of the same arithmetic (0 = the measured winners).
                                The library reads no environment variable; every bit has a
                                parity test (tests/test_gpu_tuning_flags.py).          */
  /* Dynamic loss scaling (FP16, dp_world = 1 only; off by default — static mode launches the same
   * kernels and produces the same bits as before these fields existed).  Two multipliers live on the
   * device, both powers of two starting at 1: the critic's multiplies the critic step's scale, the
   * actor's those of the dQ/da pass and the actor step.  Once per net per update, inside that net's
   * optimiser launch (captured graphs included; no extra launch, no host read):
   *   norm not finite           -> the step is skipped as in static mode (dqnhip_skipped_steps counts it),
   *                                the multiplier is halved, the update reports NO error;
   *   ... at loss_scale_min_mult -> no backoff is left: "Gradient norm not finite" as in static mode;
   *   norm finite                -> the step is taken; after loss_scale_growth_interval such steps in a row
   *                                the multiplier doubles, up to loss_scale_max_mult.
   * Gradients (dqnhip_get_params(.., DQNHIP_KIND_G)) are unscaled in either mode, and a dynamic learner
   * whose multipliers are m computes, bit for bit, what a static one with loss_scale x m computes.
   * dqnhip_apply_update* never move the multipliers.  The Caffe snapshots do not carry them; the learner-state file
   * (dqnhip_save_state) does. */
  int32_t loss_scale_mode;            /* DQNHIP_LOSS_SCALE_STATIC (default) / DQNHIP_LOSS_SCALE_DYNAMIC            */
  int32_t loss_scale_growth_interval; /* finite steps in a row before the multiplier doubles; 0: never grow.
                                         Default 2000, the customary value of mixed-precision trainers —
                                         NOT measured on this workload.                                       */
  float loss_scale_min_mult;          /* floor, a power of two <= 1 (default 2^-12: the dQ/da scale x 2^-12 = 1,
                                         no scaling left)                                                     */
  float loss_scale_max_mult;          /* cap, a power of two >= 1 (default 1: nothing measured says scales above
                                         the built-in ones help)                                              */
} dqnhip_config;

/* fp16 learner: one wgrad launch per layer (a layer's dgrad + wgrad sharing a launch at small
 * minibatches) instead of ALL wgrads of a net + the bias-gradient sums in one launch. */
#define DQNHIP_TUNE_FP16_WGRAD_PER_LAYER 1
/* fp32 learner: the seed of the critic's dq = -1 backward pass (src/dqn.cpp:918-923) and q(s, mu(s)) from a head-backward
 * launch of their own instead of the top layer's forward epilogue / rider blocks of the chain's last launch. */
#define DQNHIP_TUNE_SEPARATE_HEAD_SEED 2
/* fp32 learner: a tower's backward as wgrad(i) + dgrad(i) per layer and a last launch with the first layer's wgrad alone,
 * instead of the shifted schedule dgrad(L-1) | wgrad(i+1) + dgrad(i) ... | wgrad(1) + wgrad(0) (same launch count). */
#define DQNHIP_TUNE_BWD_UNSHIFTED 4
/* The critic's first-layer action-column input gradient in a launch of its own (+ the q riders) and the inverting gradients + actor
 * heads' backward in another (k_head_bwd<10>), instead of all three in one launch (k_dqda_head_bwd, round 5; any tower-top width and
 * the fp16 learner below 1024 rows since round 6 — there the launch of its own is k_dqda_head_bwd<true> forming the tile alone,
 * DqdaHeadArgs::dxc, so that both precisions cut the fused form's arithmetic in two: bit-identical dQ/da). */
#define DQNHIP_TUNE_SEPARATE_ACTOR_HEAD_BWD 8
/* fp32 learner: Step(1)'s head arithmetic (q', q, TD target, loss, dq, the tower-top gradient) in a launch of its own
 * (k_head_q_train) instead of inside the critic's top-layer dgrad launch (k_dgrad_qtrain, round 5: the two head dot products
 * arrive in 16-column pieces from the critics' top forward layers).  The two forms differ by fp32 round-off only (another fixed
 * summation order for q', q; the per-row scalar dq applied after the dgrad's reduction instead of before). */
#define DQNHIP_TUNE_SEPARATE_Q_TRAIN 16
/* fp32 learner: the first tower layer of critic(s, mu(s)) in a launch of its own instead of inside the critic's optimiser launch
 * (FirstLayerRider, round 5: the optimiser workgroups that own W1 run the layer on the weights they have just stepped).  Same bits. */
#define DQNHIP_TUNE_SEPARATE_FIRST_LAYER 32
/* fp32 learner, Step(1): the two critics' first tower layers in a launch of their own behind the actor heads, instead of
 * critic(s, a)'s in the update's first GEMM launch and critic_target(s', mu'(s'))'s split into a state half (that launch) and an
 * action half applied by the target actor's head kernel (round 5).  critic_target's first layer then differs by fp32 round-off
 * (another summation order); everything else is the same arithmetic. */
#define DQNHIP_TUNE_SEPARATE_CRITIC_FIRST_LAYERS 64
/* fp32 learner, multi-update graphs (dqnhip_update_async_n): the next update's gather in the update's LAST launch and its four first
 * layers in a launch of their own (rounds 3-5), instead of the gather in the critic's optimiser launch and the first layers as riders
 * of the actor's optimiser launch (round 5).  Same bits. */
#define DQNHIP_TUNE_LATE_GATHER 128
/* No kernarg preload.  The chain's fp32 GEMM kernels and the two head kernels take, in front of their argument struct, up to 14 scalar words that gfx950
 * delivers in SGPRs at wave launch (what a workgroup's first operand loads are addressed from); with this bit the host marks every
 * such block "not valid" and the workgroups read everything from the argument struct, behind one uniform branch.  Same bits. */
#define DQNHIP_TUNE_NO_KERNARG_PRELOAD 256

typedef struct dqnhip_learner* dqnhip_handle;

/* Fill *cfg with the reference defaults (B=32, tower 1024-512-256-128, replay
 * 500k, gamma .99, beta .5, tau .001, Adam .95/.999, lr 1e-5/1e-3, clip 10). */
void dqnhip_default_config(dqnhip_config* cfg, int32_t state_size);

/* Caffe's type string of a DQNHIP_SOLVER_* value ("Adam", "SGD", "Nesterov", "AdaGrad", "RMSProp", "AdaDelta"); NULL: no such solver. */
const char* dqnhip_solver_name(int32_t solver_type);
/* Caffe's lr_policy string of a DQNHIP_LR_* value ("fixed", "step", "exp", "inv", "multistep", "poly", "sigmoid"); NULL: no such policy. */
const char* dqnhip_lr_policy_name(int32_t lr_policy);

/* Bytes the caller must provide in cfg->grad_arena (0 on invalid config). */
size_t dqnhip_grad_arena_bytes(const dqnhip_config* cfg);

/* Thread-local message of the last failure in this thread. */
const char* dqnhip_last_error(void);

/* Replaces DQN::DQN + DQN::Initialize (src/dqn.cpp:457-483, 622-662):
 * allocates nets (gaussian(0.01) weights, zero biases, src/dqn.cpp:350-352),
 * Adam state, target nets as hard copies (CloneNet, :660-661) and the
 * device-resident replay ring. */
int dqnhip_create(const dqnhip_config* cfg, dqnhip_handle* out);
/* Replaces DQN::~DQN (src/dqn.cpp:485). */
int dqnhip_destroy(dqnhip_handle h);

/* ---- the hot path ------------------------------------------------------ */

/* Replaces DQN::UpdateActorCritic (src/dqn.cpp:828-972): one full update —
 * minibatch gather, target-net forward, TD target, critic Step (fwd, bwd,
 * clip, Adam), actor forward, critic forward, critic input-gradient,
 * inverting gradients, actor backward, clip, Adam, soft target update.
 * idx_host: B logical replay indices in [0, memory_size) — the explicit form
 * of SampleTransitionsFromMemory (src/dqn.cpp:501-509); NULL = sample on the
 * device with the counter-based generator.  Blocks until the update is done
 * and returns (critic_loss, avg_q) exactly as the reference's return value. */
int dqnhip_update(dqnhip_handle h, const int32_t* idx_host,
                  float* critic_loss, float* avg_q);

/* One-deep pipelined dqnhip_update: enqueues update t and returns (critic_loss, avg_q) of update t-1
 * ((0, 0) on the first call).  What dqnhip_update costs beside the kernels — the host's index draw, the
 * H2D copy of the indices and a blocking read-back per update — then overlaps the previous update
 * instead of idling the device; the indices and scalars use two pinned slots each.  Semantic
 * difference to the reference's UpdateActorCritic: the returned pair (and a "Target not finite!" /
 * "Critic loss not finite!" failure) lags by one update; dqnhip_read_stats drains the last one. */
int dqnhip_update_pipelined(dqnhip_handle h, const int32_t* idx_host,
                            float* critic_loss, float* avg_q);

/* dqnhip_update for a caller that runs its updates in bursts of blocking calls — the reference's driver:
 * `for (i < n_updates) dqn->Update()`, src/dqn_main.cpp:359-361, each Update() drawing its indices on the host
 * (src/dqn.cpp:501-509) and returning (critic_loss, avg_q) — and can say which indices its NEXT call will bring
 * (idx_next, NULL: unknown).  The next update's minibatch gather then rides in this update's critic optimiser launch and
 * its four first tower layers in the actor's, as inside dqnhip_update_async_n's sixteen-update graphs, instead of heading
 * the next call's chain (~12 us of ~300).  What rode along is used only if the next call's idx_host equals this call's
 * idx_next element for element AND no entry point changed weights, iteration counters or the replay memory in between
 * (AddTransition(s), set_params, Load*, Restore*, CloneNet, sharing, any other update call, an env step); otherwise the
 * next call simply starts a fresh chain.  Every update computes what dqnhip_update computes on the same indices, bit for
 * bit.  Learners the riders do not fit (see dqnhip_get_update_plan: early_gather_l0; fp16, data-parallel, sharing
 * learners; use_graph = 0) run dqnhip_update.  The drop-in draws idx_next from a COPY of its std::mt19937 and adopts the
 * copy's state only when the prediction held, so the engine's observable call order is the reference's.
 * critic_loss == avg_q == NULL: enqueue only (the caller works while the update runs — the drop-in draws the prediction
 * after next — and collects the pair with dqnhip_read_stats). */
int dqnhip_update_chained(dqnhip_handle h, const int32_t* idx_host, const int32_t* idx_next,
                          float* critic_loss, float* avg_q);

/* Same update, enqueued on the stream without a host sync (the scalars stay
 * on the device; read them with dqnhip_read_stats). */
int dqnhip_update_async(dqnhip_handle h, const int32_t* idx_host);

/* n such updates back to back with on-device sampling — the reference's inner loops `for (i < n_updates)
 * dqn->Update()` (src/dqn_main.cpp:359-361) and DQN::Benchmark (src/dqn.cpp:487-498) as ONE call.  Exactly the
 * state n calls of dqnhip_update_async(h, NULL) leave (bit for bit); with use_graph the updates are replayed
 * sixteen to a hipGraph launch: the GPU idles ~8 us between two graph launches, and inside such a graph the minibatch
 * gather and the four first tower layers of update u + 1 ride in update u's two optimiser launches instead of heading the
 * next chain (~12 us; DQNHIP_TUNE_LATE_GATHER: the gather alone, in update u's last launch). */
int dqnhip_update_async_n(dqnhip_handle h, int32_t n);

/* The same bursts on the CALLER's indices: n updates, update u on idx_host[u*B .. u*B+B), enqueued on the learner's stream without
 * waiting for them.  The reference's driver calls DQN::Update() in bursts and discards what it returns (`for (i < n_updates)
 * dqn->Update()`, src/dqn_main.cpp:359-361; `while (dqn->max_iter() < FLAGS_max_iter) dqn->Update()`, :340-343; Update() is void and
 * only logs two smoothed values and snapshots, src/dqn.cpp:799-826), so nothing at that boundary needs one host wake-up and one graph
 * launch per update.  Exactly the state n calls of dqnhip_update(h, idx_host + u*B, ..) leave, bit for bit (weights, m, v, iteration
 * counters, replay bookkeeping, sampling counter); with use_graph the updates are replayed as graphs of 16 / 8 / 4 / 2 / 1 updates,
 * cut as dqnhip_update_async_n cuts n, each position reading its indices from a pinned index bank and writing its scalars into a
 * pinned stats bank (two banks: the host waits only for the graph BEFORE the one that is running).  All n*B indices are checked
 * against the current memory size before anything is enqueued ("update 1: sampled index 3 = 5000 out of range [0,3000)"; the learner
 * is then untouched); idx_host may be reused as soon as the call returns.  n == 0: no-op.  Data-parallel learners are refused. */
int dqnhip_update_indexed_n(dqnhip_handle h, const int32_t* idx_host /* [n][B] */, int32_t n);

/* Waits for the dqnhip_update_indexed_n updates enqueued so far and writes the (critic_loss, avg_q) pairs of those not yet
 * collected, in update order, up to cap; the rest stay collectable (8 bytes each, until collected or dqnhip_destroy).  *n_out: the
 * count.  The pairs are what the blocking calls return, bit for bit.  If a collected update raised a flag or left a non-finite loss
 * the pairs are still written and the call fails with dqnhip_read_stats' texts behind "collected update <i>: ", i the zero-based
 * position within this collection of the first such update (a flag is attributed to the update that raised it; the sticky device
 * flags are cleared as dqnhip_read_stats clears them).  dqnhip_read_stats after indexed updates still returns the last update's
 * pair and reports flags; it consumes no pair.
 * Attribution works on the sticky device flags: an update "raised" the bits the update before it had not left behind.  Two
 * consequences: (i) a flag raised by another entry point (dqnhip_update_async, ..) between two indexed bursts and never read is
 * attributed to the first update of the next burst - read the stats of non-indexed updates before mixing them with bursts if
 * the position matters; (ii) a flag that dqnhip_read_stats has already reported (and cleared on the device) is reported once
 * more by the dqnhip_collect_stats that hands out the update which raised it: it is a property of that update's pair. */
int dqnhip_collect_stats(dqnhip_handle h, float* critic_loss /* [cap] */, float* avg_q /* [cap] */,
                         int32_t cap, int32_t* n_out);

/* Data-parallel form of the same update, cut at its two exchange points:
 *   phase 0: gather .. critic backward      -> critic gradients ready
 *   phase 1: critic clip+Adam(+soft update), actor fwd, critic fwd, critic
 *            input-gradient, inverting gradients, actor backward
 *                                            -> actor gradients ready
 *   phase 2: actor clip+Adam(+soft update), iteration counters
 * Between phases the caller sum-all-reduces dqnhip_grad_buffer(net) across
 * the DP group (RCCL).  With dp_world == 1 running 0,1,2 back to back is
 * identical to dqnhip_update_async.
 * Overlap form: phase 10 = phase 0 without the online actor's forward mu(s)
 * (src/dqn.cpp:910-911), phase 11 = that forward; 11 touches neither gradient
 * arena, so 10, [start all-reduce of the critic gradients], 11, [wait], 1, .. hides
 * it behind the collective.  10 + 11 compute exactly what 0 computes. */
int dqnhip_update_phase(dqnhip_handle h, int32_t phase, const int32_t* idx_host);
/* Abandons a phased update that will not be completed (the caller's exchange step failed): the
 * next dqnhip_update_phase / dqnhip_update* starts a fresh update.  A phase that itself returns
 * non-zero abandons the update on its own.  Weights already stepped by phase 1 stay stepped. */
int dqnhip_update_abort(dqnhip_handle h);

/* Replaces one solver's ApplyUpdate() in isolation (actor_solver_->ApplyUpdate(), src/dqn.cpp:964; the
 * tail of critic_solver_->Step(1), :904): ClipGradients + Adam + Net::Update on the gradient currently in
 * the net's arena (e.g. written with dqnhip_set_params(.., DQNHIP_KIND_G, ..)), the soft update of that
 * net's target under the reference's condition (:967: max_iter() after both solvers' increments of a full
 * update), then set_iter(iter() + 1) of that solver (:965).  net = DQNHIP_ACTOR or DQNHIP_CRITIC.
 * The optimiser pass of dqnhip_update is this same kernel: tests pin it here on identical (w, g, m, v,
 * w', iter) to a few ulp. */
int dqnhip_apply_update(dqnhip_handle h, int32_t net);
/* The same step evaluated the way a `world`-rank group with a SHARDED optimiser (DQNHIP_DP_SHARD_OPT, below) evaluates it,
 * this one learner standing in for every rank in turn: each slice's share of the clip norm, their sum in rank order (what
 * the group's 4-float all-reduce leaves on every rank), clip + Adam + soft update slice by slice with that norm.  The
 * gradient in the arena already is the reduced one, so no exchange is involved: this pins the slice arithmetic and the
 * norm's composition on ONE GPU.  world = 1 equals dqnhip_apply_update bit for bit; world > 1 differs only through the
 * summation order of the norm (identical bits whenever the clip is inactive). */
int dqnhip_apply_update_sharded(dqnhip_handle h, int32_t net, int32_t world);

/* ---- the launch plan of this learner's update ---------------------------------------------
 * No reference counterpart (Caffe runs one layer at a time).  Which merged forms of the launch sequence behind
 * dqnhip_update* this learner takes — they depend on its shapes, its tuning flags, sharing and the data-parallel mode —
 * and how many kernels one update launches, COUNTED from a stream capture of the very sequence dqnhip_update* enqueues
 * (nothing executes).  Exists so that a shape predicate that stops matching shows up as a failed assertion
 * (tests/test_gpu_update_plan.py; bench.py prints it in `config.plan`) instead of as a silently slower schedule. */
#define DQNHIP_PLAN_FP16 1                      /* cfg.precision == DQNHIP_FP16 */
#define DQNHIP_PLAN_DATA_PARALLEL 2             /* phases cut for an exchange: dp_world > 1, or a one-rank group with bf16 exchange / sharded optimiser */
#define DQNHIP_PLAN_BWD_SHIFTED_CRITIC 4        /* the shifted backward schedule (see DQNHIP_TUNE_BWD_UNSHIFTED) in Step(1) */
#define DQNHIP_PLAN_BWD_SHIFTED_ACTOR 8         /* ... in the actor's backward */
#define DQNHIP_PLAN_HEAD_WGRAD_RIDES_CRITIC 16  /* the critic head's dW / db as rider blocks of the net's last backward launch (both precisions) */
#define DQNHIP_PLAN_HEAD_WGRAD_RIDES_ACTOR 32   /* ... the actor heads' */
#define DQNHIP_PLAN_Q_TRAIN_IN_DGRAD 64         /* fp32: k_dgrad_qtrain (see DQNHIP_TUNE_SEPARATE_Q_TRAIN); fp16: k_head_q_train also writes the tower-top gradient — either way Step(1) has no head-backward launch */
#define DQNHIP_PLAN_HEAD_SEED_FUSED 128         /* the dq = -1 seed from the top layer's forward epilogue (DQNHIP_TUNE_SEPARATE_HEAD_SEED) */
#define DQNHIP_PLAN_DQDA_HEAD_BWD 256           /* k_dqda_head_bwd (DQNHIP_TUNE_SEPARATE_ACTOR_HEAD_BWD) */
#define DQNHIP_PLAN_CRITIC_L0_RIDES 512         /* critic(s, mu(s))'s first layer inside the critic's optimiser launch (DQNHIP_TUNE_SEPARATE_FIRST_LAYER) */
#define DQNHIP_PLAN_FIRST_LAYERS_MERGED 1024    /* Step(1)'s four first layers in one launch (DQNHIP_TUNE_SEPARATE_CRITIC_FIRST_LAYERS) */
#define DQNHIP_PLAN_EARLY_GATHER_L0 2048        /* multi-update graphs: next gather / next first layers ride in the two optimiser launches (DQNHIP_TUNE_LATE_GATHER) */
#define DQNHIP_PLAN_DP_TAILS_RIDE 4096          /* data parallel: the [loss, q, flag] tails of the exchange ride in each net's last backward launch */
#define DQNHIP_PLAN_PRIORITIZED 8192            /* prioritized replay (dqnhip_per_enable): sampler / fill before, k_head_q_train_w inside, the write-back behind every update */
#define DQNHIP_PLAN_TARGET_SMOOTHING 32768      /* target policy smoothing (dqnhip_target_noise_enable): k_target_smooth behind the actors' heads, the critics' first layers in a launch of their own behind it */
#define DQNHIP_PLAN_NSTEP 16384                 /* n-step returns (dqnhip_nstep_enable): k_gather_n first, k_head_q_train_n in the head launch's place; the stand-alone sequence per update */
typedef struct dqnhip_update_plan {
  int32_t struct_size;          /* in: sizeof(dqnhip_update_plan) */
  int32_t forms;                /* DQNHIP_PLAN_* bits */
  int32_t launches_single;      /* kernels of one stand-alone update: eager, dqnhip_update, the one-update graph */
  int32_t launches_graph_first; /* ... of the first update of a multi-update graph (dqnhip_update_async_n / dqnhip_dp_update_n) */
  int32_t launches_in_graph;    /* ... of every later update of such a graph */
  int32_t updates_per_graph;    /* 16 */
  int32_t collectives;          /* RCCL calls per update once a communicator is up (not counted in launches_*), else 0 */
  int32_t solver_type;          /* DQNHIP_SOLVER_* of the learner (0 = Adam; this word was reserved, always 0, before the other solvers existed) */
  int32_t lr_policy;            /* DQNHIP_LR_* of the learner (appended; a caller may pass the struct_size without the two words and gets the rest) */
  int32_t regularised;          /* 1: weight_decay != 0 */
} dqnhip_update_plan;
/* The rate net's NEXT optimiser step will apply (lr_policy at the net's current iteration): the host build of the function the
 * device evaluates, at the host's mirror of the counter (dqnhip_get_iters; no sync).  Both evaluate in double and round once; the two pow() / exp() implementations may land on
 * different sides of a float32 rounding boundary, so the value can differ from the device's in the last float32 bit. */
int dqnhip_get_learning_rate(dqnhip_handle h, int32_t net, float* out);
/* Fails while a phased update is in progress or kernel timing is on; launches_* are 0 for a sharded optimiser (its
 * sequence contains collectives and is not captured here). */
int dqnhip_get_update_plan(dqnhip_handle h, dqnhip_update_plan* out);

/* Device pointer + length (floats) of one net's gradient arena, including a
 * 4-float tail [loss_sum, q_sum, 0, 0] so the two reported scalars ride in the
 * same all-reduce.  net = DQNHIP_ACTOR or DQNHIP_CRITIC. */
int dqnhip_grad_buffer(dqnhip_handle h, int32_t net, void** dptr, size_t* nfloats);

/* ---- native data parallelism: RCCL over xGMI inside the library --------------
 * The reference scales with threads + one mutex (src/dqn_main.cpp:62-63, 359-363); there is no
 * collective to replace.  One learner per GPU (cfg.dp_world / cfg.dp_rank), each with its own
 * replay shard; dqnhip_dp_update runs phase 0, sum-all-reduces the critic gradient arena, phase 1,
 * all-reduces the actor's, phase 2 — all on the learner's stream, no host sync.
 *   dqnhip_dp_unique_id   rank 0 creates the RCCL id (DQNHIP_DP_ID_BYTES); the launcher ships it
 *   dqnhip_dp_init        every rank: ncclCommInitRank, then rank 0's weights (4 nets), Adam
 *                         history and iterations are broadcast so the replicas start identical
 *   dqnhip_dp_init_file   the same with files as the rendezvous (one node, no launcher support):
 *                         dqnhip_dp_rendezvous_file + dqnhip_dp_init; rank 0 removes the files once the group is up
 *   dqnhip_dp_rendezvous_file   the rendezvous alone (needs no GPU): rank 0 passes the id in, ranks 1..world-1
 *                         receive it.  Every waiter publishes <path>.req<rank> with a fresh nonce and accepts <path>
 *                         only if it carries that nonce, rank 0 clears leftovers first: a file from an earlier or a
 *                         crashed job can never hand out a dead id, and the same path can be reused.
 * flags: 0 — ONE sum all-reduce per net (arena + 4-float tail), the supported form, what bench.py --gpus N and the drop-in use.
 * DQNHIP_DP_HALF_GRADS: the gradient arenas cross the links as bf16 — half the bytes (6.4 instead of 12.9 MB per
 * net at 4x1024); the [loss, q, flag] tails stay fp32 and travel once, with the actor's gradients.  The reduced
 * gradient then carries 8 significant bits (tests/test_gpu_dp_hip.py bounds the effect); meant for the fp16 learner.
 * cfg.use_graph: dqnhip_dp_update captures phase 0 / all-reduce / phase 1 / all-reduce / phase 2 ONCE and replays
 * it as a hipGraph (eager if RCCL refuses the capture: dqnhip_dp_graph_active tells).
 * Since round 6 a data-parallel learner runs the single learner's merged launches (dqnhip_get_update_plan): the riders sit
 * between the exchange points, the tails of the exchange ride in each net's last backward launch.
 * (Two further exchange forms exist behind DQNHIP_DP_UNVERIFIED_OK — see the end of this header.) */
#define DQNHIP_DP_ID_BYTES 128
#define DQNHIP_DP_PER_LAYER 1
#define DQNHIP_DP_HALF_GRADS 2
#define DQNHIP_DP_SHARD_OPT 4
#define DQNHIP_DP_UNVERIFIED_OK 256     /* lets DQNHIP_DP_PER_LAYER / DQNHIP_DP_SHARD_OPT through for dp_world > 1 (see the end of this header) */
/* ncclGetVersion() and the shared object RCCL was resolved from in this process (a PyTorch host process resolves torch's
 * bundled librccl, a bare host /opt/rocm's); dqnhip_dp_init cross-checks the version over the group and fails on a mix. */
int dqnhip_dp_info(int32_t* rccl_version, char* path, size_t path_bytes);
int dqnhip_dp_unique_id(void* id_out, size_t bytes);
int dqnhip_dp_init(dqnhip_handle h, const void* id, size_t bytes, int32_t flags);
int dqnhip_dp_init_file(dqnhip_handle h, const char* path, int32_t flags, int32_t timeout_s);
int dqnhip_dp_rendezvous_file(const char* path, int32_t rank, int32_t world, int32_t timeout_s, void* id, size_t bytes);
int dqnhip_dp_rendezvous_cleanup(const char* path, int32_t world);
int dqnhip_dp_graph_active(dqnhip_handle h, int32_t* active);
int dqnhip_dp_broadcast_params(dqnhip_handle h, int32_t root);
int dqnhip_dp_update(dqnhip_handle h, const int32_t* idx_host);
/* n of them with on-device sampling: dqnhip_update_async_n for a group (every rank calls it with the same n; sixteen
 * updates, collectives included, per hipGraph launch). */
int dqnhip_dp_update_n(dqnhip_handle h, int32_t n);
int dqnhip_dp_gather_state(dqnhip_handle h);
int dqnhip_dp_destroy(dqnhip_handle h);

/* Waits for the stream and returns the scalars of the last update.  Fails — the reference
 * aborts: CHECK(std::isfinite(target)) src/dqn.cpp:898, CHECK(std::isfinite(critic_loss)) :906 —
 * with "Target not finite!" / "Critic loss not finite!" if any update since the last call
 * (blocking, async, phased or graph-replayed alike: the flags are raised on the device and are
 * sticky until reported here) produced a non-finite TD target or loss, or if a clip+Adam step was
 * skipped because the gradient norm was not finite (fp16 overflow; weights are left untouched). */
int dqnhip_read_stats(dqnhip_handle h, float* critic_loss, float* avg_q);
/* Optimiser steps skipped so far because of a non-finite gradient norm (one count per net per update).
 * A skipped step still ends the update normally: the iteration counters, the soft-update schedule and
 * the sampling counter advance (as they would after Caffe's Step with a zero update); only w, m, v and
 * the targets are left untouched.  Under native data parallelism every rank takes the same decision (the
 * norm is that of the REDUCED gradient) and a rank-local "Target not finite!" is shared through the
 * all-reduced tail, so all ranks report the same error at the same update. */
int dqnhip_skipped_steps(dqnhip_handle h, int64_t* count);

/* Dynamic loss scaling (cfg.loss_scale_mode): the device's state, read behind everything enqueued so far
 * (stream-ordered, like dqnhip_skipped_steps).  A static learner reports mode 0, multipliers 1, counters 0. */
typedef struct dqnhip_loss_scale_state {
  int32_t struct_size;                       /* filled in by the library */
  int32_t mode;                              /* cfg.loss_scale_mode */
  float mult_critic, mult_actor;             /* the live multipliers */
  int32_t good_critic, good_actor;           /* finite steps in a row since the multiplier last moved */
  int32_t backoffs_critic, backoffs_actor;   /* halvings so far */
  int32_t growths_critic, growths_actor;     /* doublings so far */
  int32_t skipped_steps;                     /* dqnhip_skipped_steps */
  int32_t reserved;
} dqnhip_loss_scale_state;
int dqnhip_get_loss_scale(dqnhip_handle h, dqnhip_loss_scale_state* out);
/* Sets both multipliers (powers of two inside [loss_scale_min_mult, loss_scale_max_mult]) and zeroes both
 * finite-step counters; with loss_scale_growth_interval = 0 and no overflow they then stay put.  Waits for the
 * stream.  Refused on a static learner. */
int dqnhip_set_loss_scale(dqnhip_handle h, float mult_critic, float mult_actor);

/* Sum-reduce the gradient arenas (tails included) of n learners of one data-parallel group that
 * live on ONE device, in rank order, leaving the sum in each: the exchange step between
 * dqnhip_update_phase calls without a communicator (co-located agents; the one-GPU test of the
 * dp_world > 1 arithmetic).  Groups that span devices use dqnhip_dp_* (RCCL over xGMI). */
int dqnhip_reduce_gradients_local(dqnhip_handle* learners, int32_t n, int32_t net);

/* Replaces DQN::Benchmark (src/dqn.cpp:487-498): times `iterations` updates
 * (after `warmup` untimed ones) with HIP events on the learner's stream and
 * returns the average in milliseconds ("Average Update: X ms"). */
int dqnhip_benchmark(dqnhip_handle h, int32_t warmup, int32_t iterations,
                     float* avg_ms);

/* DQN::Benchmark as the reference's driver experiences it through the drop-in (src/dqn.cpp:487-498 loops over
 * UpdateActorCritic(): indices drawn on the host with std::mt19937 + uniform_int_distribution, :501-509, and a
 * blocking (critic_loss, avg_q) per update): wall-clock average over `iterations` calls of dqnhip_update
 * (pipelined = 0), dqnhip_update_pipelined (pipelined = 1) or dqnhip_update_chained with the next call's indices drawn one
 * call ahead (pipelined = 2: what the drop-in's UpdateActorCritic() does) after `warmup` untimed ones.  pipelined = 3: the
 * drop-in's -deferred_updates form of the same loop — the same draws, dqnhip_update_indexed_n every sixteen updates, one
 * dqnhip_collect_stats every 1000 updates and at the end. */
int dqnhip_benchmark_blocking(dqnhip_handle h, int32_t warmup, int32_t iterations, uint64_t seed,
                              int32_t pipelined, float* avg_ms);

/* Replaces the greedy branch of DQN::SelectActions -> SelectActionGreedily
 * (src/dqn.cpp:695-711, 734-766): actor forward on n states [n, S] (host),
 * returns [n, 10] ActorOutputs (host).  n is not capped at kMinibatchSize.
 * The epsilon draw and GetRandomActorOutput stay in the caller so the
 * reference's std::mt19937 call order is preserved (src/dqn.cpp:700). */
int dqnhip_select_actions(dqnhip_handle h, const float* states_host, int32_t n,
                          float* actor_out_host);
/* Same with states / outputs in HBM ([n,S] and [n,10], dense). */
int dqnhip_select_actions_device(dqnhip_handle h, const float* states_dev,
                                 int32_t n, float* actor_out_dev);
/* Target-actor variant (SelectActionGreedily(*actor_target_net_, ...)). */
int dqnhip_select_actions_net(dqnhip_handle h, int32_t net,
                              const float* states_host, int32_t n,
                              float* actor_out_host);

/* Replaces DQN::CriticForward / EvaluateAction (src/dqn.cpp:982-1020,
 * 688-693): Q(s, a) for n host rows using `net` (CRITIC or CRITIC_TARGET). */
int dqnhip_critic_forward(dqnhip_handle h, int32_t net, const float* states_host,
                          const float* actor_out_host, int32_t n, float* q_host);

/* Acting precision of an fp16 learner (no reference counterpart: the reference acts and trains with one
 * Caffe net, src/dqn.cpp:734-766 and :982-1020 run the nets :828-972 updates).  A runtime switch, per learner:
 *   DQNHIP_FP32 (default)  dqnhip_select_actions*, dqnhip_critic_forward and the greedy branch of
 *                          dqnhip_env_step run the exact-fp32 GEMMs on the fp32 master weights, with the
 *                          kernels and launch arguments they had before this switch existed;
 *   DQNHIP_FP16            the same entry points compute what the update's own forward passes compute:
 *                          inputs (states; [s | a | p] for a critic) rounded to fp16, round to nearest even;
 *                          every tower layer an fp16-MFMA GEMM on the net's fp16 weight mirror with fp32
 *                          accumulation, fp32 bias, leaky ReLU, stored as an fp16 panel; the heads fp32
 *                          weights on the fp16 tower top with fp32 accumulation.  The behaviour policy is
 *                          then the function mu(s) the update differentiates.  Inputs beyond the fp16
 *                          range (|x| > 65504 becomes +-Inf) are the caller's business.
 * DQNHIP_FP16 needs cfg.precision == DQNHIP_FP16 (refused otherwise).  The call launches nothing and does
 * not wait: an env handle notices the change at its next dqnhip_env_step and captures its step anew; the
 * learner's captured updates are untouched (the update path does not read the switch). */
int dqnhip_set_act_precision(dqnhip_handle h, int32_t precision);   /* DQNHIP_FP32 (default) | DQNHIP_FP16 */
int dqnhip_get_act_precision(dqnhip_handle h, int32_t* precision);

/* Replaces DQN::AddTransitions (src/dqn.cpp:775-781): FIFO-evicts while
 * size + n >= capacity, then appends n transitions.  terminal[i] != 0 means
 * next_state == boost::none (src/dqn.cpp:878); next_states rows of terminal
 * transitions are ignored. */
int dqnhip_add_transitions(dqnhip_handle h, const float* states, const float* actor_out,
                           const float* rewards, const float* on_policy_targets,
                           const float* next_states, const uint8_t* terminal, int32_t n);
/* Replaces DQN::AddTransition (src/dqn.cpp:768-773): evicts one iff size ==
 * capacity, then appends one. */
int dqnhip_add_transition(dqnhip_handle h, const float* state, const float* actor_out,
                          float reward, float on_policy_target,
                          const float* next_state, uint8_t terminal);
/* AddTransitions with all arrays already in HBM (batched env workers). */
int dqnhip_add_transitions_device(dqnhip_handle h, const float* states, const float* actor_out,
                                  const float* rewards, const float* on_policy_targets,
                                  const float* next_states, const uint8_t* terminal, int32_t n);

/* Replaces DQN::LabelTransitions (src/dqn.cpp:783-797) for one episode held in
 * host arrays: on_policy_target[last] = r[last]; [i] = r[i] + gamma*[i+1]
 * (gamma double, result rounded to float). */
int dqnhip_label_transitions(double gamma, const float* rewards, int32_t n,
                             float* on_policy_targets);

/* Replaces DQN::SampleStatesFromMemory (src/dqn.cpp:511-523): the states ([n,S], host) of n
 * transitions sampled uniformly with replacement.  idx_host: explicit logical indices (the
 * SampleTransitionsFromMemory part, src/dqn.cpp:501-509) or NULL = counter-based draw on the device. */
int dqnhip_sample_states(dqnhip_handle h, const int32_t* idx_host, int32_t n, float* states_host);
/* Replaces getActorOutput (src/dqn.cpp:719-732): the first batch_size rows [batch_size,10] of the
 * output blobs an actor's last minibatch forward left behind (ACTOR: mu(s) of the last update,
 * ACTOR_TARGET: mu'(s')). */
int dqnhip_get_actor_output(dqnhip_handle h, int32_t net, int32_t batch_size, float* actor_out_host);

/* DQN::memory_size / ClearReplayMemory (src/dqn.hpp:106,112). */
int dqnhip_memory_size(dqnhip_handle h, int32_t* size);
int dqnhip_clear_memory(dqnhip_handle h);
/* Read logical transitions [first, first+n) back to host arrays (for
 * DQN::SnapshotReplayMemory, src/dqn.cpp:1146-1178).  Any pointer may be NULL. */
int dqnhip_read_memory(dqnhip_handle h, int32_t first, int32_t n, float* states,
                       float* actor_out, float* rewards, float* on_policy_targets,
                       float* next_states, uint8_t* terminal);

/* Replaces DQN::SnapshotReplayMemory / LoadReplayMemory (src/dqn.cpp:1146-1226): the
 * reference's `.replaymemory` file — a gzip stream holding int32 num_transitions, then per
 * transition: state[S] floats, ActorOutput[10] floats, float reward, float on_policy_target,
 * 1-byte bool terminal (= next_state is none).  Next states are not stored: transition i's
 * next state is transition i+1's state when i is not terminal; a trailing non-terminal
 * transition loads as terminal (boost::none), exactly as in the reference.  Load clears the
 * memory first and does not evict (the reference resizes the deque to num_transitions);
 * it fails if num_transitions exceeds the capacity. */
int dqnhip_snapshot_replay_memory(dqnhip_handle h, const char* filename);
int dqnhip_load_replay_memory(dqnhip_handle h, const char* filename);

/* ---- parameters, iterations, targets ----------------------------------- */

/* number of learnable parameters of a net in the dense order above */
int dqnhip_param_count(dqnhip_handle h, int32_t net, size_t* count);
/* Copy a whole net's dense parameter vector out / in.  Used by Snapshot /
 * Restore / LoadWeights (src/dqn.cpp:525-557, 586-620).  kind M/V/G only for
 * ACTOR and CRITIC. */
int dqnhip_get_params(dqnhip_handle h, int32_t net, int32_t kind, float* host, size_t count);
int dqnhip_set_params(dqnhip_handle h, int32_t net, int32_t kind, const float* host, size_t count);
/* CloneNet (src/dqn.cpp:1022-1035): hard copy online -> target.
 * net = DQNHIP_ACTOR or DQNHIP_CRITIC (the source). */
int dqnhip_clone_to_target(dqnhip_handle h, int32_t net);
/* Solver::iter / set_iter (src/dqn.hpp:129-130, src/dqn.cpp:965). */
int dqnhip_get_iters(dqnhip_handle h, int32_t* actor_iter, int32_t* critic_iter);
int dqnhip_set_iters(dqnhip_handle h, int32_t actor_iter, int32_t critic_iter);

/* ---- multi-agent sharing (src/dqn.cpp:1036-1083; src/dqn_main.cpp:305-323) ------------
 * DQN::ShareParameters(other, n_actor, n_critic): the first n layers-with-blobs (Caffe layer
 * order: ip1..ipL, then the head layers) of `other`'s actor / critic AND of its two target nets
 * read and write `owner`'s storage from now on (Blob::ShareData — data only: gradients and
 * Adam history stay per learner, exactly the reference's Hogwild arrangement; both learners'
 * solvers and soft updates write the shared weights).  n may be 0..L (tower layers) or all
 * layers; splitting the actor's two heads is refused.  Both learners must be on one device
 * and of the same shape.  Calling again changes the layer counts; (0, 0) un-shares.
 * `owner` must outlive `other` (dqnhip_destroy(owner) fails while sharers exist). */
int dqnhip_share_parameters(dqnhip_handle owner, dqnhip_handle other, int32_t num_actor_layers,
                            int32_t num_critic_layers);
/* DQN::ShareReplayMemory(other) (src/dqn.cpp:1080-1082): `other` drops its own deque and uses
 * `owner`'s ring (capacity included) for AddTransition(s), sampling, memory_size, snapshot
 * and load.  Users of a shared ring on different streams are ordered in host-call order by
 * events; a private ring pays nothing. */
int dqnhip_share_replay_memory(dqnhip_handle owner, dqnhip_handle other);

/* The configuration the learner was created with (for clients that need the shapes). */
int dqnhip_get_config(dqnhip_handle h, dqnhip_config* out);

/* ---- Caffe snapshot layout (src/dqn.cpp:525-620; Caffe Solver::Snapshot/Restore) -------
 * `.caffemodel` = binary caffe.NetParameter{name=1, layer=100{name=1, type=2, blobs=7}},
 * `.solverstate` = binary caffe.SolverState{iter=1, learned_net=2, history=3, current_step=4},
 * blobs = caffe.BlobProto{shape=7{dim=1 packed}, data=5 packed float}.  Layer names are the
 * reference's: ip<i>_layer (src/dqn.cpp:406), action_layer, actionpara_layer (:426-427),
 * q_values_layer (src/dqn.hpp:43); weight blob [num_output, K] then bias [num_output]; Adam
 * history = [m of every param in order, then v of every param].
 * net = DQNHIP_ACTOR or DQNHIP_CRITIC. */
/* Net::ToProto + WriteProtoToBinaryFile */
int dqnhip_save_caffemodel(dqnhip_handle h, int32_t net, const char* filename);
/* Net::CopyTrainedLayersFrom (layers matched by NAME, others ignored) followed by CloneNet to
 * the target net — DQN::LoadActorWeights / LoadCriticWeights (src/dqn.cpp:525-539) */
int dqnhip_load_caffemodel(dqnhip_handle h, int32_t net, const char* filename);
/* Solver::Snapshot: writes <prefix>_iter_<iter>.caffemodel and .solverstate (learned_net =
 * the caffemodel's path), returns the iteration */
int dqnhip_solver_snapshot(dqnhip_handle h, int32_t net, const char* prefix, int32_t* iter_out);
/* Solver::Restore + CloneNet — DQN::RestoreActorSolver / RestoreCriticSolver (:541-557):
 * iteration, learned_net weights, Adam history; the target net becomes a hard copy */
int dqnhip_solver_restore(dqnhip_handle h, int32_t net, const char* solverstate);
/* DQN::Snapshot (src/dqn.cpp:586-620): both solvers under save_path, renamed to
 * snapshot_prefix, optional `<prefix>_iter_<max_iter>.replaymemory`, optional removal of
 * older snapshots of the same prefix */
int dqnhip_snapshot(dqnhip_handle h, const char* save_path, const char* snapshot_prefix,
                    int32_t remove_old, int32_t snapshot_memory);
/* ---- the same files, written behind training (opt-in) ---------------------------------------------------------------------------
 * dqnhip_snapshot_async writes the files dqnhip_snapshot would have written at this point of the learner's stream, under the same
 * names, without waiting for the stream: the four protobuf files byte for byte, the `.replaymemory` as one gzip member whose
 * decompressed bytes are the synchronous file's (its chunks are deflated independently by `compress_threads` threads, 0: 8; the
 * compressed size differs by a few bytes per MiB).  On the caller's thread: the checks and v1 refusals (a learner in a sharing
 * relationship, dp_world > 1 or a live communicator, a phased update in progress, kernel timing on), then the launches on the
 * learner's stream — actor / critic weights and histories into dense Caffe order plus a record of the iteration counters and the
 * ring's (head, size), the replay memory as the uncompressed stream (i32 n, n records of 4 S + 49 bytes in logical order), the
 * stream's CRC-32 for the gzip trailer — into a device staging buffer of the snapshot's own, and one event.  The learner's writer
 * thread, which it shares with dqnhip_save_state_async (jobs are taken first in first out, at most one of each kind in flight),
 * waits for the event on a stream of its own, builds the files and publishes each as <name>.tmp, fsync, rename — a killed process
 * leaves no partial file under a name dqnhip_find_latest_snapshot matches.  With remove_old the older files go only after all of
 * this snapshot's files are in place.  The file names carry the iteration counters of the image, not the host's at a later moment.
 * Whatever is enqueued after the call returns is not in the image.
 * A second dqnhip_snapshot_async, dqnhip_snapshot, dqnhip_solver_snapshot, dqnhip_snapshot_replay_memory, dqnhip_solver_restore,
 * dqnhip_load_caffemodel, dqnhip_load_replay_memory, dqnhip_load_state and dqnhip_destroy first join the one in flight; if it
 * failed, the joining call fails with its message (dqnhip_destroy still destroys and does not fail).
 * Cost: from the first asynchronous snapshot until dqnhip_destroy, device memory of the stream's upper bound for the capacity plus
 * the six dense parameter arrays (about 360 MB at 1 M transitions of 58 floats), and the writer's 16 MB of pinned host memory; while
 * a job runs, compress_threads x (1 MiB in + its deflate bound out) of host memory.  If the staging buffer cannot be allocated the
 * call fails and says so; dqnhip_snapshot needs none. */
int dqnhip_snapshot_async(dqnhip_handle h, const char* save_path, const char* snapshot_prefix, int32_t remove_old, int32_t snapshot_memory,
                          int32_t compress_threads);
int dqnhip_snapshot_wait(dqnhip_handle h, int32_t* actor_iter, int32_t* critic_iter);   /* joins; the job's status and the iterations its
                                                                                          files are named by (either may be NULL); 0 when none */
int dqnhip_snapshot_poll(dqnhip_handle h, int32_t* done);                               /* never blocks; *done = 1: nothing is in flight */
/* FindLatestSnapshot (src/dqn.cpp:122-144): newest <prefix>_{actor,critic}_iter_N.solverstate
 * and <prefix>_iter_N.replaymemory; each buffer receives "" when none is found */
int dqnhip_find_latest_snapshot(const char* snapshot_prefix, char* actor, char* critic, char* memory,
                                size_t buf_len);
/* FindHiScore (src/dqn.cpp:146-158) */
int dqnhip_find_hiscore(const char* snapshot_prefix, int32_t* score);
/* RemoveFilesMatchingRegexp (src/dqn.cpp:92-98) */
int dqnhip_remove_files_matching_regexp(const char* regexp);
/* FilesMatchingRegexp (src/dqn.hpp:213-216; src/dqn.cpp:559-580): regular files in the regexp's
 * directory whose file NAME matches its last path component; paths '\n'-separated (sorted) in
 * buf, their number in *count.  Fails if buf is too small. */
int dqnhip_files_matching_regexp(const char* regexp, char* buf, size_t buf_len, int32_t* count);
/* RemoveSnapshots (src/dqn.hpp:222-224; src/dqn.cpp:100-109): removes the matching files whose
 * iteration (the number between the last '_' and the last '.') is < min_iter. */
int dqnhip_remove_snapshots(const char* regexp, int32_t min_iter);

/* ---- introspection for parity tests ------------------------------------ */

/* Copy a named [B, *] intermediate of the last update to the host:
 * "q_target" [B] (Q'(s',mu'(s'))), "y" [B] (TD target), "q_train" [B],
 * "q_policy" [B], "actor_out" [B,10] (mu(s)), "dq_da" [B,10] (post
 * inverting-gradients), "idx" [B] (as float), "terminal" [B];
 * "indexed_graph_launches" [1]: the kernel nodes of the sixteen-update graph dqnhip_update_indexed_n has captured (0: none
 * captured, or dropped since - sharing, set-up of data parallelism); a buffer of 5 floats or more also gets those of the eight-,
 * four-, two- and one-update graphs in [1] .. [4].
 * "optimiser_launches" [3]: host counters of the optimiser launches this learner has enqueued or captured (the captures of
 * dqnhip_get_update_plan included): Adam's kernels (k_adam_soft*), k_solver_soft<>, k_solver_soft_gather<>.
 * What the head layers hand on, for per-element tests between the phases of dqnhip_update_phase:
 * "dq" [B]: Step(1)'s loss diff (q - y) / B, valid after phase 0;
 * "actor_target_out" [B,10]: mu'(s'), valid after phase 0;
 * "dz_c" / "dz_a" [B,H]: the critic's / actor's tower-top gradient (H = the last hidden width).  dz_c holds Step(1)'s after
 *   phase 0; phase 1 OVERWRITES it with the dq = -1 seed of the dQ/da pass (read Step(1)'s between the phases).  dz_a is
 *   written by phase 1.  The fp16 learner returns its fp16 panels widened to float as stored, i.e. still times the pass's
 *   loss scale (critic: loss_scale, seed: the dQ/da pass's, actor: the actor's);
 * "dxc" [B,10]: the action columns of the critic's first-layer input gradient, i.e. dQ/da BEFORE the inverting gradients,
 *   valid after phase 1.  Fails on a learner whose plan has DQNHIP_PLAN_DQDA_HEAD_BWD: that form keeps dQ/da in LDS and
 *   never writes the buffer (DQNHIP_TUNE_SEPARATE_ACTOR_HEAD_BWD restores it).
 * Nothing else in an update overwrites these before the phase that wrote them returns; after a whole update they hold what
 * phase 1 left (dz_c: the seed).
 * "w16_0" .. "w16_3" [dqnhip_param_count(net)]: fp16 learner only — the fp16 mirror of that net's weights (the copy the fp16
 *   GEMMs read; the optimiser pass writes it beside the fp32 master), as stored, widened to float, in dqnhip_get_params' dense
 *   order.  After any update or dqnhip_apply_update it equals (fp16)master element for element.
 * count = floats the caller's buffer holds; fails if too small. */
int dqnhip_debug_read(dqnhip_handle h, const char* name, float* host, size_t count);

/* The HIP stream (hipStream_t) the learner enqueues on. */
int dqnhip_get_stream(dqnhip_handle h, void** stream);
/* Average duration (ms) of the dominant kernel family over the launches since
 * the last call with reset != 0; measured with HIP events when profiling is
 * enabled via dqnhip_set_kernel_timing.  Used by bench.py's roofline leg. */
int dqnhip_set_kernel_timing(dqnhip_handle h, int32_t enable);
int dqnhip_get_kernel_timing(dqnhip_handle h, const char* family, float* avg_ms,
                             int64_t* launches, int32_t reset);

/* ---- update diagnostics (opt-in) ----------------------------------------------------------------------------------------
 * Replaces what Caffe's debug_info prints in the reference's debug builds (DQN::Initialize / CloneNet switch it on,
 * src/dqn.cpp:623-626, 632-635, 1027-1029): the magnitude of every top blob after a forward, of every parameter gradient after a
 * backward, of every parameter's data and update after the solver step.  ONE call reduces what the last update left on the
 * device — exactly the buffers dqnhip_get_params / dqnhip_debug_read / dqnhip_per_debug_read would return at that moment, whatever
 * update form ran last — to this fixed-size report, in three launches on the learner's stream (csrc/diag_kernels.hip.h: a
 * streaming pass over w, w', g, m, v of both online nets, the 5 x L activation panels and the [B] rows).  A learner that never
 * makes the call launches what it launched before the call existed; the call reads, and writes nothing but its own scratch
 * (allocated on first use, freed by dqnhip_destroy).  Stream-ordered, blocks.  Non-finite content is counted, never an error.
 * Every floating-point sum is a double accumulated in one fixed order (no floating-point atomics): two collections with nothing in
 * between return byte-identical reports.
 *
 * Moments of a set of elements x: count; n_zero (+-0); n_nonfinite (NaN, +-Inf); over the FINITE elements sum_abs = sum |x| and
 * sum_sq = sum x^2 in double (a float's square is exact in double) and max_abs (float; 0 when no element is finite).
 * Exponent histogram (64 bins) of the finite non-zero elements: e = the biased exponent field of the float32 bits (denormals:
 * e = 0), bin = min(max(e - 87, 0), 63) — bin k in 1..62 holds 2^(k-40) <= |x| < 2^(k-39), bin 0 everything below 2^-39, bin 63
 * everything from 2^23 up; sum of bins + n_zero + n_nonfinite = count.  Pad words of the internal layout are counted nowhere.
 *
 * Blobs: dense Caffe order of dqnhip_get_params — the actor's ip1 .. ipL, action_layer, actionpara_layer (2L + 4 blobs), then the
 * critic's ip1 .. ipL, q_values_layer (2L + 2), weight before bias.  `layer` = 0 .. L-1 for the tower, L (and L + 1: actionpara_layer)
 * for the heads.  Per blob: moments of w; of g as stored (DQNHIP_KIND_G: unscaled on every learner) with its histogram; of
 * lag = (double)w - (double)w' against the net's target (exact differences; max_abs rounded to float); of
 * step = s * (m / (sqrtf(v) + delta)) in float32, s = lr * adam_correction(beta1, beta2, t), t the net's iteration as it stands — the
 * value the last optimiser step subtracted from w, recomputed from the m, v it stored (Caffe's "[Update] .. diff"); 0 everywhere
 * while the iteration is 0.  After a SKIPPED step (non-finite gradient norm) it is the step the stored history implies, not one
 * that was taken.
 * Panels: pass p = 0 actor_target(s'), 1 actor(s), 2 critic_target, 3 critic(s, a), 4 critic(s, mu(s)), layer i = 1 .. L, the
 * stored post-ReLU values ("act<p>_<i>"; fp16 learner: each half widened exactly): moments, histogram, n_negative (elements < 0:
 * on the leaky branch), dead_units (columns < 0 in every row).
 * Rows: q_target, y, q_train, q_policy, td = q_train - y (float subtraction): min / max / sum / sum_sq over the finite elements
 * (min = max = 0 when none is), n_nonfinite; n_terminal; per actor-output column min / max / sum over the finite values and
 * n_out_of_bounds = values outside the inverting gradients' bounds ([-1, 1] for the 4 actions, [0, 100] for parameters 0 and 4,
 * [-180, 180] for the angles; src/dqn.cpp:927-957; a NaN is outside); sum_abs / max_abs of the finite dq_da.  Prioritized learner
 * (has_per): min / sum of the importance weights, min of prob, max of td_abs, over the finite values; else 0.
 * grad_norm[net] = sqrt(sum over the net's blobs of g.sum_sq), clip_scale[net] = clip_gradients >= 0 && norm > clip ? clip / norm : 1
 * (double, formed on the host from the report).  net index: DQNHIP_ACTOR, DQNHIP_CRITIC.
 *
 * v1 refuses: a phased update in progress; a learner that reads another learner's parameters (dqnhip_share_parameters: the arenas
 * it steps are not all its own — the owner is fine); a DQNHIP_DP_SHARD_OPT learner (m, v of foreign slices are stale). */
typedef struct dqnhip_diag_moments {
  int64_t count, n_zero, n_nonfinite;
  double sum_abs, sum_sq;
  float max_abs, reserved;
} dqnhip_diag_moments;
#define DQNHIP_DIAG_BINS 64
typedef struct dqnhip_diag_blob {
  int32_t net, layer, is_bias, reserved;
  dqnhip_diag_moments w, g, lag, step;
  int32_t g_hist[DQNHIP_DIAG_BINS];
} dqnhip_diag_blob;
typedef struct dqnhip_diag_panel {
  int32_t pass, layer, rows, cols;
  int64_t n_negative;
  int32_t dead_units, reserved;
  dqnhip_diag_moments a;
  int32_t hist[DQNHIP_DIAG_BINS];
} dqnhip_diag_panel;
typedef struct dqnhip_diag_row { float min, max; double sum, sum_sq; int64_t n_nonfinite; } dqnhip_diag_row;
typedef struct dqnhip_diag_action { float min, max; double sum; int64_t n_out_of_bounds; } dqnhip_diag_action;
#define DQNHIP_DIAG_MAX_BLOBS (2 * (2 * DQNHIP_MAX_HIDDEN + 4))
#define DQNHIP_DIAG_MAX_PANELS (5 * DQNHIP_MAX_HIDDEN)
typedef struct dqnhip_diag_report {
  int32_t struct_size;       /* in: sizeof(dqnhip_diag_report) */
  int32_t n_blobs, n_panels, has_per;
  dqnhip_diag_blob blobs[DQNHIP_DIAG_MAX_BLOBS];
  dqnhip_diag_panel panels[DQNHIP_DIAG_MAX_PANELS];     /* pass-major: panel (p, i) at p * L + i - 1 */
  dqnhip_diag_row q_target, y, q_train, q_policy, td;
  int64_t n_terminal;
  dqnhip_diag_action actor_out[DQNHIP_ACTOR_OUT];
  double dq_da_sum_abs;
  float dq_da_max_abs;
  float per_w_min;
  double per_w_sum;
  float per_prob_min, per_td_abs_max;
  int32_t actor_iter, critic_iter;
  float critic_loss, avg_q;                             /* the last update's pair, as dqnhip_read_stats returns it (no flag is read or cleared) */
  double grad_norm[2], clip_scale[2];
  int32_t fp16, loss_scale_mode;                        /* fp16 learner: the scales the histograms are read against, else 0 */
  float loss_scale_critic, loss_scale_dqda, loss_scale_actor;    /* the three static scales */
  float mult_critic, mult_actor;                        /* the live multipliers (1 in static mode) */
  int32_t reserved;
} dqnhip_diag_report;
int dqnhip_diag_collect(dqnhip_handle h, dqnhip_diag_report* out);

/* ---- data parallelism: exchange forms that are NOT part of the supported surface -----------------------------------------
 * Built in rounds 3-4, priced net-negative by this library's own model and never run on more than one rank (no box
 * with more than one GPU has been available): dqnhip_dp_init refuses them for dp_world > 1 unless DQNHIP_DP_UNVERIFIED_OK says the
 * caller knows.  One-rank groups stay open (tests pin their launch sequences).
 * DQNHIP_DP_PER_LAYER buckets each all-reduce per tower layer on a communication stream, started as soon as that layer's backward
 * launch has run (backward order), head + tail last (fp32 learner only).
 * DQNHIP_DP_SHARD_OPT: the optimiser sharded over the group (ZeRO-1 style) instead of replicated: per net, a reduce-scatter leaves
 * rank r with slice r of the summed gradient, the ranks all-reduce a 4-float tail {loss, q, target flag, sum of squares of their
 * slice} — the clip norm — each rank runs clip + Adam + soft update on its 1/N slice only, and the updated online AND target weights
 * (the targets move every update, src/dqn.cpp:967-970; fp16 learner: the fp16 mirrors too) are all-gathered.  m and v of foreign
 * slices go stale: dqnhip_dp_gather_state (collective) brings them back before a snapshot / dqnhip_get_params(KIND_M, KIND_V);
 * dqnhip_dp_destroy refuses until it has been called since the last update.  Combines with DQNHIP_DP_HALF_GRADS, not with
 * DQNHIP_DP_PER_LAYER; the arena must be divisible by 4 x dp_world.  dqnhip_apply_update_sharded pins its slice arithmetic on one GPU. */

/* ---- prioritized experience replay (opt-in) -------------------------------------------------------------------------------
 * No reference counterpart: the reference samples its deque uniformly (SampleTransitionsFromMemory, src/dqn.cpp:501-509), and so
 * does every learner that never calls dqnhip_per_enable — it launches exactly the kernels it launched before this section existed.
 * Proportional prioritization (Schaul et al. 2016): a transition is drawn with probability p^alpha / sum, the critic's loss is
 * corrected by the importance weight (pmin / prob)^beta (normalised by the minibatch's largest weight), and |TD error| + eps is written
 * back as the new priority.  All of it on the device: a radix-64 float32 sum tree over the ring's physical slots (a node = the sum
 * of its 64 children in one fixed order, always recomputed from them — csrc/per_kernels.hip.h has the definition), a stratified
 * sampler in front of every update, k_head_q_train_w in k_head_q_train's place, the write-back behind the update's last launch.  A
 * new transition gets p_max, the largest priority written so far (initially 1); FIFO eviction zeroes its slot's leaf.
 * `.replaymemory` files carry no priorities (a load gives every transition p_max); the learner-state file (dqnhip_save_state) does.
 * Schedule: fp32 learners take the DQNHIP_TUNE_SEPARATE_Q_TRAIN form; inside dqnhip_update_async_n's graphs the updates are the
 * stand-alone sequence back to back (no rider carries the next update's gather: its indices do not exist before this update's
 * write-back).  Explicit indices (dqnhip_update(h, idx, ...), dqnhip_update_async(h, idx)) skip the sampler: their slots and
 * probabilities are read from the tree, the rest is the same.
 * v1 refuses, on a prioritized learner: dqnhip_update_chained / _pipelined / _indexed_n / _phase, dqnhip_dp_init*, dp_world > 1,
 * dqnhip_share_replay_memory in either role (and enabling on a learner that already shares a ring).
 * The defaults are the customary values of the paper, NOT measured on this workload. */
typedef struct dqnhip_per_config {
  int32_t struct_size;       /* in: sizeof(dqnhip_per_config) */
  float alpha;               /* 0.6; 0: uniform */
  float beta0;               /* 0.4; the importance exponent at critic iteration 0 */
  int32_t beta_anneal_iters; /* 0: constant; else beta = min(1, beta0 + (1 - beta0) critic_iter / beta_anneal_iters), on the device */
  float eps;                 /* 1e-6 */
  uint64_t seed;             /* Philox key of the sampler */
} dqnhip_per_config;
void dqnhip_per_default_config(dqnhip_per_config* cfg);

/* Once per learner; freed by dqnhip_destroy; drops the captured update graphs; transitions already in the memory get p_max. */
int dqnhip_per_enable(dqnhip_handle h, const dqnhip_per_config* cfg);

typedef struct dqnhip_per_state {
  int32_t struct_size;       /* in: sizeof(dqnhip_per_state) */
  int32_t enabled;           /* 0: every other field is 0 */
  int32_t levels;            /* tree levels above the leaves */
  int32_t size;              /* transitions in the window the tree describes */
  float total, p_max, beta_now, reserved;
  uint64_t next_counter;     /* the Philox counter the next device-sampled update draws on */
  int64_t syncs;             /* k_per_sync launches so far */
} dqnhip_per_state;
/* Stream-ordered, blocks; brings the tree in step with the ring first. */
int dqnhip_per_get_state(dqnhip_handle h, dqnhip_per_state* out);

/* The leaves (p^alpha, as stored) of the logical range [first, first + n); syncs first. */
int dqnhip_per_get_priorities(dqnhip_handle h, int32_t first, int32_t n, float* leaf_host);
/* Finite, >= 0; stored as given; the nodes above are recomputed; raises p_max to the largest of them. */
int dqnhip_per_set_priorities(dqnhip_handle h, int32_t first, int32_t n, const float* leaf_host);

/* The sampler alone: n_batches minibatches on the counters counter .. counter + n_batches - 1, as logical indices
 * idx_host[n_batches][minibatch] and their probabilities prob_host (either may be NULL).  Touches neither the learner's counter
 * nor the tree; with counter = dqnhip_per_state.next_counter the first minibatch is what the next update draws. */
int dqnhip_per_sample(dqnhip_handle h, uint64_t counter, int32_t n_batches, int32_t* idx_host, float* prob_host);

/* "level<k>" (k = 0: the cap leaves by PHYSICAL slot; level k has ceil(cap / 64^k) nodes, the last one is the total), and of the
 * last update, [minibatch] each: "u", "slot", "prob", "w", "td_abs".  count: floats the buffer holds. */
int dqnhip_per_debug_read(dqnhip_handle h, const char* name, float* host, size_t count);

/* ---- n-step returns (opt-in) ----------------------------------------------------------------------------------------------------
 * No reference counterpart: the reference's off-policy target is one step, r + gamma Q'(s', mu'(s')) (src/dqn.cpp:892-900), and so is
 * that of every learner that never calls dqnhip_nstep_enable — it launches exactly the kernels it launched before this section
 * existed.  With n-step returns the off-policy target of a sampled transition t becomes
 *   sum_{k < m} gamma^k r_{t+k} + gamma^m Q'(s_{t+m}, mu'(s_{t+m}))
 * gathered on the device from the ring as it is (no new array).  For a sampled logical index li, ring size `size`, gamma = cfg.gamma:
 *   m     the smallest k in 1 .. n with terminal[li + k - 1] != 0, or li + k - 1 == size - 1, or k == n
 *   R     acc = r[li + m - 1]; for k = m - 2 .. 0: acc = (double)r[li + k] + gamma * acc; R = (float)acc   (double, no contraction)
 *   disc  d = gamma, then m - 1 times d = d * gamma                                                          (a double)
 *   b     li + m - 1: the next state and the terminal flag are those stored with b; state, action, on_policy_target, "idx": li's
 *   off   terminal ? R : (float)((double)R + disc * (double)q'), then the beta mix and everything after it as in the 1-step update
 * At n = 1 every bit is the 1-step learner's.  The window walks LOGICAL successors, so it relies on the invariant the
 * `.replaymemory` format relies on too: the logical successor of a non-terminal transition is the next step of its episode.  Every
 * path that fills the memory appends whole episodes contiguously (the caller's dqnhip_add_transitions of a labelled episode, the
 * env front-ends' flush, dqnhip_load_replay_memory, dqnhip_load_state); a caller that appends anything else — single transitions
 * from interleaved episodes — breaks it, and dqnhip_nstep_validate says so.  An episode whose head was evicted keeps a valid
 * suffix; a window never reads beyond the ring's last transition.
 * Schedule: what a prioritized learner runs — the stand-alone sequence per update (fp32: the DQNHIP_TUNE_SEPARATE_Q_TRAIN form, no
 * gather-ahead riders; inside dqnhip_update_async_n's graphs the sequences back to back), k_gather_n as its first launch and
 * k_head_q_train_n as its head launch.  Composes with prioritized replay (the sampler feeds the indices, |q - y_n| is written back),
 * both precisions, every solver and lr policy, shared replay memories and parameters, env front-ends, dqnhip_diag_collect.
 * v1 refuses, on an n-step learner: dqnhip_update_chained / _pipelined / _indexed_n / _phase, dqnhip_dp_init*, dp_world > 1,
 * dqnhip_evaluate_memory / dqnhip_per_refresh (the sweep forms 1-step targets).  The learner-state file does not hold n (a
 * hyper-parameter, not state): enable it again before dqnhip_load_state.  Typical n (3 - 5) is the literature's value (D4PG,
 * Rainbow), NOT measured on this workload. */
#define DQNHIP_NSTEP_MAX 64
/* n in [1, DQNHIP_NSTEP_MAX]; may be called again with another n; drops the captured update graphs; there is no disable. */
int dqnhip_nstep_enable(dqnhip_handle h, int32_t n);
/* *n = 0 if n-step returns were never enabled on this learner. */
int dqnhip_nstep_get(dqnhip_handle h, int32_t* n);
/* Of the last update, [minibatch] each: "reward" (R) and "steps" (m, as floats the way dqnhip_debug_read serves "idx").  The
 * discount is a double and has an entry point of its own: dqnhip_nstep_debug_read_f64 serves "disc".  count: elements the buffer
 * holds.  The window's terminal flag and "idx" are dqnhip_debug_read's "terminal" and "idx". */
int dqnhip_nstep_debug_read(dqnhip_handle h, const char* name, float* host, size_t count);
int dqnhip_nstep_debug_read_f64(dqnhip_handle h, const char* name, double* host, size_t count);
/* The invariant above over the logical range [first, first + n) (n = -1: to the end): *violations = the non-terminal transitions
 * whose stored next state differs, bitwise over state_size floats, from the state of their logical successor (the memory's last
 * transition is exempt), *first_bad = the smallest such logical index, -1 when there is none.  Any learner may validate, n-step or
 * not.  Stream-ordered, blocks. */
int dqnhip_nstep_validate(dqnhip_handle h, int32_t first, int32_t n, int64_t* violations, int32_t* first_bad);

/* ---- replay sweep: the nets evaluated over the stored memory (opt-in) ------------------------------------------------------------
 * No reference counterpart: the reference's -learn_offline only logs the smoothed loss of the minibatches it happened to draw.
 * dqnhip_evaluate_memory runs the update's forward passes — no backward, no optimiser step — over the logical transitions
 * [first, first + n) (as dqnhip_read_memory counts them; n = -1: from first to the end of the memory; n = 0: a no-op — nothing is
 * allocated, launched or captured — whose report is valid: all zero but for the iteration counters) in chunks of `minibatch` consecutive transitions, and reduces, per transition, with the nets as they stand:
 *   q            Q(s, a_stored) of the online critic
 *   y            the TD target exactly as the update forms it (src/dqn.cpp:892-900): terminal mask, gamma, the beta mix with
 *                on_policy_target, the target nets
 *   td           q - y, one float32 subtraction (dqnhip_diag_collect's definition)
 *   q_policy     Q(s, mu(s)) of the online critic as it stands (the update evaluates it on the critic it has just stepped)
 *   mc, reward   the stored on_policy_target and reward
 *   q_minus_mc   q - mc, one float32 subtraction
 *   action_match GetAction (TACKLE masked, the first maximum wins) gives the same index on mu(s) and on the stored actor output
 * Each dqnhip_diag_row holds min, max, sum, sum_sq over the FINITE values and n_nonfinite (no finite value: min = max = 0); td_hist is
 * the exponent histogram of td by dqnhip_diag_collect's bin rule (finite, non-zero values).  Every double sum is formed in one fixed
 * order without floating-point atomics (csrc/sweep_kernels.hip.h): two sweeps with nothing in between return byte-identical reports,
 * with and without use_graph.  The last chunk is padded with the window's last index; pad rows are counted nowhere.
 * rows (may be NULL; so may each pointer in it): host arrays of n elements, one per transition of the window.
 * A sweep overwrites the update's per-minibatch scratch: the gathered minibatch (input panels, reward / mc / terminal, "idx"), the
 * activation panels, the [minibatch] row buffers q_target / y / q_train / q_policy / dq / actor_out / actor_target_out and the loss
 * partials (what dqnhip_debug_read and dqnhip_diag_collect read: collect diagnostics of an update BEFORE sweeping); a refresh also
 * the sampler's "slot", "prob" and "td_abs" (dqnhip_per_debug_read).  It ends a dqnhip_update_chained chain as any other update call
 * does, and keeps 20 bytes of device memory per slot of the ring's capacity from the first sweep on.  It leaves
 * everything else as it was: weights, solver histories, target nets, iteration counters, the sampling counters, the replay memory, the
 * sticky flags, the (critic_loss, avg_q) pair and uncollected stats of dqnhip_update_indexed_n.
 * Blocks until the report is there.  An out-of-range window is refused and nothing runs.
 * v1 refuses: a phased update in progress; dp_world > 1 or a learner after dqnhip_dp_init*; precision = DQNHIP_FP16.  Learners that
 * share parameters or a replay memory may evaluate.
 *
 * dqnhip_per_refresh: the same sweep on a prioritized learner (dqnhip_per_enable), and per chunk the update's own write-back: the
 * leaf of every transition of the window becomes (|td| + eps)^alpha; a non-finite td leaves the old leaf; p_max is only ever raised;
 * the nodes above are recomputed.  The remedy for a `.replaymemory` load, which gives every transition p_max.  out may be NULL. */
typedef struct dqnhip_sweep_report {
  int32_t struct_size;       /* in: sizeof(dqnhip_sweep_report) */
  int32_t first, n, n_chunks;
  int64_t n_terminal, n_action_match;
  dqnhip_diag_row q, y, td, q_policy, mc, q_minus_mc, reward;
  int32_t td_hist[DQNHIP_DIAG_BINS];
  int32_t actor_iter, critic_iter;
} dqnhip_sweep_report;
typedef struct dqnhip_sweep_rows {
  int32_t struct_size;       /* in: sizeof(dqnhip_sweep_rows) */
  float *q, *y, *td, *q_policy;
  int32_t* action_match;
} dqnhip_sweep_rows;
int dqnhip_evaluate_memory(dqnhip_handle h, int32_t first, int32_t n, dqnhip_sweep_report* out, const dqnhip_sweep_rows* rows);
int dqnhip_per_refresh(dqnhip_handle h, int32_t first, int32_t n, dqnhip_sweep_report* out);

/* ---- native learner-state file: exact resume (opt-in) -------------------------------------------------------------------------
 * No reference counterpart: the reference resumes from its three snapshot files (src/dqn_main.cpp:213-220, 268-286), which cannot
 * hold what this learner keeps on the device beside the weights — the target nets (Restore re-clones them), the sampling
 * counters, the loss-scale multipliers, the ring's physical position, the priority tree.  One file, written and read by the
 * two calls below, holds all of it, with one guarantee: save, destroy, create, load, continue computes bit for bit what the
 * learner would have computed had it never stopped.  A learner that never calls them does what it did; the reference's files are
 * written and read as before.  Byte layout: DESIGN.md 9 (tests/state_ref.py reads and writes it from that description alone).
 *
 * dqnhip_save_state waits for the learner's stream, brings a priority tree in step with the ring, writes filename + ".tmp" and
 * renames it over filename (a job killed mid-write never leaves a truncated latest file; a failed save leaves an existing file
 * alone).  Saved: the four nets' weights and m / v of the two online nets (dense Caffe order); both iterations, the sampling
 * counter, the last (critic_loss, avg_q), the sticky flags as they are, skipped_steps, the loss-scale state of a dynamic learner;
 * the dqnhip_sample_states call count and cfg.seed; unless DQNHIP_STATE_NO_MEMORY: (ring_head, ring_size) and the window's
 * transitions in logical order and, on a prioritized learner, dqnhip_per_config, p_max, the sync count and the window's leaves;
 * the caller's opaque `user` bytes.  NOT saved: gradient arenas, the last update's intermediates (dqnhip_debug_read,
 * dqnhip_get_actor_output), uncollected dqnhip_collect_stats pairs, the pipelined lag slot, the acting precision (a runtime
 * switch), env front-end handles (their open episodes are lost, as the reference loses a half-played episode).
 *
 * dqnhip_load_state reads and validates the WHOLE file before it touches the learner: any failure leaves the learner bit for bit
 * as it was, and the message names the file and what failed.  In this order: magic, version, header CRC; the table's CRC, the
 * section bounds, every section's CRC; state_size and hidden[] equal the learner's; with a memory in the file: replay_capacity
 * equal, prioritized on both sides or on neither, alpha equal (the leaves are p^alpha).  minibatch and precision may differ (the
 * master weights are fp32 either way); a loss-scale section is applied to a dynamic learner only, its multipliers must lie inside
 * the learner's [loss_scale_min_mult, loss_scale_max_mult].  Then: the arenas are filled (the fp16 mirrors become dirty), the
 * counters and flags restored, cfg.seed adopted (dqnhip_get_config reports the file's), logical transition i placed at physical
 * slot (ring_head + i) % capacity, the tree restored to the saved learner's bits at every level (a prioritized learner also adopts
 * the file's beta0, beta_anneal_iters, eps and sampler seed), captured graphs dropped.
 *
 * Solver: a learner whose solver is not Adam writes a 16-byte SOLV section (solver_type, rms_decay) behind the history sections, an
 * Adam learner writes none (its file is what it was before the other solvers existed); dqnhip_load_state refuses a file whose solver
 * is not the learner's, in either direction, before it touches the learner.  ADM<net> / ADV<net> carry history 1 / history 2.
 * Schedule: a learner with an lr policy or a weight decay writes a 104-byte LRSC section (the schedule's words, the decay, its kind)
 * behind them, by the same rules: a learner with neither writes the file it always wrote, and a load refuses any difference.
 *
 * v1 refuses, in both calls: a learner in any sharing relationship (parameters or replay memory, either role), dp_world > 1 or a
 * live communicator, a phased update in progress, kernel timing on.  Env front-end handles attached to a learner that loads see
 * what they see after dqnhip_load_replay_memory: the ring changed under them, their open episodes continue on it. */
#define DQNHIP_STATE_NO_MEMORY 1   /* neither the replay memory nor (head,size) nor the priority tree are written / touched on load */
int dqnhip_save_state(dqnhip_handle h, const char* filename, int32_t flags,
                      const void* user, size_t user_bytes);          /* user: an opaque caller section (may be NULL / 0) */
int dqnhip_load_state(dqnhip_handle h, const char* filename);
/* host only, needs no GPU */
typedef struct dqnhip_state_info {
  int32_t struct_size;       /* in: sizeof(dqnhip_state_info_t) (or its size before solver_type / rms_decay were appended: that much is filled) */
  int32_t version, flags, precision, minibatch, state_size, num_hidden, hidden[DQNHIP_MAX_HIDDEN], replay_capacity, memory_size,
      actor_iter, critic_iter, has_memory, has_per, has_loss_scale;
  uint64_t seed, update_counter, user_bytes, file_bytes;
  int32_t solver_type;       /* DQNHIP_SOLVER_* of the learner that wrote the file (0 = Adam: a file without a SOLV section) */
  float rms_decay;           /* ... and its rms_decay (0 in an Adam learner's file: it is not stored there) */
} dqnhip_state_info_t;       /* (the type carries _t: in C a typedef and a function cannot share a name) */
/* Validates the whole file (every CRC) as dqnhip_load_state does, and reports the header. */
int dqnhip_state_info(const char* filename, dqnhip_state_info_t* out);
/* The caller's section: *n_out = its length (0: none); fails if it exceeds cap. */
int dqnhip_state_read_user(const char* filename, void* buf, size_t cap, size_t* n_out);

/* ---- the same file, written behind training (opt-in) ---------------------------------------------------------------------------
 * dqnhip_save_state_async writes, byte for byte, the file dqnhip_save_state would have written at this point of the learner's
 * stream, without waiting for the stream.  On the caller's thread: the argument checks and v1 refusals of dqnhip_save_state
 * (reported by this call), the tree brought in step with the ring, then three launches on the learner's stream — the parameters
 * into dense Caffe order plus a record of the DevState fields, the ring's window in logical order ((ring_head, ring_size) are read
 * on the device), zlib's CRC-32 of every section in 1 KB chunks (csrc/state_kernels.hip.h) — into a device staging buffer, and
 * an event.  `user` and the host-side values are copied; the call returns.  A writer thread (one per learner) waits for the
 * event, folds the chunk CRCs, and streams the staging buffer through two pinned 8 MB chunks to filename + ".tmp", then renames.
 * Whatever is enqueued after the call returns — updates, appends, acting, env steps, parameter writes, snapshots — is not in the
 * image.  Not part of it: the host-side conveniences of the synchronous call (harvesting indexed updates, refreshing the host's
 * (head, size) mirror).
 * One save is in flight per learner: a second dqnhip_save_state_async, dqnhip_save_state, dqnhip_load_state and dqnhip_destroy
 * first join it; if it failed, the joining call fails with its message (dqnhip_destroy still destroys and does not fail).
 * Cost: from the first asynchronous save until dqnhip_destroy, device memory of the file's upper bound for this learner (the
 * staging buffer) and 16 MB of pinned host memory.  If the staging buffer cannot be allocated the call fails and says so;
 * dqnhip_save_state needs none. */
int dqnhip_save_state_async(dqnhip_handle h, const char* filename, int32_t flags, const void* user, size_t user_bytes);
int dqnhip_save_state_wait(dqnhip_handle h);                 /* joins; the save's status; 0 when none is in flight */
int dqnhip_save_state_poll(dqnhip_handle h, int32_t* done);  /* never blocks; *done = 1: nothing is in flight */
/* The save's checksum path on caller-supplied bytes: host_bytes are copied into device scratch `misalign` bytes (0 ... 15) past
 * a 16-byte boundary, the chunk kernel and the combine step of the asynchronous save run, *crc = zlib's crc32 of the bytes.
 * Stream-ordered, blocks.  For tests, and for anyone who wants to verify a buffer. */
int dqnhip_state_crc32_device(dqnhip_handle h, const void* host_bytes, size_t bytes, int32_t misalign, uint32_t* crc);

/* ---- action noise on the device: exploration (env handles), target policy smoothing (learner) ---------------------------------
 * Gaussian noise added to an ActorOutput row inside the kernels that form it.  Both uses are OPT-IN: a learner or env handle that
 * never enables them launches exactly the kernels it launched before.  One noise body (csrc/noise_bodies.hip.h, one text for host
 * and device) and one counter-based generator (the Philox-4x32-10 of the sampler):
 *     standard normal z of the key (seed, ctr, lane0): x1, x2 = the generator's words at lanes lane0, lane0 + 1;
 *         u1 = ((x1 >> 8) + 1) 2^-24 in (0, 1], u2 = (x2 >> 8) 2^-24 in [0, 1);
 *         z = (float)(sqrt(-2 log u1) cos(6.283185307179586 u2)), evaluated in double and rounded once; |z| <= 5.77
 *     column scale: range_j = max - min of ActorOutput column j's bounds (the inverting gradients' table): 2 for the four action
 *         logits, 100 for the two powers, 360 for the four angles.  sigma_j = sigma_logits for j < 4, sigma_params from there.
 *         sigma_logits, sigma_params and clip are in UNITS OF THE COLUMN'S RANGE.
 *     everything after the draw is one separately rounded float32 operation per step (no fma).
 * Exploration (dqnhip_env_set_noise, dqnhip_env.h): an Ornstein-Uhlenbeck state per worker and column,
 *         x <- (x - theta x) + sigma_j z,      greedy value v' = v + range_j x,      clamp: min(max(v', min_j), max_j)
 *     with z keyed by (noise seed, the worker's draw counter at the step's start, worker 32 + 2 j).  theta = 1 is white Gaussian
 *     noise.  x is zero at creation and after every episode end, and advances on every step whether or not epsilon chose the
 *     random ActorOutput, which stays un-noised.
 * The defaults are the literature's values rescaled to units of the range and NOT MEASURED ON THIS WORKLOAD:
 *     DQNHIP_NOISE_EXPLORE: theta 0.15, sigma_params 0.1 (the OU parameters of Lillicrap et al. 2016 are theta 0.15, sigma 0.2 on
 *         actions in [-1, 1], a range of 2), sigma_logits 0 (the discrete choice is explored by epsilon), clip 0 (unused), clamp on;
 *     DQNHIP_NOISE_TARGET: theta 1, sigma_logits = sigma_params = 0.1, clip 0.25 (TD3's sigma 0.2 and clip 0.5 on a range of 2),
 *         clamp on.
 * Refused, by message: a sigma that is negative or not finite, theta outside (0, 1], a negative clip, a struct_size mismatch.
 * Target policy smoothing (TD3, Fujimoto et al. 2018; dqnhip_target_noise_enable; cfg NULL switches it off):
 *         y = r + gamma Q'(s', a~),   a~_j = clamp(mu'(s')_j + range_j t_j),   t_j = sigma_j z, clipped to [-clip, clip] if clip > 0
 *     for row r and column j of the update whose sampling counter is c (DevState's update counter: consecutive updates, also the
 *     sixteen of one dqnhip_update_async_n graph, use consecutive c), z keyed by (noise seed, c, r 32 + 2 j).  a~ replaces mu'(s') as
 *     the critic-target's action input and nowhere else: dqnhip_debug_read "actor_target_out" keeps the clean mu'(s'),
 *     "actor_target_smoothed" [B,10] is a~, "target_noise_z" [B,10] the z used, "target_noise_counter" [2] c as (c mod 2^24, c / 2^24).
 *     One launch more per update (k_target_smooth, between the actors' heads and the critics' first layers), on the schedule of
 *     DQNHIP_TUNE_SEPARATE_CRITIC_FIRST_LAYERS (DQNHIP_PLAN_TARGET_SMOOTHING).  It composes with prioritized replay, n-step returns,
 *     every solver and lr policy and dqnhip_update_async_n.  theta must be 1.  Refused in this version, each by a message naming target
 *     smoothing: precision = DQNHIP_FP16; dqnhip_update_chained / _pipelined / _indexed_n / _phase; data parallelism; parameter and
 *     replay sharing.  The replay sweep (dqnhip_evaluate_memory, dqnhip_per_refresh) keeps evaluating the CLEAN target.  The
 *     learner-state file is unchanged (the noise is a hyper-parameter plus the saved update counter): enable it again before
 *     dqnhip_load_state.  Twin critics and delayed policy updates, TD3's other two ingredients, are not built. */
#define DQNHIP_NOISE_EXPLORE 0
#define DQNHIP_NOISE_TARGET 1
typedef struct dqnhip_noise_config {
  int32_t struct_size;   /* = sizeof(dqnhip_noise_config) */
  int32_t clamp;         /* non-zero: clamp the noisy value to the column's bounds */
  float sigma_logits, sigma_params, theta, clip;
  uint64_t seed;         /* key of the noise draws (not the env's or the sampler's seed) */
} dqnhip_noise_config;
int dqnhip_noise_default_config(dqnhip_noise_config* cfg, int32_t purpose);
/* The exploration step of ONE row on the host — the text the env kernels evaluate, compiled for the host — for a caller that
 * selects its actions one state at a time (dqn_dropin.cpp's SelectAction): draws the ten normals of the key (cfg->seed, counter,
 * row 32 + 2 j), advances ou_state[10] and puts it on actor_out[10] in place.  No device is touched. */
int dqnhip_target_noise_enable(dqnhip_handle h, const dqnhip_noise_config* cfg);
int dqnhip_target_noise_get(dqnhip_handle h, int32_t* enabled, dqnhip_noise_config* cfg);   /* cfg may be NULL */
int dqnhip_noise_explore_host(const dqnhip_noise_config* cfg, uint64_t counter, int32_t row, float* ou_state, float* actor_out);

/* ---- batched env front-end (HFOGameState reward shaping, N workers) ----- */

/* Replaces HFOGameState::update + reward (src/hfo_game.cpp:122-236) for n
 * synthetic workers whose state vectors are in HBM: see dqnhip_env.h. */

#ifdef __cplusplus
}
#endif
#endif /* DQNHIP_H_ */
