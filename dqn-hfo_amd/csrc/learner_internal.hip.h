// learner_internal.hip.h — what the translation units of libdqnhip.so share: the learner object behind dqnhip_handle, the
// parameter-arena layout, the error convention, and the prototypes of the host-side building blocks.
//   learner.hip         what an update launches: the forward / backward / optimiser building blocks and the three phases of the
//                       fp32 and fp16 schedules (run_phase), dqnhip_apply_update*.  Every kernel of the update is launched — and
//                       has its launch attributes set (prepare_kernels) — from this unit
//   learner_plan.hip    the error channel, parameter layout, config validation, shape predicates, the plan (plan_of); host only
//   learner_create.hip  learner lifetime: dqnhip_create / dqnhip_destroy, staging buffers, drop_graphs; host only
//   learner_update.hip  index staging, graph capture (capture_updates), dqnhip_update* / dqnhip_get_update_plan / dqnhip_read_stats,
//                       the in-library benchmark loops; host only
//   learner_dp.hip      native data parallelism: RCCL inside the library, the file rendezvous (dqnhip_dp_*)
//   learner_io.hip      acting, replay memory (+ .replaymemory files, dqnhip_nstep_validate), parameters, multi-agent sharing,
//                       iterations / learning rate, dqnhip_debug_read, stream and kernel timing (head_fwd_kernels.hip.h, io_kernels.hip.h)
//   learner_per.hip     prioritized replay: the per_* launchers the other units call and dqnhip_per_* (per_kernels.hip.h)
//   learner_eval.hip    update diagnostics (dqnhip_diag_collect: diag_kernels.hip.h) and the replay sweep (dqnhip_evaluate_memory /
//                       dqnhip_per_refresh: sweep_kernels.hip.h; its forward launches are sweep_forward's, learner.hip)
//   learner_features.hip  n-step returns (dqnhip_nstep_*) and target smoothing (dqnhip_target_noise_*), whose kernels learner.hip
//                       launches, and feature_refuse: the one place a call refuses a learner for an opt-in feature; host only
//   learner_env.hip     host side of the batched env front-end (include/dqnhip_env.h)
//   learner_state.hip   the native learner-state file: dqnhip_save_state / dqnhip_load_state; host only
//   learner_save_async.hip  dqnhip_save_state_async and dqnhip_snapshot_async: their pack and checksum launches (state_kernels.hip.h,
//                       snapshot_kernels.hip.h), the writer thread they share and each one's staging buffer and job.
//                       learner_state.hip.h: what the two units above share
//   snapshot.cpp        Caffe snapshot layout (no device code); snapshot_codec.h: its builders on host pointers, for the writer thread
//   state_codec.cpp     the learner-state file's container (header, table, CRCs) and its manifest (the order of the sections),
//                       dqnhip_state_info / _read_user (no device code, no HIP)
//   gzip_parallel.cpp   one gzip member from chunks deflated by a pool of threads: the asynchronous snapshot's .replaymemory (no HIP)
// This header includes the ARGUMENT layer only (learner_args.hip.h has the map of the kernel headers): a unit includes the headers
// of the kernels it launches and embeds exactly those (tests/test_kernel_inventory.py), the host-only units embed no device code.
// A launch attribute (hipFuncSetAttribute) of a kernel with internal linkage holds for the calling unit's copy only: it is set in
// the unit that launches the kernel.
// Not installed, not part of the C-ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <zlib.h>
#include <unistd.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <random>
#include <string>
#include <vector>
#include <mutex>
#include <chrono>
#include <thread>

#include "../../include/dqnhip.h"
#include "../../include/dqnhip_env.h"
#include "gemm_common.hip.h"      // LaunchOn, launch, TailsArgs, the flags
#include "learner_args.hip.h"
#include "noise_bodies.hip.h"     // NoiseCfg and the host side of the noise body (no kernel)
#include "gemm_plan.hip.h"        // the fp32 forms and their choosers (bwd_layer_is_pair)
#include "hgemm_plan.hip.h"

namespace dqnhip_host {
using namespace dqnhip;

extern thread_local std::string g_err;      // defined in learner_plan.hip; dqnhip_last_error() returns it

inline int fail(const char* fmt, ...) {
  char buf[1024];
  va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
  g_err = buf;
  return 1;
}

#define HIPCHK(expr)                                                                  \
  do {                                                                                \
    hipError_t e__ = (expr);                                                          \
    if (e__ != hipSuccess)                                                            \
      return fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
  } while (0)
#define RC(expr) do { int rc__ = (expr); if (rc__) return rc__; } while (0)

inline int round_up(int x, int m) { return (x + m - 1) / m * m; }
inline size_t round_up_z(size_t x, size_t m) { return (x + m - 1) / m * m; }

constexpr int kMaxL = DQNHIP_MAX_HIDDEN;
// dqnhip_update_indexed_n: host-mapped index / stats banks, one multi-update graph in flight per bank (see learner_update.hip), and
// the graph sizes an n is cut into (16 / 8 / 4 / 2 / 1, as dqnhip_update_async_n cuts it)
constexpr int kIxBanks = 2;
constexpr int kIxSizes = 5;
// fp16 learner: ALL wgrads of a net in one launch of 128x128 tiles from this many minibatch rows (the reduction
// length); below, the per-layer form (a layer's dgrad + wgrad sharing a launch of 64x64 split-K tiles) is as fast or
// faster (measured at 256 / 512 / 1024 / 2048 / 4096 rows: +0.7 / -6 / -28 / -37 / -68 us per update)
constexpr int kGroupMinRows = 512;

// Internal parameter arena of one net: tower layer l has W_l[dims[l+1]][kp[l]] (K
// padded to a multiple of 64 so every GEMM tile is whole) and b_l[dims[l+1]];
// the head(s) are stored as one [NH][H] matrix (action_layer rows 0-3,
// actionpara_layer rows 4-9: the Split layer disappears) and bh[16].
struct NetLayout {
  int L = 0, in_dim = 0, NH = 0;
  int dims[kMaxL + 1] = {0};   // logical widths: dims[0] = in_dim
  int kp[kMaxL + 1] = {0};     // padded widths of each activation panel
  size_t w_off[kMaxL] = {0}, b_off[kMaxL] = {0}, hw_off = 0, hb_off = 0;
  size_t arena = 0;            // floats, multiple of 64
  size_t dense = 0;            // dense (Caffe-order) parameter count
  // sum-of-squares partial slots
  int part_off[kMaxL + 1] = {0};  // per tower layer, then head
  int part_db = 0;                // fp16 learner: first slot of the bias-gradient workgroups
  int n_part = 0;
};

void layout_init(NetLayout& l, int in_dim, const dqnhip_config& c, bool actor);

// the kernel families of timing mode (dqnhip_get_kernel_timing), named by kFamily[] (learner.hip)
enum Family { kFamFwdLds4x2, kFamDgrad, kFamWgrad, kFamAdam, kFamBwdPair, kFamFwdLds2x2, kFamFwdDirect, kFamHgemmFwd, kFamHgemmDgrad, kFamHgemmWgrad,
              kFamPerSync, kFamPerSample, kFamPerUpdate, kNumFamily };
extern const char* const kFamily[kNumFamily];
struct TimingRec { Family family; hipEvent_t a, b; };

// the captured launch sequences a single learner replays (dqnhip_learner::graph_exec)
enum GraphSlot {
  kGraphSampled,      // one update, indices sampled on the device
  kGraphExplicit,     // one update, explicit indices (the pinned buffer)
  kGraphPipe0,        // dqnhip_update_pipelined: explicit indices in pipeline slot 0 ...
  kGraphPipe1,        // ... and slot 1
  kGraphMulti,        // kMultiU device-sampled updates (dqnhip_update_async_n)
  kGraphChainHead,    // dqnhip_update_chained: head of a chain (own gather, parity 0) ...
  kGraphChainPar1,    // ... continued at panel parity 1 ...
  kGraphChainPar0,    // ... and at parity 0
  kNumGraphSlots
};

// Prioritized replay (dqnhip_per_enable; the kernels and the tree's definition: per_kernels.hip.h).  Owned by the learner that owns the
// ring; a prioritized learner shares no ring (v1), so that is the learner itself.
struct PerTreeHost { float* lvl[8] = {nullptr}; int n[8] = {0}; int levels = 0; };      // PerTree's members (per_kernels.hip.h: device code)
struct PerHost {
  dqnhip_per_config cfg{};
  PerTreeHost tree; float* tree_base = nullptr; size_t tree_floats = 0;
  void* dev = nullptr;                  // PerDev
  int* idx = nullptr; int* slot = nullptr;          // [B]: the sampler's logical indices (what the gather reads) and physical slots
  float *prob = nullptr, *u = nullptr, *w = nullptr, *td_abs = nullptr;   // [B]
  // the host's upper bound on the transitions appended since the last k_per_sync, and whether the ring may have changed at all
  long long pending = 0; bool changed = false;
  long long syncs = 0;                  // k_per_sync launches so far
};
// n-step returns (dqnhip_nstep_enable; k_gather_n, k_head_q_train_n).  Owned by the learner that enabled it, whoever owns the ring.
struct NstepHost {
  int n = 1;                            // 1 .. kNstepMax
  double* disc = nullptr; int* steps = nullptr;     // [B]: gamma^m and m of the last update's rows (the gathered reward buffer holds R)
  unsigned long long* viol = nullptr;   // dqnhip_nstep_validate's two result words: {violations, first_bad (an int in the second word)}
};
// target policy smoothing (dqnhip_target_noise_enable; k_target_smooth, head_kernels.hip.h)
struct TargetNoiseHost {
  dqnhip::NoiseCfg cfg{};
  float* smoothed16 = nullptr; float* z16 = nullptr;   // [B][kAP]: a~ and the z of the last update
  unsigned long long* counter = nullptr;               // [1] the Philox counter the last update's noise was keyed by
};
struct DiagHost;                        // update diagnostics (learner_eval.hip; the kernels: diag_kernels.hip.h)
struct SweepHost;                       // replay sweep (learner_eval.hip; the kernels: sweep_kernels.hip.h)
struct SaveWriter;                      // asynchronous learner-state save and Caffe snapshot (learner_save_async.hip; the kernels: state_kernels.hip.h, snapshot_kernels.hip.h)

}  // namespace dqnhip_host

using namespace dqnhip;          // (internal header: every includer is a translation unit of this library)
using namespace dqnhip_host;

struct dqnhip_learner {
  dqnhip_config cfg;
  int B = 0, S = 0, L = 0;
  NetLayout la, lc;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  // parameter arenas
  float* w[4] = {nullptr, nullptr, nullptr, nullptr};
  float* m[2] = {nullptr, nullptr};
  float* v[2] = {nullptr, nullptr};
  float* g[2] = {nullptr, nullptr};     // inside grad_base
  float* grad_base = nullptr; bool own_grad = false;
  // replay
  Ring ring{};
  DevState* st = nullptr;
  int* done_counter = nullptr;
  long long h_head = 0, h_size = 0;     // host mirror of (head,size)
  bool ring_stale = false;              // the device changed (head,size) on its own (env front-end)
  // sharing (DQN::ShareParameters / ShareReplayMemory, src/dqn.cpp:1036-1083): a sharer keeps
  // its own allocations and reads the owner's through these
  dqnhip_learner* ring_owner = nullptr; // whose ring / (head,size) this learner uses (nullptr: own)
  dqnhip_learner* w_owner = nullptr;    // owner of the shared first layers
  size_t shared_fl[2] = {0, 0};         // arena floats [0, shared_fl) of actor / critic (+targets) live in w_owner
  int sharers = 0;                      // learners that reference this one
  bool ring_shared = false;             // more than one learner uses this ring: order users across streams
  hipEvent_t ring_ev = nullptr; hipStream_t ring_last = nullptr; bool ring_ev_valid = false;
  std::mutex ring_mu;
  int h_actor_iter = 0, h_critic_iter = 0;
  unsigned long long sample_states_calls = 0;
  // native data parallelism (dqnhip_dp_*): one RCCL communicator per learner
  ncclComm_t comm = nullptr;
  int rccl_version = 0;                 // ncclGetVersion of the build this process resolved (cross-checked over the group in dqnhip_dp_init)
  bool dp_per_layer = false;            // bucket the gradient all-reduce per layer on comm_stream
  bool dp_half = false;                 // gradients cross the links as bf16 (half the bytes); [loss, q, flag] tails stay fp32
  // DQNHIP_DP_SHARD_OPT: reduce-scatter -> clip + Adam + soft update on this rank's 1/N slice of each arena -> all-gather of
  // the updated online and target weights (m, v of the other slices go stale until dqnhip_dp_gather_state)
  bool dp_shard = false;
  float* shard_total = nullptr;         // dqnhip_apply_update_sharded: the group's sum of squares, accumulated rank by rank
  bool shard_stale = false;             // a sharded update ran since the last dqnhip_dp_gather_state: m, v of foreign slices are stale
  uint16_t* g16[2] = {nullptr, nullptr};   // bf16 transfer image of each gradient arena (dp_half)
  float* dp_tails = nullptr;            // dp_half: {critic tail[4], actor tail[4]}, one fp32 all-reduce with the actor's gradients
  hipStream_t comm_stream = nullptr;
  hipEvent_t comm_ev[2] = {nullptr, nullptr};
  hipGraphExec_t dp_graph = nullptr;    // the whole data-parallel update (collectives included), captured
  bool dp_graph_failed = false;
  hipGraphExec_t dp_graph_n = nullptr;  // kMultiU of them (dqnhip_dp_update_n)
  bool dp_graph_n_failed = false;
  int next_phase = 0;                   // dqnhip_update_phase order check (0: an update may start)
  // minibatch panels / activations: pass 0 AT, 1 A, 2 CT, 3 C1, 4 C2
  float* Xa_s = nullptr; float* Xa_n = nullptr; float* Xc_tr = nullptr; float* Xc_pl = nullptr; float* Xc_nx = nullptr;
  // inside multi-update graphs that gather one launch group early (early_l0): the two panels an update still reads after the next
  // update's gather has run exist twice, by update parity; Xa_s / Xc_pl (and act[1][0] / act[4][0]) point at the current update's
  float* Xa_s2[2] = {nullptr, nullptr}; float* Xc_pl2[2] = {nullptr, nullptr};
  float* act[5][kMaxL + 1] = {{nullptr}};
  float* dZa[kMaxL + 1] = {nullptr};
  float* dZc[kMaxL + 1] = {nullptr};
  float *mb_reward = nullptr, *mb_mc = nullptr, *mb_term = nullptr;
  float* qdot[2] = {nullptr, nullptr};   // [B][kp[L] / 16]: the head dot products of critic_target(s', .) / critic(s, a) in 16-column pieces (GemmProblem::dot_w)
  float* Wact_t = nullptr;              // [kNO][dims[1]] (first_layers_launch)
  float* Zs = nullptr;                  // [B][kp[1]]: the state half of critic_target's first layer, before bias / ReLU (first_layers_launch)
  float* U3 = nullptr;                  // [B][kp[L]]: (-w_h) lrelu'(x_L) of the critic(s, a) training pass (left by its top forward layer for k_dgrad_qtrain)
  int* mb_idx = nullptr;
  int* idx_pinned = nullptr;
  const int* idx_pinned_dev = nullptr;  // device alias of idx_pinned: the gather reads explicit indices straight from host memory (no H2D copy)
  float* stats_dev = nullptr;           // device alias of pinned_stats: the update's last block writes {loss, avg_q, flags} there
  float *aout_t16 = nullptr, *aout16 = nullptr, *dA16 = nullptr;
  float *q_t = nullptr, *q1 = nullptr, *q2 = nullptr, *y = nullptr, *dq = nullptr;
  float* loss_partial = nullptr; double* q_partial = nullptr; int n_head_blocks = 0;
  float* part[2] = {nullptr, nullptr};  // GEMM-epilogue sumsq partials per net
  float* part_dp = nullptr; int n_part_dp = 0;
  float* head_slab = nullptr; int* head_ticket = nullptr;   // k_head_bwd cross-block reduction
  float* head_slab2 = nullptr;                               // k_head_bwd_big row-chunk slabs (minibatch >= 1024)
  // mixed precision (cfg.precision == DQNHIP_FP16): ONE fp16 mirror of each weight arena and batch-major fp16
  // activation / gradient panels; the dgrad and wgrad GEMMs read them reduction-major (hgemm.hip.h), so no
  // transposed copy of anything exists
  bool fp16 = false;
  float ls_c = 1.f, ls_q = 1.f, ls_a = 1.f;  // static loss scales: critic step, dQ/da pass, actor step
  // cfg.loss_scale_mode == DQNHIP_LOSS_SCALE_DYNAMIC: the kernels multiply the static scales by the live multipliers in
  // DevState::ls_mult (ls_c by the critic's, ls_q and ls_a by the actor's), which the optimiser launches of an update adjust
  bool ls_dynamic = false;
  int k16[2][kMaxL + 1] = {{0}};             // fp16 panel widths per net kind (k16[.][0] = in_dim rounded to 128)
  h16* w16a[4] = {nullptr, nullptr, nullptr, nullptr};   // fp16 mirror of each weight arena (written by the Adam pass)
  h16* w16[4][kMaxL] = {{nullptr}};          // = w16a[net] + w_off[i]: [N_out][kp]
  h16* act16[5][kMaxL + 1] = {{nullptr}};    // [B][k16]
  h16* dZ16[2][kMaxL + 1] = {{nullptr}};     // [B][k16]   per net kind
  bool w16_dirty[4] = {true, true, true, true};
  std::vector<void*> allocs16;
  // fp16 acting (dqnhip_set_act_precision): a host flag and an epoch (an env handle compares it and drops its captured steps),
  // and acting panels of their own — act16[] belong to the update and hold B rows.  actp16[i]: [actp16_rows][max(k16[0][i],
  // k16[1][i])] (a pass uses its net kind's k16 as the row pitch), actp16_out: [actp16_rows][kAP + 1] floats (head outputs / q);
  // rows are a multiple of 64, the smallest hgemm tile (ensure_act16 grows them, zero-filled)
  bool act_fp16 = false;
  unsigned long long act_epoch = 0;
  h16* actp16[kMaxL + 1] = {nullptr};
  float* actp16_out = nullptr;
  int actp16_rows = 0;
  // host-staging for add_transitions / acting
  void* stage_dev = nullptr; size_t stage_bytes = 0;
  float* act_buf = nullptr; size_t act_floats = 0;
  float* pinned_stats = nullptr;
  // timing
  bool timing = false;
  std::vector<TimingRec> recs;
  // graph
  int cap_u = -1;              // while capturing a multi-update graph: the position of the update being captured (else -1)
  int cap_n = 16;              // ... and the number of updates of that graph (the last one carries no riders for a successor)
  hipGraphExec_t graph_small[3] = {nullptr, nullptr, nullptr};   // dqnhip_update_async_n: 8 / 4 / 2 updates, for what is left after the sixteen-update graphs
  hipGraphExec_t graph_exec[kNumGraphSlots] = {nullptr};         // by GraphSlot
  bool graph_failed = false;
  // dqnhip_update_chained (the drop-in's blocking update with the NEXT update's indices known one call ahead): the next update's gather
  // and first layers ride in this update's optimiser launches, as inside a multi-update graph.  What rode along is only used if the
  // next call brings exactly those indices and nothing touched weights, iterations or the replay memory in between (epoch).
  unsigned long long epoch = 0;         // bumped by every entry point that changes weights, iteration counters or the replay memory
  bool chain_cap = false;               // a chain graph is being captured (gather_args: riders read idx_next, counters = live + 1)
  bool chain_valid = false; int chain_par = 0;
  unsigned long long chain_epoch = 0, chain_ring_epoch = 0;
  std::vector<int32_t> chain_idx;       // the indices the riders gathered
  int* idx_next_pinned[2] = {nullptr, nullptr}; const int* idx_next_dev[2] = {nullptr, nullptr};   // by the parity of the update they belong to
  // dqnhip_update_pipelined
  hipEvent_t pipe_ev[2] = {nullptr, nullptr};
  int* pipe_idx_dev[2] = {nullptr, nullptr}; int* pipe_idx_pinned[2] = {nullptr, nullptr};
  float* pipe_stats[2] = {nullptr, nullptr};
  unsigned long long pipe_count = 0;
  // dqnhip_update_indexed_n / dqnhip_collect_stats.  Bank b: kMultiU index vectors and kMultiU {loss, avg_q, flags, -} slots in pinned,
  // host-mapped memory; position u of a graph captured for bank b gathers from index slot u and its tick writes stats slot u.
  // ix_ev[b] is recorded behind whatever was enqueued on the bank; ix_busy[b] is the number of updates of it not yet harvested.
  int* ix_idx[kIxBanks] = {nullptr}; const int* ix_idx_dev[kIxBanks] = {nullptr};
  float* ix_stats[kIxBanks] = {nullptr}; float* ix_stats_dev[kIxBanks] = {nullptr};
  hipEvent_t ix_ev[kIxBanks] = {nullptr};
  int ix_busy[kIxBanks] = {0};
  int ix_next = 0;                      // the bank the next graph takes (round robin: the busy banks are the most recent ones, in order)
  hipGraphExec_t ix_graph[kIxBanks][kIxSizes] = {{nullptr}};   // [bank][16, 8, 4, 2, 1 updates]
  long long opt_launches[3] = {0, 0, 0};   // optimiser launches enqueued or captured: k_adam_soft*, k_solver_soft<>, k_solver_soft_gather<> (dqnhip_debug_read "optimiser_launches")
  // lr policy / weight decay (cfg.lr_policy, cfg.weight_decay): the schedule as the device reads it (GatherArgs::sched; null: fixed)
  LrSchedule sched{}; LrSchedule* sched_dev = nullptr;
  long long sched_launches[2] = {0, 0};    // k_sched_soft<>, k_sched_soft_gather<> enqueued or captured (dqnhip_debug_read "sched_launches")
  int ix_nodes[kIxSizes] = {0};         // kernel nodes of the captured graph of each size (dqnhip_debug_read "indexed_graph_launches")
  const int* cap_idx = nullptr;         // while an indexed graph is captured / an indexed update runs eagerly: the bank's index slots ...
  float* cap_stats = nullptr;           // ... and its stats slots (device aliases); tick_args / gather_args read them
  std::deque<float> ix_pairs;           // harvested, uncollected (loss, avg_q) pairs, flat: 8 bytes per update
  std::deque<std::pair<unsigned long long, int>> ix_flagged;   // (sequence number, flags that update raised) of harvested updates
  unsigned long long ix_harvested = 0, ix_collected = 0;       // sequence numbers: updates harvested / handed out so far
  int ix_prev_flags = 0;                // the sticky device flags as the last harvested update left them (a raise = a bit not in here)
  long long per_env_slack = 0;          // transitions the recording env front-ends of this ring may hold back and append later (workers x max_steps each)
  PerHost* per = nullptr;               // prioritized replay (dqnhip_per_enable); null: uniform sampling, nothing below runs
  TargetNoiseHost* tnoise = nullptr;    // target policy smoothing (dqnhip_target_noise_enable); null: the clean mu'(s'), nothing of it runs
  NstepHost* nstep = nullptr;           // n-step returns (dqnhip_nstep_enable); null: the 1-step target, nothing of it runs
  DiagHost* diag = nullptr;             // update diagnostics (dqnhip_diag_collect): its work table and scratch, allocated by the first collection
  // replay sweep (dqnhip_evaluate_memory / dqnhip_per_refresh): its scratch, allocated by the first sweep, and one captured chunk of
  // each kind (by refresh)
  SweepHost* sweep = nullptr;
  hipGraphExec_t sweep_graph[2] = {nullptr, nullptr};
  SaveWriter* sasync = nullptr;        // dqnhip_save_state_async / dqnhip_snapshot_async: the writer thread, the pinned ring and each kind's staging buffer, allocated at first use
};

namespace dqnhip_host {

using H = dqnhip_learner;

// ring owner / weight views under sharing
inline H* RO(H* h) { return h->ring_owner ? h->ring_owner : h; }
inline const H* RO(const H* h) { return h->ring_owner ? h->ring_owner : h; }
inline float* wat(const H* h, int net, size_t off) {
  return ((off < h->shared_fl[net & 1]) ? h->w_owner->w[net] : h->w[net]) + off;
}

// Orders the users of a SHARED ring across their streams in host-call order: each user waits
// for the previous user's completion event.  No-op (no lock, no event) for a private ring.
struct RingUse {
  H* o; hipStream_t st; bool on;
  RingUse(H* h) : o(RO(h)), st(h->stream), on(RO(h)->ring_shared) {
    if (!on) return;
    o->ring_mu.lock();
    if (o->ring_ev_valid && o->ring_last != st) hipStreamWaitEvent(st, o->ring_ev, 0);
  }
  ~RingUse() {
    if (!on) return;
    hipEventRecord(o->ring_ev, st); o->ring_last = st; o->ring_ev_valid = true;
    o->ring_mu.unlock();
  }
};

// Where one launch of family `fam` goes: `st`, and in timing mode a fresh event pair, filed in h->recs, that launch() has the
// dispatch packet stamp.  The caller hands the result to exactly ONE launcher: events that no launch records cannot be read back.
inline LaunchOn timed(H* h, Family fam, hipStream_t st) {
  LaunchOn on(st);
  on.no_preload = (h->cfg.tuning_flags & DQNHIP_TUNE_NO_KERNARG_PRELOAD) != 0;
  if (!h->timing) return on;
  hipEventCreate(&on.start); hipEventCreate(&on.stop);
  h->recs.push_back({fam, on.start, on.stop});
  return on;
}

// ---- dense (Caffe order) <-> internal arena ----------------------------------
void dense_to_arena(const NetLayout& l, const float* dense, std::vector<float>& arena);
void arena_to_dense(const NetLayout& l, const std::vector<float>& arena, float* dense);
inline const NetLayout& layout_of(const H* h, int net) { return (net & 1) ? h->lc : h->la; }
// validates *c — of today's struct_size, or of the size before the lr_policy .. regularization_type block existed — into *full
int validate(const dqnhip_config* c, dqnhip_config* full);
LrSchedule schedule_of(const dqnhip_config& c);
inline bool has_policy(const H* h) { return h->cfg.lr_policy != DQNHIP_LR_FIXED; }
inline bool has_decay(const H* h) { return h->cfg.weight_decay != 0.0f; }
// does this learner's optimiser pass run k_sched_soft<>?  (an Adam learner with a policy and no decay keeps the tuned kernels)
inline bool sched_family(const H* h) { return has_decay(h) || (has_policy(h) && h->cfg.solver_type != DQNHIP_SOLVER_ADAM); }
// ---- what a call asks of a learner before it refuses it: every site composes these, none writes a condition out ----
// Data parallelism, twice: a one-rank group has a communicator (dqnhip_dp_init) and still runs the single-learner entry points.
// dp_exchanges: this learner's update runs the N-rank code path (plan_of's dp; the single-learner update forms refuse it)
inline bool dp_exchanges(const H* h) { return h->cfg.dp_world > 1 || h->dp_half || h->dp_shard; }
// dp_grouped: ... or it belongs to a group at all, a one-rank group included (what the opt-in features, the sweep and the state file refuse)
inline bool dp_grouped(const H* h) { return dp_exchanges(h) || h->comm; }
// uses another learner's ring, or others use (or used) its own
inline bool shares_ring(const H* h) { return h->ring_owner || h->ring_shared; }
// reads another learner's parameters, or other learners reference this one (sharers counts ring users too)
inline bool shares_params(const H* h) { return h->w_owner || h->sharers; }
// The four opt-in features a learner can carry, in the order feature_refuse checks them
enum Feature : unsigned {
  kFeatSched = 1u,                      // cfg.lr_policy / cfg.weight_decay
  kFeatPer = 2u,                        // prioritized replay (dqnhip_per_enable)
  kFeatNstep = 4u,                      // n-step returns (dqnhip_nstep_enable)
  kFeatSmooth = 8u,                     // target policy smoothing (dqnhip_target_noise_enable)
  kFeatSampling = kFeatPer | kFeatNstep | kFeatSmooth,      // the three that change what an update gathers and targets
  kFeatAll = kFeatSched | kFeatSampling
};
// the v1 refusals (learner_features.hip): fails, as `what`, naming the first feature of `mask` — in the order above — that h carries
int feature_refuse(const H* h, unsigned mask, const char* what);
bool is_pow2(float x);                                   // a positive, normal power of two (loss-scale multipliers)
// shape predicates of the launch schedules (learner_plan.hip)
bool bwd_layer_is_pair(const NetLayout& l, int i, int rows);
bool bwd_is_shifted(const H* h, const NetLayout& l, int rows);
bool head_big_ok(const H* h, int rows, int Hd);
bool dqda_head_shape_ok(const H* h, int panel_w);   // k_dqda_head_bwd's shapes (the fused form, and the fp16 learner's tile-alone launch)
bool early_l0(const H* h);                               // plan_of(h).early_l0 while a multi-update graph is being captured
inline size_t grad_arena_floats(const NetLayout& la, const NetLayout& lc) { return la.arena + 64 + lc.arena + 64; }

// ---- building blocks defined in learner.hip ----------------------------------------------------------------------
// seed_w / seed_out: the TOP layer's launch also writes the dq = -1 pass's tower-top gradient (GemmProblem::seed_w)
struct FwdPass { int net; const NetLayout* l; float** act; const float* seed_w = nullptr; float* seed_out = nullptr;
                 const float* dot_w = nullptr; float* dot_out = nullptr; };   // dot_w / dot_out: GemmProblem::dot_w, same layer

int layer_forward(H* h, hipStream_t st, const FwdPass* passes, int n, int rows, int i);
int tower_forward(H* h, hipStream_t st, const FwdPass* passes, int n, int rows, int first_layer = 0);   // first_layer 1: layer 0 came out of a FirstLayerRider
// the fp16 tower of `net` on caller-supplied panels: panels[i] is [rows][k16[net & 1][i]] fp16, rows % 64 == 0; layer i reads
// panels[i] and the net's fp16 weight mirror and writes panels[i + 1].  A dirty mirror (set_params, Load*, Restore*, CloneNet) is
// brought up to date first — not while `st` is capturing: the caller of a capture runs sync_dirty16 before it begins
int tower_forward16_on(H* h, hipStream_t st, int net, h16* const* panels, int rows);
// head_forward<NH, MODE>: head_fwd_kernels.hip.h (a template that names kernels: its users include it)
constexpr int kMultiU = 16;    // updates per replay of the multi-update graph (dqnhip_update_async_n; see learner_update.hip)
// Philox key of SampleTransitionsFromMemory: cfg.seed on rank 0 (what oracle/c_oracle.philox_indices
// reproduces); data-parallel ranks get distinct streams from the SAME cfg.seed, so that the weight
// initialisation (also keyed by cfg.seed) stays identical across the group
inline uint64_t sample_key(const H* h) { return (uint64_t)h->cfg.seed + 0x9E3779B97F4A7C15ull * (uint64_t)h->cfg.dp_rank; }
inline void shard_range(const H* h, int net, size_t& lo, size_t& hi, int rank = -1) {
  const size_t slice = layout_of(h, net).arena / (size_t)h->cfg.dp_world;
  const size_t r = (size_t)(rank < 0 ? h->cfg.dp_rank : rank);
  lo = r * slice; hi = lo + slice;
}
// Which merged forms the update of a learner takes (plan_of, learner_plan.hip: the one place that decides; dqnhip_get_update_plan reports it)
struct UpdatePlan {
  bool fp16, dp;
  bool shifted_c, shifted_a;        // the shifted backward schedule (tower_backward) for the critic's Step(1) / the actor's backward
  bool head_rides_c, head_rides_a;  // the head's dW / db as rider blocks of the net's last backward launch
  bool fuse_q;                      // k_dgrad_qtrain: Step(1)'s head arithmetic inside the critic's top-layer dgrad launch
  bool fused_seed;                  // the dq = -1 seed from the top layer's forward epilogue, q(s, mu(s)) as rider blocks
  bool fuse_head;                   // k_dqda_head_bwd: dQ/da's last step + inverting gradients + actor heads' backward in one launch
  bool critic_l0;                   // the first layer of critic(s, mu(s)) inside the critic's optimiser launch
  bool first_layers_merged;         // Step(1)'s four first layers in one launch (critic_target's action half in the head kernel)
  bool early_l0;                    // multi-update graphs: next gather in the critic's optimiser launch, next first layers in the actor's
  bool tails_ride;                  // data parallel: the [loss, q, flag] tails block rides in each net's last backward launch (no k_tails launches)
  bool prioritized;                 // prioritized replay: k_per_sample / k_per_fill before, k_head_q_train_w inside, k_per_update behind every update
  bool smooth;                      // target policy smoothing: k_target_smooth behind the actors' heads, the critics' first layers behind it (never merged)
  bool nstep;                       // n-step returns: k_gather_n first, k_head_q_train_n<prioritized> in the head launch's place; the stand-alone sequence per update
};
UpdatePlan plan_of(const H* h);
// the current update's copies of the two double-buffered panels (by update parity inside a multi-update graph that gathers early;
// parity 0 everywhere else — every capture ends by selecting parity 0 again)
inline void select_panels(H* h, int par) { h->Xa_s = h->Xa_s2[par]; h->Xc_pl = h->Xc_pl2[par]; h->act[1][0] = h->Xa_s; h->act[4][0] = h->Xc_pl; }
struct NextL0 { ActorL0 a; PlainL0 c, ct; };           // the next update's first layers as riders of the actor's optimiser launch
int adam_launch(H* h, hipStream_t st, int net, const float* partial, int n_partial, size_t begin, size_t end, const TickArgs* tick = nullptr,
                bool corr_pre = true, const FirstLayerRider* fl = nullptr, const GatherArgs* early_gather = nullptr, const NextL0* next_l0 = nullptr);
int sumsq_launch(H* h, int net, size_t begin = 0, size_t end = 0);
int to_bf16_launch(H* h, int net);                       // k_to_bf16: the bf16 transfer image of a gradient arena
int shard_scal_launch(H* h, float* tail);                // k_shard_scal: this rank's share of the clip norm -> tail[3]
int run_phase(H* h, int phase, const int* idx_dev);
int sync_dirty16(H* h);
// One chunk of a replay sweep up to its row kernel: the update's gather on idx_dev (without its scalars block: DevState stays as it
// is) and the update's forward launches — actor_target(s'), actor(s), critic_target, critic(s, a), k_head_q_train, critic(s, mu(s))
// and its q head — on the learner's panels and row buffers.  No backward, no optimiser.  flag_sink: where k_head_q_train raises its
// non-finite-target flag instead of the learner's DevState (the sticky flags belong to updates).  fp32 learners.
int sweep_forward(H* h, const int* idx_dev, DevState* flag_sink);
int prepare_kernels(const H* h);                         // the launch attributes (dynamic-LDS limits) of the update's kernels
// learner_update.hip
int refresh_ring(H* h);
int stage_indices(H* h, const int32_t* idx_host, const int** idx_dev);
int run_update(H* h, const int* idx_dev);                // phases 0, 1, 2
// One capture: `updates` runs of `body` on the learner's stream.  multi: as positions 0 .. updates - 1 of a multi-update graph of
// `of` updates (each update's riders serve its successor; the last of `of` has none).  chain_pos >= 0 (dqnhip_update_chained): ONE
// update captured as that position, its riders reading the next update's explicit indices.
struct CaptureSpec {
  int updates = 1; bool multi = false; int of = kMultiU; int chain_pos = -1;
  const int* idx_dev = nullptr;                          // explicit indices (nullptr: sampled on the device)
  // dqnhip_update_indexed_n: position u gathers from idx_bank + u * B (position 0: idx_dev, the same address) and its tick writes
  // stats_bank + 4 * u instead of the learner's one pinned triple
  const int* idx_bank = nullptr; float* stats_bank = nullptr;
  int (*body)(H*, const int*) = run_update;              // (data parallel: dp_sequence, the phases with the exchange between them)
};
int capture_updates(H* h, const CaptureSpec& s, hipGraph_t* graph);
int capture_exec(H* h, const CaptureSpec& s, hipGraphExec_t* out, int* kernel_nodes = nullptr);      // ... and instantiate
// n_chunks runs of `body` (one chunk of a replay sweep: its launches read the chunk base from device memory) on the learner's stream:
// replays of *g, captured from `body` on first use, or eagerly where graphs are off
int run_chunks(H* h, hipGraphExec_t* g, int n_chunks, int (*body)(H*, const int*));
int ix_harvest_all(H* h);                                // waits for every indexed update enqueued so far and files its scalars
// learner_create.hip
int ensure_stage(H* h, size_t bytes);
int ensure_act(H* h, int rows);
inline int act16_rows(int n) { return round_up(n, 64); }                  // acting-panel rows for n inputs: whole 64-row hgemm tiles
inline int act16_width(const H* h, int i) { return std::max(h->k16[0][i], h->k16[1][i]); }
int ensure_act16(H* h, int rows);                        // the fp16 acting panels (H::actp16, actp16_out) for `rows` rows
void drop_graphs(H* h);                                  // every captured launch sequence of this learner
// learner_dp.hip
int dp_reduce_slice(H* h, hipStream_t st, int net, size_t off, size_t count);
int dp_allgather_weights(H* h, int net);
int dp_destroy_impl(H* h, bool keep_learner);
const char* rccl_path();
// learner_io.hip
bool same_nets(const H* a, const H* b);
// k_pack_rows16: fp32 [n][ld_src] (the first S columns of each row) -> fp16 [rows][k16], pad rows and columns zero
int pack_rows16_launch(hipStream_t st, const float* src, int n, int S, int ld_src, h16* dst, int rows, int k16);
// learner_per.hip — prioritized replay: the host launchers of per_kernels.hip.h and what the other units need of it
int per_sync_if_needed(H* h);                            // k_per_sync, if the ring may have changed since the last one
void per_note_append(H* h, long long n);                 // BEFORE up to n transitions are appended: keeps the bound below cap (may enqueue a sync)
int per_sample_launch(H* h);                             // k_per_sample on the live counter -> per->idx / slot / prob
int per_fill_launch(H* h, const int* idx_dev);           // k_per_fill: explicit indices -> per->slot / prob
int per_update_launch(H* h);                             // k_per_update
int per_clear(H* h);                                     // dqnhip_clear_memory: the tree zero, p_max stays
void per_free(H* h);
const float* per_p_max_dev(const H* h);                  // the device address of PerDev::p_max (null: not a prioritized learner)
int per_read_p_max(H* h, float* p_max);                  // PerDev::p_max, behind everything enqueued so far
int per_restore(H* h, const float* leaves, int head, int size, float p_max, long long syncs);   // dqnhip_load_state: the tree from a window's leaves
// learner_features.hip
void nstep_free(H* h);
void smooth_free(H* h);
// does every update of this learner run the stand-alone sequence, also inside a multi-update graph?  (no rider serves a successor)
inline bool standalone_updates(const H* h) { return h->per != nullptr || h->nstep != nullptr; }
// learner_eval.hip
void diag_free(H* h);                                    // dqnhip_diag_collect's scratch
void sweep_free(H* h);                                   // the replay sweep's scratch
// learner_save_async.hip
int state_async_join(H* h, const char* what);            // waits for a save in flight; fails, as `what`, with its message if it failed
void state_async_free(H* h);                             // dqnhip_destroy: joins both kinds of job, stops the writer thread, frees; never fails
int snapshot_async_join(H* h, const char* what);         // waits for a snapshot in flight; fails, as `what`, with its message if it failed

}  // namespace dqnhip_host
