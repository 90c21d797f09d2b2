// learner_env.hip — host side of the batched env front-end (include/dqnhip_env.h; device side: env.hip.h).
#include "learner_internal.hip.h"
#include "env.hip.h"
#include "gemm_bodies.hip.h"        // k_env_l0_flush carries a forward GEMM tile
#include "head_fwd_kernels.hip.h"

using namespace dqnhip;
using namespace dqnhip_host;

struct dqnhip_env {
  dqnhip_learner* h = nullptr;
  dqnhip_env_config cfg{};
  EnvDev d{};
  int Npad = 0;
  float* acts[kMaxL + 1] = {nullptr};
  std::vector<void*> allocs;
  float* eps_dev = nullptr;
  int* commit_ticket = nullptr;
  hipGraphExec_t graph[2] = {nullptr, nullptr};   // one batched step / kEnvUnroll steps, captured on first use
  bool graph_failed = false;
  int graph_nodes[2] = {0, 0};                    // launches in each captured graph (dqnhip_env_debug_read "graph_nodes")
  // inside a sequence of batched steps the episode flush of step t (LabelTransitions + AddTransitions of the
  // finished episodes) rides as extra workgroups of step t+1's first-layer launch: k_env_step resets the worker
  // itself, so nothing before the next k_env_step depends on the flush
  bool flush_deferred = false;
  // fp16 acting (dqnhip_set_act_precision): the learner's switch as this handle last saw it — a changed epoch drops the captured
  // steps — and fp16 panels of the env's own: p16[0] the actor's input panel k_env_step<true> writes, p16[i] layer i's output;
  // [Npad16][k16[0][i]], whole 64-row hgemm tiles, zero-filled (the pad rows stay zero), allocated when the mode is first seen
  unsigned long long act_epoch = 0;
  bool slack_counted = false;           // this handle's workers x max_steps is in the ring owner's per_env_slack
  bool f16 = false;
  int Npad16 = 0;
  h16* p16[kMaxL + 1] = {nullptr};
  // the external kind (dqnhip_env_create_external): the caller's simulator sits between dqnhip_env_act and dqnhip_env_observe
  bool external = false, record = true;
  bool acted = false;                   // an act is waiting for its observe
  EnvExt x{};
  long long observes = 0;
  // the host variants' staging: device copies of what act hands out / observe takes in, and their pinned host mirrors
  int* d_action = nullptr; float* d_args = nullptr; float* d_ao = nullptr;
  float* d_next = nullptr; int* d_status = nullptr; int* d_pob = nullptr;
  void* pinned = nullptr;               // [action N | status N | pob N | args 2N | actor_out 10N | next N*S]
  // episode records: what each worker's ring has handed out so far, and the merged records not yet read
  std::vector<unsigned long long> rec_read;
  std::deque<dqnhip_env_episode> pending;
  long long dropped = 0;
  // exploration noise (dqnhip_env_set_noise): off — the handle launches the kernels it always launched — or on: the NOISE
  // instantiations with nz as their further argument.  nz's buffers are allocated when noise is first enabled.
  bool noise = false;
  EnvNoise nz{};
};
constexpr int kEnvUnroll = 16;
static_assert(sizeof(EnvEpisode) == sizeof(dqnhip_env_episode) && offsetof(EnvEpisode, step_index) == offsetof(dqnhip_env_episode, step_index) &&
              offsetof(EnvEpisode, steps) == offsetof(dqnhip_env_episode, steps), "k_env_observe writes dqnhip_env_episode records");

namespace {
template <typename T>
int env_alloc(dqnhip_env* e, T** p, size_t n) {
  HIPCHK(hipMalloc(p, n * sizeof(T)));
  HIPCHK(hipMemsetAsync(*p, 0, n * sizeof(T), e->h->stream));
  e->allocs.push_back((void*)*p);
  return 0;
}
}  // namespace

extern "C" {

static int env_create_impl(dqnhip_env* e, const float* first_states_host);

// the pinned staging block's parts (dqnhip_env::pinned)
static int32_t* pin_action(dqnhip_env* e) { return (int32_t*)e->pinned; }
static int32_t* pin_status(dqnhip_env* e) { return (int32_t*)e->pinned + e->d.N; }
static int32_t* pin_pob(dqnhip_env* e) { return (int32_t*)e->pinned + 2 * (size_t)e->d.N; }
static float* pin_args(dqnhip_env* e) { return (float*)e->pinned + 3 * (size_t)e->d.N; }
static float* pin_ao(dqnhip_env* e) { return (float*)e->pinned + 5 * (size_t)e->d.N; }
static float* pin_next(dqnhip_env* e) { return (float*)e->pinned + (5 + kNO) * (size_t)e->d.N; }

// the env's fp16 panels (allocated once, zero-filled) and the fp16 kernels' extra argument
static int env_panels16(dqnhip_env* e) {
  dqnhip_learner* h = e->h;
  if (e->p16[0]) return 0;
  if (h->k16[0][0] != e->d.SP) return fail("internal: the fp16 actor input panel is %d wide, the env's state rows %d", h->k16[0][0], e->d.SP);
  e->Npad16 = act16_rows(e->d.N);
  for (int i = 0; i <= h->L; ++i) RC(env_alloc(e, &e->p16[i], (size_t)e->Npad16 * h->k16[0][i]));
  return 0;
}
static Env16 env16_of(const dqnhip_env* e, bool fused) {
  Env16 x{}; x.x16 = e->p16[0]; x.ldx16 = e->h->k16[0][0]; x.head_x16 = fused ? e->p16[e->h->L] : nullptr;
  return x;
}

static int env_create_any(dqnhip_handle h, const dqnhip_env_config* cfg, bool external, int32_t flags, const float* first_states_host,
                          dqnhip_env_handle* out) {
  if (!h || !cfg || !out) return fail("null argument");
  *out = nullptr;
  const bool record = !(flags & DQNHIP_ENV_NO_RECORD);
  if (cfg->struct_size != (int32_t)sizeof(dqnhip_env_config)) return fail("dqnhip_env_config.struct_size mismatch");
  if (cfg->workers < 1 || cfg->workers > (1 << 20)) return fail("workers out of range");
  if (cfg->max_steps < 1 || cfg->max_steps > 4096) return fail("max_steps out of range");
  if (h->S < 56) return fail("HFOGameState reads state indices up to 55: state_size must be >= 56 (src/hfo_game.cpp:130-152)");
  if (record && (long long)cfg->workers * cfg->max_steps >= RO(h)->ring.cap)
    return fail("replay capacity %d must exceed workers*max_steps = %lld", RO(h)->ring.cap, (long long)cfg->workers * cfg->max_steps);
  HIPCHK(hipSetDevice(h->cfg.device));
  dqnhip_env* e = new dqnhip_env();
  e->h = h; e->cfg = *cfg; e->external = external; e->record = record;
  const int rc = env_create_impl(e, first_states_host);
  if (rc) { const std::string msg = g_err; dqnhip_env_destroy(e); g_err = msg; return rc; }
  if (record) { RO(h)->per_env_slack += (long long)cfg->workers * cfg->max_steps; e->slack_counted = true; }   // (prioritized replay: what this handle may hold back)
  *out = e;
  return 0;
}

int dqnhip_env_create(dqnhip_handle h, const dqnhip_env_config* cfg, dqnhip_env_handle* out) {
  return env_create_any(h, cfg, false, 0, nullptr, out);
}
int dqnhip_env_create_external(dqnhip_handle h, const dqnhip_env_config* cfg, int32_t flags, const float* first_states_host,
                               dqnhip_env_handle* out) {
  if (flags & ~DQNHIP_ENV_NO_RECORD) return fail("unknown flags %d", (int)flags);
  if (!first_states_host) return fail("null argument");
  return env_create_any(h, cfg, true, flags, first_states_host, out);
}

static int env_create_impl(dqnhip_env* e, const float* first_states_host) {
  dqnhip_learner* h = e->h;
  const dqnhip_env_config* cfg = &e->cfg;
  EnvDev& d = e->d;
  d.N = cfg->workers; d.S = h->S; d.SP = h->la.kp[0]; d.T = cfg->max_steps; d.unum = cfg->unum;
  d.p_end = cfg->p_end; d.p_goal = cfg->p_goal; d.seed = cfg->seed;
  e->Npad = round_up(d.N, 32);
  const size_t N = d.N, Np = e->Npad;
  RC(env_alloc(e, &d.cur, Np * d.SP)); RC(env_alloc(e, &d.out16, Np * kAP));
  if (e->record) { RC(env_alloc(e, &d.ep_s, N * d.T * d.SP)); RC(env_alloc(e, &d.ep_a, N * d.T * kAP)); RC(env_alloc(e, &d.ep_r, N * d.T)); }
  RC(env_alloc(e, &d.game, N)); RC(env_alloc(e, &d.len, N)); RC(env_alloc(e, &d.done, N)); RC(env_alloc(e, &d.g, N));
  RC(env_alloc(e, &d.act, N)); RC(env_alloc(e, &d.arg1, N)); RC(env_alloc(e, &d.arg2, N)); RC(env_alloc(e, &d.rew, N));
  RC(env_alloc(e, &d.n_steps, N)); RC(env_alloc(e, &d.n_episodes, N)); RC(env_alloc(e, &d.n_goals, N)); RC(env_alloc(e, &d.reward_sum, N));
  e->acts[0] = d.cur;
  for (int i = 1; i <= h->L; ++i) RC(env_alloc(e, &e->acts[i], Np * h->la.kp[i]));
  RC(env_alloc(e, &e->eps_dev, 16)); d.eps = e->eps_dev;
  RC(env_alloc(e, &e->commit_ticket, 32));
  e->act_epoch = h->act_epoch; e->f16 = h->act_fp16;
  if (e->external) {
    EnvExt& x = e->x;
    x.record = e->record ? 1 : 0;
    RC(env_alloc(e, &x.rec, N * kEnvRecRing)); RC(env_alloc(e, &x.rec_n, N)); RC(env_alloc(e, &x.tot, N)); RC(env_alloc(e, &x.ext, N));
    RC(env_alloc(e, &x.truncated, N)); RC(env_alloc(e, &x.flag, 1));
    RC(env_alloc(e, &e->d_action, N)); RC(env_alloc(e, &e->d_args, 2 * N)); RC(env_alloc(e, &e->d_ao, kNO * N));
    RC(env_alloc(e, &e->d_next, N * d.S)); RC(env_alloc(e, &e->d_status, N)); RC(env_alloc(e, &e->d_pob, N));
    HIPCHK(hipHostMalloc(&e->pinned, N * 4 * (3 + 2 + kNO + (size_t)d.S), hipHostMallocDefault));
    e->rec_read.assign(N, 0);
    memcpy(pin_next(e), first_states_host, N * d.S * sizeof(float));
    HIPCHK(hipMemcpyAsync(e->d_next, pin_next(e), N * d.S * sizeof(float), hipMemcpyHostToDevice, h->stream));
    x.next = e->d_next;
    if (e->f16) {
      RC(env_panels16(e));
      HIPCHK(launch(h->stream, k_env_ext_init<true>, dim3(d.N), dim3(64), d.SP * sizeof(float), EnvArgs<true>{d, env16_of(e, false)}, x));
    } else HIPCHK(launch(h->stream, k_env_ext_init<false>, dim3(d.N), dim3(64), d.SP * sizeof(float), EnvArgs<false>{d}, x));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
  }
  if (e->f16) {
    RC(env_panels16(e));
    HIPCHK(launch(h->stream, k_env_init<true>, dim3(d.N), dim3(64), d.SP * sizeof(float), EnvArgs<true>{d, env16_of(e, false)}));
  } else HIPCHK(launch(h->stream, k_env_init<false>, dim3(d.N), dim3(64), d.SP * sizeof(float), EnvArgs<false>{d}));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

int dqnhip_env_destroy(dqnhip_env_handle e) {
  if (!e) return 0;
  if (e->slack_counted) RO(e->h)->per_env_slack -= (long long)e->cfg.workers * e->cfg.max_steps;
  hipSetDevice(e->h->cfg.device);
  hipStreamSynchronize(e->h->stream);
  for (void* p : e->allocs) hipFree(p);
  if (e->pinned) hipHostFree(e->pinned);
  for (int i = 0; i < 2; ++i) if (e->graph[i]) hipGraphExecDestroy(e->graph[i]);
  delete e;
  return 0;
}

// First tower layer of batched step t+1 (the small-K direct kernel's 32x32 tiles) and the episode flush of step t
// in ONE launch: blocks [0, tiles) are GEMM tiles, the next N blocks are k_env_flush's.  The two parts share no data
// (the layer reads the state panel k_env_step(t) wrote, the flush reads done[] and the episode rows).  A side
// stream was measured first (A/B in one call, 64 workers, S = 68): 48.0 us per step against 33.5 — every
// cross-stream edge of a replayed graph costs more than the 7 us flush it would hide.
static __global__ __launch_bounds__(256) void k_env_l0_flush(const GemmBatch batch, EnvDev e, Ring ring, const DevState* st, double gamma) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  if ((int)blockIdx.x < batch.total_tiles) {
    int pi, tile_p, tile_q;
    tile_of_block(batch, pi, tile_p, tile_q);
    fwd_direct_body<2, 2>(batch.prob[pi], tile_p, tile_q, smem);
    return;
  }
  env_flush_block(e, ring, st, gamma, (int)blockIdx.x - batch.total_tiles, (int)gridDim.x - batch.total_tiles, smem);
}
// one batched env step on the learner's stream: SelectActionGreedily for all workers, then the
// per-worker epsilon draw / GetAction / reward / episode bookkeeping / AddTransitions
static int env_one_step16(dqnhip_env* e);
static int env_one_step(dqnhip_env* e, bool more_follow) {
  if (e->f16) return env_one_step16(e);
  dqnhip_learner* h = e->h;
  EnvDev d = e->d;
  hipStream_t st = h->stream;
  const NetLayout& la = h->la;
  FwdPass fp{DQNHIP_ACTOR, &la, e->acts};
  // 5 launches per batched step at L = 4 inside a sequence: the actor heads ride in k_env_step (the four waves of a
  // worker's block compute its own 10 outputs), the ring bookkeeping in the flush's last block, and the flush itself
  // in the NEXT step's first-layer launch.
  // (beyond a few hundred workers the dedicated head kernel and a separate commit win: one block per head row is
  // slower than the tiled head kernel there, and N arrivals on one counter serialise at ~12 ns each)
  const bool fused = la.dims[la.L] % 4 == 0 && d.N <= 512;
  if (fused) {
    d.head_x = e->acts[la.L]; d.head_h = la.dims[la.L];
    d.head_w = wat(h, DQNHIP_ACTOR, la.hw_off); d.head_b = wat(h, DQNHIP_ACTOR, la.hb_off);
    d.commit_ticket = e->commit_ticket;
  }
  const bool l0_direct = !((la.kp[0] >= 512) && (la.kp[0] % 256 == 0)) && la.dims[1] % 32 == 0 && e->Npad % 32 == 0;
  int first = 0;
  if (e->flush_deferred) {
    // the previous step's flush + this step's first layer (the deferral below is only made when this holds)
    GemmBatch b{}; b.n = 1;
    GemmProblem& p = b.prob[0];
    p.P = wat(h, DQNHIP_ACTOR, la.w_off[0]); p.ldp = la.kp[0];
    p.Q = e->acts[0]; p.ldq = la.kp[0];
    p.C = e->acts[1]; p.ldc = la.kp[1];
    p.Pdim = la.dims[1]; p.Qdim = e->Npad; p.Kred = la.kp[0];
    p.bias = wat(h, DQNHIP_ACTOR, la.b_off[0]); p.relu = 1;
    p.tiles_p = p.Pdim / 32; p.tiles_q = p.Qdim / 32; p.tile_base = 0;
    b.total_tiles = p.tiles_p * p.tiles_q;
    const size_t lds = std::max<size_t>(4 * 2 * 2 * 64 * 16, d.T * sizeof(float));
    HIPCHK(launch(st, k_env_l0_flush, dim3(b.total_tiles + d.N), dim3(256), lds, b, d, RO(h)->ring,
                       (const DevState*)RO(h)->st, h->cfg.gamma));
    e->flush_deferred = false;
    first = 1;
  }
  for (int i = first; i < la.L; ++i) RC(layer_forward(h, st, &fp, 1, e->Npad, i));
  if (!fused) {
    HeadArgs a{}; a.X = e->acts[la.L]; a.ldx = la.dims[la.L]; a.H = la.dims[la.L]; a.rows = e->Npad;
    a.W = wat(h, DQNHIP_ACTOR, la.hw_off); a.b = wat(h, DQNHIP_ACTOR, la.hb_off); a.out16 = d.out16;
    RC((head_forward<kNO, HEAD_ACTOR>(h, st, a)));
  }
  if (e->noise) HIPCHK(launch(st, k_env_step<false, true, EnvNoise>, dim3(d.N), dim3(256), 2 * d.SP * sizeof(float), EnvArgs<false>{d}, e->nz));
  else HIPCHK(launch(st, k_env_step<false>, dim3(d.N), dim3(256), 2 * d.SP * sizeof(float), EnvArgs<false>{d}));
  if (more_follow && fused && l0_direct && !h->timing) { e->flush_deferred = true; return 0; }
  HIPCHK(launch(st, k_env_flush, dim3(d.N), dim3(256), d.T * sizeof(float), d, RO(h)->ring,
                     (const DevState*)RO(h)->st, h->cfg.gamma));
  if (d.commit_ticket == nullptr) {
    HIPCHK(launch(st, k_env_commit, dim3(1), dim3(256), 0, d, RO(h)->ring, RO(h)->st));
  }
  return 0;
}

// the same step in fp16 acting mode: L hgemm tower layers on the actor's fp16 mirror (tower_forward16_on, learner.hip), the heads on
// the fp16 tower top — inside k_env_step<true> up to 512 workers, head_forward with HeadArgs::X16 above — then k_env_step<true>, which
// writes the next fp16 input row itself (no pack launch), and the episode flush as a launch of its own: the deferred form rides in
// the fp32 first-layer launch (k_env_l0_flush), which this mode does not have.  L + 2 launches per step at <= 512 workers (fp32 mode:
// L + 1 inside a sequence), L + 4 above (as fp32 mode).
static int env_one_step16(dqnhip_env* e) {
  dqnhip_learner* h = e->h;
  EnvDev d = e->d;
  hipStream_t st = h->stream;
  const NetLayout& la = h->la;
  const bool fused = la.dims[la.L] % 4 == 0 && d.N <= 512;
  if (fused) {
    d.head_h = la.dims[la.L];
    d.head_w = wat(h, DQNHIP_ACTOR, la.hw_off); d.head_b = wat(h, DQNHIP_ACTOR, la.hb_off);
    d.commit_ticket = e->commit_ticket;
  }
  RC(tower_forward16_on(h, st, DQNHIP_ACTOR, e->p16, e->Npad16));
  if (!fused) {
    HeadArgs a{}; a.X16 = e->p16[la.L]; a.ldx = la.dims[la.L]; a.H = la.dims[la.L]; a.rows = e->Npad;
    a.W = wat(h, DQNHIP_ACTOR, la.hw_off); a.b = wat(h, DQNHIP_ACTOR, la.hb_off); a.out16 = d.out16;
    RC((head_forward<kNO, HEAD_ACTOR>(h, st, a)));
  }
  if (e->noise) HIPCHK(launch(st, k_env_step<true, true, EnvNoise>, dim3(d.N), dim3(256), 2 * d.SP * sizeof(float), EnvArgs<true>{d, env16_of(e, fused)}, e->nz));
  else HIPCHK(launch(st, k_env_step<true>, dim3(d.N), dim3(256), 2 * d.SP * sizeof(float), EnvArgs<true>{d, env16_of(e, fused)}));
  HIPCHK(launch(st, k_env_flush, dim3(d.N), dim3(256), d.T * sizeof(float), d, RO(h)->ring,
                     (const DevState*)RO(h)->st, h->cfg.gamma));
  if (d.commit_ticket == nullptr) {
    HIPCHK(launch(st, k_env_commit, dim3(1), dim3(256), 0, d, RO(h)->ring, RO(h)->st));
  }
  return 0;
}

// the learner's acting precision changed since this handle last looked: the captured steps are those of the other mode
static int env_follow_act_precision(dqnhip_env* e) {
  dqnhip_learner* h = e->h;
  if (e->act_epoch == h->act_epoch) return 0;
  HIPCHK(hipStreamSynchronize(h->stream));
  for (int i = 0; i < 2; ++i) if (e->graph[i]) { HIPCHK(hipGraphExecDestroy(e->graph[i])); e->graph[i] = nullptr; }
  e->graph_failed = false;
  if (h->act_fp16) {
    // the actor's input panel from the fp32 state rows, once; from here on k_env_step<true> keeps it current
    RC(env_panels16(e));
    RC(pack_rows16_launch(h->stream, e->d.cur, e->d.N, e->d.SP, e->d.SP, e->p16[0], e->Npad16, h->k16[0][0]));
  }
  e->f16 = h->act_fp16; e->act_epoch = h->act_epoch;
  return 0;
}

static int env_capture(dqnhip_env* e, int which) {
  dqnhip_learner* h = e->h;
  hipGraph_t graph = nullptr;
  HIPCHK(hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
  int rc = 0;
  const int n = which ? kEnvUnroll : 1;
  for (int s = 0; s < n && !rc; ++s) rc = env_one_step(e, s + 1 < n);
  e->flush_deferred = false;                     // (only left set if a launch failed: the sequence is abandoned)
  hipError_t err = hipStreamEndCapture(h->stream, &graph);
  if (rc) { if (graph) hipGraphDestroy(graph); return rc; }
  if (err != hipSuccess) return fail("hipStreamEndCapture (env): %s", hipGetErrorString(err));
  size_t nodes = 0;
  if (hipGraphGetNodes(graph, nullptr, &nodes) == hipSuccess) e->graph_nodes[which] = (int)nodes;
  err = hipGraphInstantiate(&e->graph[which], graph, nullptr, nullptr, 0);
  hipGraphDestroy(graph);
  if (err != hipSuccess) return fail("hipGraphInstantiate (env): %s", hipGetErrorString(err));
  return 0;
}

int dqnhip_env_step(dqnhip_env_handle e, float epsilon, int32_t n_steps) {
  if (!e) return fail("null env");
  if (e->external) return fail("dqnhip_env_step: this handle takes its states from the caller: use dqnhip_env_act / dqnhip_env_observe");
  if (!(epsilon >= 0.0f && epsilon <= 1.0f)) return fail("Check failed: epsilon >= 0.0 && epsilon <= 1.0");   // src/dqn.cpp:698
  if (n_steps < 1) return fail("n_steps must be >= 1");
  dqnhip_learner* h = e->h;
  RO(h)->epoch += 1;            // episodes may end inside: the ring changes on the device
  HIPCHK(hipSetDevice(h->cfg.device));
  hipStream_t st = h->stream;
  RingUse ring_use(h);
  RC(env_follow_act_precision(e));
  if (e->f16) RC(sync_dirty16(h));          // (outside any capture: a captured step holds the tower launches only)
  HIPCHK(launch(st, k_set_float<0>, dim3(1), dim3(1), 0, e->eps_dev, epsilon));
  // the step is a fixed launch sequence (9 launches at L = 4, ~6 us each when launch-bound): replay it
  // as a hipGraph unless the learner's layers may be re-pointed (sharing) or graphs are off
  const bool use_graph = h->cfg.use_graph && !e->graph_failed && !h->timing && !h->w_owner && !h->ring_owner;
  int s = 0;
  if (use_graph) {
    for (int which = 1; which >= 0; --which) {
      const int n = which ? kEnvUnroll : 1;
      while (n_steps - s >= n) {
        if (!e->graph[which] && env_capture(e, which)) { e->graph_failed = true; break; }
        per_note_append(h, (long long)e->d.N * n);      // (prioritized replay: at most one transition per worker and step reaches the ring)
        HIPCHK(hipGraphLaunch(e->graph[which], st));
        s += n;
      }
      if (e->graph_failed) break;
    }
  }
  for (; s < n_steps; ++s) {
    per_note_append(h, e->d.N);
    const int rc = env_one_step(e, s + 1 < n_steps);
    if (rc) { e->flush_deferred = false; return rc; }
  }
  RO(h)->ring_stale = true;
  return 0;
}

// ---- the external kind: dqnhip_env_act / dqnhip_env_observe ----------------------------------------------------------------------
// A pair is L + 3 launches at L = 4 up to 512 workers (L tower layers, k_env_act with the heads inside, k_env_observe, k_env_flush
// with the commit in its last block), L + 5 above (head_forward and k_env_commit on their own); a NO_RECORD handle has no flush.
// Eager launches: the caller's pointers are kernel arguments.

int dqnhip_env_act_device(dqnhip_env_handle e, float epsilon, int32_t* action_dev, float* args_dev, float* actor_out_dev) {
  if (!e) return fail("null env");
  if (!e->external) return fail("dqnhip_env_act: this handle generates its own states: use dqnhip_env_step");
  if (!action_dev || !args_dev) return fail("null argument");
  if (e->acted) return fail("dqnhip_env_act: the previous act has not been answered by dqnhip_env_observe");
  if (!(epsilon >= 0.0f && epsilon <= 1.0f)) return fail("Check failed: epsilon >= 0.0 && epsilon <= 1.0");   // src/dqn.cpp:698
  dqnhip_learner* h = e->h;
  HIPCHK(hipSetDevice(h->cfg.device));
  hipStream_t st = h->stream;
  RC(env_follow_act_precision(e));
  EnvDev d = e->d;
  const NetLayout& la = h->la;
  // the forward pass and the heads' place are those of env_one_step / env_one_step16: the same launches at the same padded rows
  const bool fused = la.dims[la.L] % 4 == 0 && d.N <= 512;
  if (fused) {
    d.head_h = la.dims[la.L];
    d.head_w = wat(h, DQNHIP_ACTOR, la.hw_off); d.head_b = wat(h, DQNHIP_ACTOR, la.hb_off);
    if (!e->f16) d.head_x = e->acts[la.L];
  }
  HeadArgs ha{}; ha.ldx = la.dims[la.L]; ha.H = la.dims[la.L]; ha.rows = e->Npad;
  ha.W = wat(h, DQNHIP_ACTOR, la.hw_off); ha.b = wat(h, DQNHIP_ACTOR, la.hb_off); ha.out16 = d.out16;
  if (e->f16) {
    RC(sync_dirty16(h));
    RC(tower_forward16_on(h, st, DQNHIP_ACTOR, e->p16, e->Npad16));
    ha.X16 = e->p16[la.L];
  } else {
    FwdPass fp{DQNHIP_ACTOR, &la, e->acts};
    for (int i = 0; i < la.L; ++i) RC(layer_forward(h, st, &fp, 1, e->Npad, i));
    ha.X = e->acts[la.L];
  }
  if (!fused) RC((head_forward<kNO, HEAD_ACTOR>(h, st, ha)));
  EnvExt x = e->x;
  x.epsilon = epsilon; x.out_action = action_dev; x.out_args = args_dev; x.out_ao = actor_out_dev;
  if (e->noise) {
    if (e->f16) HIPCHK(launch(st, k_env_act<true, true, EnvNoise>, dim3(d.N), dim3(256), 0, EnvArgs<true>{d, env16_of(e, fused)}, x, e->nz));
    else HIPCHK(launch(st, k_env_act<false, true, EnvNoise>, dim3(d.N), dim3(256), 0, EnvArgs<false>{d}, x, e->nz));
  } else if (e->f16) HIPCHK(launch(st, k_env_act<true>, dim3(d.N), dim3(256), 0, EnvArgs<true>{d, env16_of(e, fused)}, x));
  else HIPCHK(launch(st, k_env_act<false>, dim3(d.N), dim3(256), 0, EnvArgs<false>{d}, x));
  e->acted = true;
  return 0;
}

int dqnhip_env_act(dqnhip_env_handle e, float epsilon, int32_t* action, float* args, float* actor_out) {
  if (!e || !action || !args) return fail("null argument");
  RC(dqnhip_env_act_device(e, epsilon, e->d_action, e->d_args, actor_out ? e->d_ao : nullptr));
  hipStream_t st = e->h->stream;
  const size_t N = e->d.N;
  HIPCHK(hipMemcpyAsync(pin_action(e), e->d_action, N * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(pin_args(e), e->d_args, 2 * N * 4, hipMemcpyDeviceToHost, st));
  if (actor_out) HIPCHK(hipMemcpyAsync(pin_ao(e), e->d_ao, kNO * N * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  memcpy(action, pin_action(e), N * 4); memcpy(args, pin_args(e), 2 * N * 4);
  if (actor_out) memcpy(actor_out, pin_ao(e), kNO * N * 4);
  return 0;
}

int dqnhip_env_observe_device(dqnhip_env_handle e, const float* next_states_dev, const int32_t* status_dev, const int32_t* player_on_ball_dev) {
  if (!e || !next_states_dev || !status_dev || !player_on_ball_dev) return fail("null argument");
  if (!e->external) return fail("dqnhip_env_observe: this handle generates its own states: use dqnhip_env_step");
  if (!e->acted) return fail("dqnhip_env_observe: no dqnhip_env_act is waiting for its observation");
  dqnhip_learner* h = e->h;
  HIPCHK(hipSetDevice(h->cfg.device));
  hipStream_t st = h->stream;
  EnvDev d = e->d;
  EnvExt x = e->x;
  x.next = next_states_dev; x.status = status_dev; x.pob = player_on_ball_dev; x.step_index = e->observes + 1;
  auto observe = [&]() -> int {
    if (e->noise) {
      if (e->f16) HIPCHK(launch(st, k_env_observe<true, true, EnvNoise>, dim3(d.N), dim3(256), d.SP * sizeof(float), EnvArgs<true>{d, env16_of(e, false)}, x, e->nz));
      else HIPCHK(launch(st, k_env_observe<false, true, EnvNoise>, dim3(d.N), dim3(256), d.SP * sizeof(float), EnvArgs<false>{d}, x, e->nz));
    } else if (e->f16) HIPCHK(launch(st, k_env_observe<true>, dim3(d.N), dim3(256), d.SP * sizeof(float), EnvArgs<true>{d, env16_of(e, false)}, x));
    else HIPCHK(launch(st, k_env_observe<false>, dim3(d.N), dim3(256), d.SP * sizeof(float), EnvArgs<false>{d}, x));
    e->observes += 1; e->acted = false;
    return 0;
  };
  if (!e->record) return observe();   // PlayOneEpisode(update = false): the replay memory, and with it an update chain, is left alone
  RO(h)->epoch += 1;            // episodes may end inside: the ring changes on the device
  RingUse ring_use(h);
  per_note_append(h, d.N);
  if (d.N <= 512) d.commit_ticket = e->commit_ticket;
  RC(observe());
  HIPCHK(launch(st, k_env_flush, dim3(d.N), dim3(256), d.T * sizeof(float), d, RO(h)->ring, (const DevState*)RO(h)->st, h->cfg.gamma));
  if (d.commit_ticket == nullptr) HIPCHK(launch(st, k_env_commit, dim3(1), dim3(256), 0, d, RO(h)->ring, RO(h)->st));
  RO(h)->ring_stale = true;
  return 0;
}

int dqnhip_env_observe(dqnhip_env_handle e, const float* next_states, const int32_t* status, const int32_t* player_on_ball) {
  if (!e || !next_states || !status || !player_on_ball) return fail("null argument");
  if (!e->external) return fail("dqnhip_env_observe: this handle generates its own states: use dqnhip_env_step");
  if (!e->acted) return fail("dqnhip_env_observe: no dqnhip_env_act is waiting for its observation");
  hipStream_t st = e->h->stream;
  const size_t N = e->d.N, S = e->d.S;
  HIPCHK(hipSetDevice(e->h->cfg.device));
  HIPCHK(hipStreamSynchronize(st));           // the previous observe's copies out of the pinned block have run
  memcpy(pin_next(e), next_states, N * S * 4); memcpy(pin_status(e), status, N * 4); memcpy(pin_pob(e), player_on_ball, N * 4);
  HIPCHK(hipMemcpyAsync(e->d_next, pin_next(e), N * S * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(e->d_status, pin_status(e), N * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(e->d_pob, pin_pob(e), N * 4, hipMemcpyHostToDevice, st));
  return dqnhip_env_observe_device(e, e->d_next, e->d_status, e->d_pob);
}

// Exploration noise on or off (cfg NULL).  The captured steps hold the kernels of the other setting and its config as kernel
// arguments: they are dropped, as a change of the acting precision drops them.  Every call zeroes the workers' OU states.
int dqnhip_env_set_noise(dqnhip_env_handle e, const dqnhip_noise_config* cfg) {
  if (!e) return fail("null env");
  dqnhip_learner* h = e->h;
  NoiseCfg c{};
  if (cfg) {
    if (cfg->struct_size != (int32_t)sizeof(dqnhip_noise_config)) return fail("dqnhip_noise_config.struct_size mismatch");
    c.sigma_logits = cfg->sigma_logits; c.sigma_params = cfg->sigma_params; c.theta = cfg->theta; c.clip = cfg->clip;
    c.clamp = cfg->clamp ? 1 : 0; c.seed = cfg->seed;
    char msg[256];
    if (noise_config_check(c, msg, sizeof msg)) return fail("dqnhip_env_set_noise: %s", msg);
  }
  if (e->acted) return fail("dqnhip_env_set_noise: an act is waiting for its observe");
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipStreamSynchronize(h->stream));
  for (int i = 0; i < 2; ++i) if (e->graph[i]) { HIPCHK(hipGraphExecDestroy(e->graph[i])); e->graph[i] = nullptr; }
  e->graph_failed = false;
  const size_t n = (size_t)e->d.N * kAP;
  if (cfg && !e->nz.ou) { RC(env_alloc(e, &e->nz.ou, n)); RC(env_alloc(e, &e->nz.z_last, n)); RC(env_alloc(e, &e->nz.chosen, n)); }
  if (e->nz.ou) {
    HIPCHK(hipMemsetAsync(e->nz.ou, 0, n * sizeof(float), h->stream));
    HIPCHK(hipMemsetAsync(e->nz.z_last, 0, n * sizeof(float), h->stream));
    // "actor_out" before the first noisy step: the greedy rows, what a handle without noise reports
    HIPCHK(hipMemcpyAsync(e->nz.chosen, e->d.out16, n * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  e->nz.cfg = c;
  e->noise = cfg != nullptr;
  return 0;
}
// the sticky status flag of an external handle (src/hfo_game.cpp:124-126 throws "Server Down!"); the stream is idle
static int env_check_flag(dqnhip_env* e) {
  if (!e->external) return 0;
  int flag = 0;
  HIPCHK(hipMemcpy(&flag, e->x.flag, sizeof flag, hipMemcpyDeviceToHost));
  if (flag & 1) return fail("Server Down!");
  if (flag & 2) return fail("dqnhip_env_observe: status out of range (the HFO status values are 0..4)");
  return 0;
}

int dqnhip_env_read_episodes(dqnhip_env_handle e, dqnhip_env_episode* out, int32_t cap, int32_t* n_out, int64_t* dropped) {
  if (!e || !n_out || (cap > 0 && !out)) return fail("null argument");
  *n_out = 0;
  if (!e->external) return fail("dqnhip_env_read_episodes: only a handle of dqnhip_env_create_external keeps episode records");
  if (cap < 0) return fail("cap must be >= 0");
  dqnhip_learner* h = e->h;
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipStreamSynchronize(h->stream));
  RC(env_check_flag(e));
  const size_t N = e->d.N;
  std::vector<unsigned long long> n(N);
  std::vector<dqnhip_env_episode> rec(N * kEnvRecRing);
  HIPCHK(hipMemcpy(n.data(), e->x.rec_n, N * 8, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(rec.data(), e->x.rec, rec.size() * sizeof(dqnhip_env_episode), hipMemcpyDeviceToHost));
  std::vector<dqnhip_env_episode> fresh;
  for (size_t w = 0; w < N; ++w) {
    unsigned long long from = e->rec_read[w];
    if (n[w] - from > (unsigned long long)kEnvRecRing) { e->dropped += (long long)(n[w] - from) - kEnvRecRing; from = n[w] - kEnvRecRing; }
    for (unsigned long long i = from; i < n[w]; ++i) fresh.push_back(rec[w * kEnvRecRing + i % kEnvRecRing]);
    e->rec_read[w] = n[w];
  }
  // every fresh record ended later than every pending one, so sorting the fresh ones keeps the whole queue in (step_index, worker) order
  std::sort(fresh.begin(), fresh.end(), [](const dqnhip_env_episode& a, const dqnhip_env_episode& b) {
    return a.step_index != b.step_index ? a.step_index < b.step_index : a.worker < b.worker; });
  e->pending.insert(e->pending.end(), fresh.begin(), fresh.end());
  int32_t k = 0;
  for (; k < cap && !e->pending.empty(); ++k) { out[k] = e->pending.front(); e->pending.pop_front(); }
  *n_out = k;
  if (dropped) *dropped = e->dropped;
  return 0;
}

int dqnhip_env_stats(dqnhip_env_handle e, int64_t* env_steps, int64_t* episodes, double* reward_sum, int64_t* goals) {
  if (!e) return fail("null env");
  dqnhip_learner* h = e->h;
  HIPCHK(hipSetDevice(h->cfg.device));
  if (e->external) { HIPCHK(hipStreamSynchronize(h->stream)); RC(env_check_flag(e)); }
  const size_t N = e->d.N;
  std::vector<unsigned long long> a(N), b(N), c(N); std::vector<double> r(N);
  HIPCHK(hipMemcpyAsync(a.data(), e->d.n_steps, N * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(b.data(), e->d.n_episodes, N * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(c.data(), e->d.n_goals, N * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(r.data(), e->d.reward_sum, N * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  long long s0 = 0, s1 = 0, s2 = 0; double s3 = 0;
  for (size_t i = 0; i < N; ++i) { s0 += a[i]; s1 += b[i]; s2 += c[i]; s3 += r[i]; }
  if (env_steps) *env_steps = s0; if (episodes) *episodes = s1; if (goals) *goals = s2; if (reward_sum) *reward_sum = s3;
  RingUse ring_use(h);
  return refresh_ring(h);
}

int dqnhip_env_debug_read(dqnhip_env_handle e, const char* name, float* host, size_t count) {
  if (!e || !name || !host) return fail("null argument");
  dqnhip_learner* h = e->h;
  HIPCHK(hipSetDevice(h->cfg.device));
  const size_t N = e->d.N;
  HIPCHK(hipStreamSynchronize(h->stream));
  if (!strcmp(name, "action") || !strcmp(name, "episode_len")) {
    if (count < N) return fail("buffer too small");
    std::vector<int> t(N);
    HIPCHK(hipMemcpy(t.data(), !strcmp(name, "action") ? e->d.act : e->d.len, N * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < N; ++i) host[i] = (float)t[i];
    return 0;
  }
  if (!strcmp(name, "graph_nodes")) {
    // launches of the captured one-step graph and of the captured 16-step graph (0: not captured yet)
    if (count < 2) return fail("buffer too small");
    host[0] = (float)(e->graph[0] ? e->graph_nodes[0] : 0); host[1] = (float)(e->graph[1] ? e->graph_nodes[1] : 0);
    return 0;
  }
  if (!strcmp(name, "truncated")) {
    // episodes that reached max_steps while IN_GAME and were closed as OUT_OF_TIME (external handles; a synthetic one reports 0)
    if (count < 1) return fail("buffer too small");
    unsigned long long total = 0;
    if (e->external) {
      std::vector<unsigned long long> t(N);
      HIPCHK(hipMemcpy(t.data(), e->x.truncated, N * 8, hipMemcpyDeviceToHost));
      for (size_t i = 0; i < N; ++i) total += t[i];
    }
    host[0] = (float)total;
    return 0;
  }
  const float* src = nullptr; size_t n = N;
  if (!strcmp(name, "arg1")) src = e->d.arg1;
  else if (!strcmp(name, "arg2")) src = e->d.arg2;
  else if (!strcmp(name, "reward")) src = e->d.rew;
  else if (!strcmp(name, "state")) {
    if (count < N * h->S) return fail("buffer too small");
    std::vector<float> t(N * e->d.SP);
    HIPCHK(hipMemcpy(t.data(), e->d.cur, t.size() * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < N; ++i) memcpy(host + i * h->S, &t[i * e->d.SP], h->S * 4);
    return 0;
  } else if (!strcmp(name, "actor_out") || !strcmp(name, "greedy_out") || !strcmp(name, "noise_state") || !strcmp(name, "noise_z")) {
    // "actor_out" without noise: the ActorOutput chosen at the last step = last written row of the open episode, or (if the
    // episode just ended) not available any more: report the greedy output instead.  With noise the NOISE kernels keep the chosen
    // row (the noisy greedy row, or the random row) and "greedy_out" is the heads' own output.
    if (count < N * kNO) return fail("buffer too small");
    const bool is_z = !strcmp(name, "noise_z"), is_state = !strcmp(name, "noise_state");
    if ((is_z || is_state) && !e->noise) return fail("env debug buffer '%s': exploration noise is not enabled on this handle (dqnhip_env_set_noise)", name);
    const float* rows = is_z ? e->nz.z_last : is_state ? e->nz.ou : (!strcmp(name, "actor_out") && e->noise) ? e->nz.chosen : e->d.out16;
    std::vector<float> t(N * kAP);
    HIPCHK(hipMemcpy(t.data(), rows, t.size() * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < N; ++i) memcpy(host + i * kNO, &t[i * kAP], kNO * 4);
    return 0;
  } else return fail("unknown env debug buffer '%s'", name);
  if (count < n) return fail("buffer too small");
  HIPCHK(hipMemcpy(host, src, n * 4, hipMemcpyDeviceToHost));
  return 0;
}
}  // extern "C"

