// learner_io.hip — everything of the C-ABI around the update: acting (SelectActions / CriticForward), the replay memory and
// its .replaymemory files, parameter access, multi-agent sharing, introspection, update diagnostics, the replay sweep (include/dqnhip.h).
#include "learner_internal.hip.h"
#include "head_fwd_kernels.hip.h"
#include "io_kernels.hip.h"
#include "per_kernels.hip.h"
#include "diag_kernels.hip.h"
#include "sweep_kernels.hip.h"
#include "state_kernels.hip.h"
#include "snapshot_kernels.hip.h"

using namespace dqnhip;
using namespace dqnhip_host;

extern "C" {

// ---- acting ------------------------------------------------------------------------

static int pack_blocks16(int rows, int k16) { return (rows * ((k16 + 511) / 512) + 3) / 4; }   // 4 waves per block, one per row piece

// fp16 acting (dqnhip_set_act_precision): the forward the update's own passes compute — fp16 input panel, hgemm layers on the
// net's fp16 mirror (tower_forward16_on, learner.hip), the fp32 heads on the fp16 tower top
static int actor_forward16_dev(H* h, int net, const float* states_dev, int n, float* out_dev) {
  const int rows = act16_rows(n);
  RC(ensure_act16(h, rows));
  const NetLayout& l = h->la;
  RC(pack_rows16_launch(h->stream, states_dev, n, h->S, h->S, h->actp16[0], rows, h->k16[0][0]));
  RC(tower_forward16_on(h, h->stream, net, h->actp16, rows));
  HeadArgs a{}; a.X16 = h->actp16[l.L]; a.ldx = l.dims[l.L]; a.H = l.dims[l.L]; a.rows = rows;
  a.W = wat(h, net, l.hw_off); a.b = wat(h, net, l.hb_off); a.out16 = h->actp16_out;
  RC((head_forward<kNO, HEAD_ACTOR>(h, h->stream, a)));
  HIPCHK(launch(h->stream, k_unpack_out, dim3((n * kNO + 255) / 256), dim3(256), 0, (const float*)h->actp16_out, n, out_dev));
  return 0;
}

static int actor_forward_dev(H* h, int net, const float* states_dev, int n, float* out_dev) {
  if (n < 1) return fail("n must be >= 1");
  if (net != DQNHIP_ACTOR && net != DQNHIP_ACTOR_TARGET) return fail("net must be an actor");
  if (h->act_fp16) return actor_forward16_dev(h, net, states_dev, n, out_dev);
  const int rows = round_up(n, 32);
  RC(ensure_act(h, rows));
  const NetLayout& l = h->la;
  float* acts[kMaxL + 1];
  float* p = h->act_buf;
  for (int i = 0; i <= l.L; ++i) { acts[i] = p; p += (size_t)rows * std::max(h->la.kp[i], h->lc.kp[i]); }
  float* out16 = p;
  HIPCHK(launch(h->stream, k_pack_rows, dim3((rows * l.kp[0] + 255) / 256), dim3(256), 0, states_dev, n,
                     h->S, acts[0], rows, l.kp[0]));
  FwdPass fp[1] = {{net, &l, acts}};
  RC(tower_forward(h, h->stream, fp, 1, rows));
  HeadArgs a{}; a.X = acts[l.L]; a.ldx = l.dims[l.L]; a.H = l.dims[l.L]; a.rows = rows;
  a.W = wat(h, net, l.hw_off); a.b = wat(h, net, l.hb_off); a.out16 = out16;
  RC((head_forward<kNO, HEAD_ACTOR>(h, h->stream, a)));
  HIPCHK(launch(h->stream, k_unpack_out, dim3((n * kNO + 255) / 256), dim3(256), 0, (const float*)out16, n, out_dev));
  return 0;
}

int dqnhip_select_actions_device(dqnhip_handle h, const float* states_dev, int32_t n, float* actor_out_dev) {
  if (!h) return fail("null handle");
  HIPCHK(hipSetDevice(h->cfg.device));
  return actor_forward_dev(h, DQNHIP_ACTOR, states_dev, n, actor_out_dev);
}

int dqnhip_select_actions_net(dqnhip_handle h, int32_t net, const float* states_host, int32_t n, float* actor_out_host) {
  if (!h) return fail("null handle");
  if (n < 1) return fail("n must be >= 1");
  HIPCHK(hipSetDevice(h->cfg.device));
  const size_t sb = (size_t)n * h->S * sizeof(float), ob = (size_t)n * kNO * sizeof(float);
  RC(ensure_stage(h, round_up_z(sb, 256) + ob));
  float* sdev = (float*)h->stage_dev;
  float* odev = (float*)((char*)h->stage_dev + round_up_z(sb, 256));
  HIPCHK(hipMemcpyAsync(sdev, states_host, sb, hipMemcpyHostToDevice, h->stream));
  RC(actor_forward_dev(h, net, sdev, n, odev));
  HIPCHK(hipMemcpyAsync(actor_out_host, odev, ob, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

int dqnhip_select_actions(dqnhip_handle h, const float* states_host, int32_t n, float* actor_out_host) {
  return dqnhip_select_actions_net(h, DQNHIP_ACTOR, states_host, n, actor_out_host);
}

static int critic_forward16(H* h, int net, const float* states_host, const float* actor_out_host, int n, float* q_host) {
  const int rows = act16_rows(n);
  const size_t sb = round_up_z((size_t)n * h->S * sizeof(float), 256), ab = round_up_z((size_t)n * kNO * sizeof(float), 256);
  RC(ensure_stage(h, sb + ab));
  float* sdev = (float*)h->stage_dev;
  float* adev = (float*)((char*)h->stage_dev + sb);
  HIPCHK(hipMemcpyAsync(sdev, states_host, (size_t)n * h->S * sizeof(float), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(adev, actor_out_host, (size_t)n * kNO * sizeof(float), hipMemcpyHostToDevice, h->stream));
  RC(ensure_act16(h, rows));
  const NetLayout& l = h->lc;
  HIPCHK(launch(h->stream, k_pack_critic16, dim3(pack_blocks16(rows, h->k16[1][0])), dim3(256), 0,
                Pack16Args{sdev, adev, n, h->S, h->S, h->actp16[0], rows, h->k16[1][0]}));
  RC(tower_forward16_on(h, h->stream, net, h->actp16, rows));
  HeadArgs a{}; a.X16 = h->actp16[l.L]; a.ldx = l.dims[l.L]; a.H = l.dims[l.L]; a.rows = rows;
  a.W = wat(h, net, l.hw_off); a.b = wat(h, net, l.hb_off); a.q = h->actp16_out;      // [rows] floats of the [rows][kAP + 1] scratch
  RC((head_forward<1, HEAD_Q>(h, h->stream, a)));
  HIPCHK(hipMemcpyAsync(q_host, h->actp16_out, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

int dqnhip_critic_forward(dqnhip_handle h, int32_t net, const float* states_host, const float* actor_out_host,
                          int32_t n, float* q_host) {
  if (!h) return fail("null handle");
  if (n < 1) return fail("n must be >= 1");
  if (net != DQNHIP_CRITIC && net != DQNHIP_CRITIC_TARGET) return fail("net must be a critic");
  HIPCHK(hipSetDevice(h->cfg.device));
  if (h->act_fp16) return critic_forward16(h, net, states_host, actor_out_host, n, q_host);
  const int rows = round_up(n, 32);
  const size_t sb = round_up_z((size_t)n * h->S * sizeof(float), 256), ab = round_up_z((size_t)n * kNO * sizeof(float), 256);
  RC(ensure_stage(h, sb + ab + (size_t)rows * sizeof(float)));
  float* sdev = (float*)h->stage_dev;
  float* adev = (float*)((char*)h->stage_dev + sb);
  float* qdev = (float*)((char*)h->stage_dev + sb + ab);
  HIPCHK(hipMemcpyAsync(sdev, states_host, (size_t)n * h->S * sizeof(float), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(adev, actor_out_host, (size_t)n * kNO * sizeof(float), hipMemcpyHostToDevice, h->stream));
  RC(ensure_act(h, rows));
  const NetLayout& l = h->lc;
  float* acts[kMaxL + 1];
  float* p = h->act_buf;
  for (int i = 0; i <= l.L; ++i) { acts[i] = p; p += (size_t)rows * std::max(h->la.kp[i], h->lc.kp[i]); }
  HIPCHK(launch(h->stream, k_pack_critic, dim3((rows * l.kp[0] + 255) / 256), dim3(256), 0, (const float*)sdev,
                     (const float*)adev, n, h->S, acts[0], rows, l.kp[0]));
  FwdPass fp[1] = {{net, &l, acts}};
  RC(tower_forward(h, h->stream, fp, 1, rows));
  HeadArgs a{}; a.X = acts[l.L]; a.ldx = l.dims[l.L]; a.H = l.dims[l.L]; a.rows = rows;
  a.W = wat(h, net, l.hw_off); a.b = wat(h, net, l.hb_off); a.q = qdev;
  RC((head_forward<1, HEAD_Q>(h, h->stream, a)));
  HIPCHK(hipMemcpyAsync(q_host, qdev, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

int dqnhip_set_act_precision(dqnhip_handle h, int32_t precision) {
  if (!h) return fail("null handle");
  if (precision != DQNHIP_FP32 && precision != DQNHIP_FP16) return fail("act precision must be DQNHIP_FP32 or DQNHIP_FP16 (got %d)", precision);
  if (precision == DQNHIP_FP16 && !h->fp16)
    return fail("act precision DQNHIP_FP16 needs a learner created with precision = DQNHIP_FP16 (this one has precision = DQNHIP_FP32: no fp16 weight mirrors)");
  const bool on = precision == DQNHIP_FP16;
  if (on != h->act_fp16) { h->act_fp16 = on; h->act_epoch += 1; }     // (env handles compare the epoch; the update path reads neither)
  return 0;
}

int dqnhip_get_act_precision(dqnhip_handle h, int32_t* precision) {
  if (!h || !precision) return fail("null argument");
  *precision = h->act_fp16 ? DQNHIP_FP16 : DQNHIP_FP32;
  return 0;
}

// ---- replay memory -------------------------------------------------------------------

static int add_dev(H* h, const float* s, const float* a, const float* r, const float* mc, const float* nx,
                   const uint8_t* term, int n, int single) {
  RO(h)->epoch += 1;          // (dqnhip_update_chained: whatever a rider gathered ahead is stale)
  // n == 0 is AddTransitions of an empty vector: `while (size() + 0 >= capacity) pop_front()` (src/dqn.cpp:776) still evicts
  // one transition from a full deque — only the bookkeeping runs
  if (n < 0 || (n == 0 && single != 0)) return fail("n must be >= 1");
  RingUse ring_use(h);
  RC(refresh_ring(h));
  const long long cap = RO(h)->ring.cap;
  if (single == 0 && n >= cap) return fail("AddTransitions: batch of %d does not fit capacity %lld (the reference would pop an empty deque)", n, cap);
  if (single == 2 && RO(h)->h_size + n > cap) return fail("LoadReplayMemory: %lld transitions exceed the capacity %lld", RO(h)->h_size + n, cap);
  per_note_append(h, n);      // (prioritized replay: the tree is brought in step first if this call could make the arithmetic ambiguous)
  HIPCHK(launch(h->stream, k_add_transitions, dim3(std::max(1, (n + 3) / 4)), dim3(256), 0, RO(h)->ring, RO(h)->st, s, a, r, mc, nx,
                     term, n, single, RO(h)->done_counter));
  // host mirror of the same deque arithmetic (src/dqn.cpp:768-781)
  if (single == 2) { }
  else if (single) { if (RO(h)->h_size == cap) { RO(h)->h_head = (RO(h)->h_head + 1) % cap; RO(h)->h_size -= 1; } }
  else {
    long long pops = RO(h)->h_size + n - cap + 1;
    pops = std::max(0LL, std::min(pops, RO(h)->h_size));
    RO(h)->h_head = (RO(h)->h_head + pops) % cap; RO(h)->h_size -= pops;
  }
  RO(h)->h_size += n;
  return 0;
}

int dqnhip_add_transitions_device(dqnhip_handle h, const float* states, const float* actor_out, const float* rewards,
                                  const float* on_policy_targets, const float* next_states, const uint8_t* terminal,
                                  int32_t n) {
  if (!h) return fail("null handle");
  HIPCHK(hipSetDevice(h->cfg.device));
  return add_dev(h, states, actor_out, rewards, on_policy_targets, next_states, terminal, n, 0);
}

static int add_host(H* h, const float* s, const float* a, const float* r, const float* mc, const float* nx,
                    const uint8_t* term, int n, int single) {
  if (!h) return fail("null handle");
  if (n < 0 || (n == 0 && single != 0)) return fail("n must be >= 1");
  HIPCHK(hipSetDevice(h->cfg.device));
  if (n == 0) return add_dev(h, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0);      // empty AddTransitions: eviction only
  if (!s || !a || !r || !mc || !term) return fail("null input array");
  const size_t sb = round_up_z((size_t)n * h->S * 4, 256), ab = round_up_z((size_t)n * kNO * 4, 256), vb = round_up_z((size_t)n * 4, 256);
  // staging is reused: wait for the previous scatter to drain before overwriting
  HIPCHK(hipStreamSynchronize(h->stream));
  RC(ensure_stage(h, 2 * sb + ab + 3 * vb));
  char* base = (char*)h->stage_dev;
  float* ds = (float*)base; float* dn = (float*)(base + sb); float* da = (float*)(base + 2 * sb);
  float* dr = (float*)(base + 2 * sb + ab); float* dm = (float*)(base + 2 * sb + ab + vb);
  uint8_t* dt = (uint8_t*)(base + 2 * sb + ab + 2 * vb);
  HIPCHK(hipMemcpyAsync(ds, s, (size_t)n * h->S * 4, hipMemcpyHostToDevice, h->stream));
  if (nx) HIPCHK(hipMemcpyAsync(dn, nx, (size_t)n * h->S * 4, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(da, a, (size_t)n * kNO * 4, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(dr, r, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(dm, mc, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(dt, term, (size_t)n, hipMemcpyHostToDevice, h->stream));
  return add_dev(h, ds, da, dr, dm, nx ? dn : nullptr, dt, n, single);
}

int dqnhip_add_transitions(dqnhip_handle h, const float* states, const float* actor_out, const float* rewards,
                           const float* on_policy_targets, const float* next_states, const uint8_t* terminal, int32_t n) {
  return add_host(h, states, actor_out, rewards, on_policy_targets, next_states, terminal, n, 0);
}

int dqnhip_add_transition(dqnhip_handle h, const float* state, const float* actor_out, float reward,
                          float on_policy_target, const float* next_state, uint8_t terminal) {
  return add_host(h, state, actor_out, &reward, &on_policy_target, next_state, &terminal, 1, 1);
}

int dqnhip_label_transitions(double gamma, const float* rewards, int32_t n, float* mc) {
  if (n < 1) return fail("Need at least one transition to label.");   // CHECK_GT, src/dqn.cpp:784
  if (!rewards || !mc) return fail("null array");
  mc[n - 1] = rewards[n - 1];
  for (int i = n - 2; i >= 0; --i) mc[i] = (float)((double)rewards[i] + gamma * (double)mc[i + 1]);
  return 0;
}

int dqnhip_memory_size(dqnhip_handle h, int32_t* size) {
  if (!h || !size) return fail("null argument");
  HIPCHK(hipSetDevice(h->cfg.device));
  RingUse ring_use(h);
  RC(refresh_ring(h));
  *size = (int32_t)RO(h)->h_size;
  return 0;
}

int dqnhip_clear_memory(dqnhip_handle h) {
  if (!h) return fail("null handle");
  RO(h)->epoch += 1;
  HIPCHK(hipSetDevice(h->cfg.device));
  RingUse ring_use(h);
  HIPCHK(hipMemsetAsync(RO(h)->st, 0, 2 * sizeof(int), h->stream));   // ring_head, ring_size
  RO(h)->h_head = 0; RO(h)->h_size = 0; RO(h)->ring_stale = false;
  RC(per_clear(h));
  return 0;
}


// caller holds the RingUse of h and has refreshed (head,size)
static int read_memory_impl(H* h, int32_t first, int32_t n, float* states, float* actor_out, float* rewards,
                            float* on_policy_targets, float* next_states, uint8_t* terminal) {
  if (n < 1 || first < 0 || (long long)first + n > RO(h)->h_size) return fail("read_memory range [%d,%d) outside [0,%lld)", first, first + n, RO(h)->h_size);
  const size_t sb = round_up_z((size_t)n * h->S * 4, 256), ab = round_up_z((size_t)n * kNO * 4, 256), vb = round_up_z((size_t)n * 4, 256);
  HIPCHK(hipStreamSynchronize(h->stream));
  RC(ensure_stage(h, 2 * sb + ab + 3 * vb));
  char* base = (char*)h->stage_dev;
  float* ds = (float*)base; float* dn = (float*)(base + sb); float* da = (float*)(base + 2 * sb);
  float* dr = (float*)(base + 2 * sb + ab); float* dm = (float*)(base + 2 * sb + ab + vb);
  uint8_t* dt = (uint8_t*)(base + 2 * sb + ab + 2 * vb);
  HIPCHK(launch(h->stream, k_read_memory, dim3((n + 3) / 4), dim3(256), 0, RO(h)->ring, (const DevState*)RO(h)->st, first, n,
                     ds, da, dr, dm, dn, dt));
  if (states) HIPCHK(hipMemcpyAsync(states, ds, (size_t)n * h->S * 4, hipMemcpyDeviceToHost, h->stream));
  if (next_states) HIPCHK(hipMemcpyAsync(next_states, dn, (size_t)n * h->S * 4, hipMemcpyDeviceToHost, h->stream));
  if (actor_out) HIPCHK(hipMemcpyAsync(actor_out, da, (size_t)n * kNO * 4, hipMemcpyDeviceToHost, h->stream));
  if (rewards) HIPCHK(hipMemcpyAsync(rewards, dr, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
  if (on_policy_targets) HIPCHK(hipMemcpyAsync(on_policy_targets, dm, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
  if (terminal) HIPCHK(hipMemcpyAsync(terminal, dt, (size_t)n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

int dqnhip_read_memory(dqnhip_handle h, int32_t first, int32_t n, float* states, float* actor_out, float* rewards,
                       float* on_policy_targets, float* next_states, uint8_t* terminal) {
  if (!h) return fail("null handle");
  HIPCHK(hipSetDevice(h->cfg.device));
  RingUse ring_use(h);
  RC(refresh_ring(h));
  return read_memory_impl(h, first, n, states, actor_out, rewards, on_policy_targets, next_states, terminal);
}

// DQN::SampleStatesFromMemory (src/dqn.cpp:511-523): n states of uniformly sampled transitions.
// idx_host = the explicit form of SampleTransitionsFromMemory (as in dqnhip_update); NULL draws on
// the device from the counter-based generator (its own key stream, one counter tick per call).
int dqnhip_sample_states(dqnhip_handle h, const int32_t* idx_host, int32_t n, float* states_host) {
  if (!h || !states_host) return fail("null argument");
  if (n < 1) return fail("n must be >= 1");
  HIPCHK(hipSetDevice(h->cfg.device));
  RingUse ring_use(h);
  RC(refresh_ring(h));
  const long long size = RO(h)->h_size;
  if (size < 1) return fail("replay memory is empty");
  const size_t ib = round_up_z((size_t)n * sizeof(int), 256), sb = (size_t)n * h->S * sizeof(float);
  HIPCHK(hipStreamSynchronize(h->stream));
  RC(ensure_stage(h, ib + sb));
  int* di = (int*)h->stage_dev; float* ds = (float*)((char*)h->stage_dev + ib);
  if (idx_host) {
    for (int i = 0; i < n; ++i)
      if (idx_host[i] < 0 || idx_host[i] >= size) return fail("sampled index %d = %d out of range [0,%lld)", i, idx_host[i], size);
    HIPCHK(hipMemcpyAsync(di, idx_host, (size_t)n * sizeof(int), hipMemcpyHostToDevice, h->stream));
  }
  HIPCHK(launch(h->stream, k_sample_states, dim3((n + 3) / 4), dim3(256), 0, RO(h)->ring, (const DevState*)RO(h)->st,
                     idx_host ? (const int*)di : (const int*)nullptr, sample_key(h) ^ 0x5354415445535F5Full, h->sample_states_calls, n, ds));
  if (!idx_host) h->sample_states_calls += 1;
  HIPCHK(hipMemcpyAsync(states_host, ds, sb, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

// getActorOutput (src/dqn.cpp:719-732): the first `batch_size` rows of an actor's output blobs as
// left by its last forward — here the last update's minibatch forward (ACTOR: mu(s), ACTOR_TARGET: mu'(s')).
int dqnhip_get_actor_output(dqnhip_handle h, int32_t net, int32_t batch_size, float* actor_out_host) {
  if (!h || !actor_out_host) return fail("null argument");
  if (net != DQNHIP_ACTOR && net != DQNHIP_ACTOR_TARGET) return fail("net must be an actor");
  if (batch_size < 1 || batch_size > h->B) return fail("batch_size %d outside [1, %d]", batch_size, h->B);
  HIPCHK(hipSetDevice(h->cfg.device));
  std::vector<float> tmp((size_t)batch_size * kAP);
  HIPCHK(hipMemcpyAsync(tmp.data(), net == DQNHIP_ACTOR ? h->aout16 : h->aout_t16, tmp.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  for (int r = 0; r < batch_size; ++r) memcpy(actor_out_host + (size_t)r * kNO, &tmp[(size_t)r * kAP], kNO * sizeof(float));
  return 0;
}

// Sum the gradient arenas (4-float tails included) of n co-located learners of one data-parallel
// group in rank order and leave the sum in every one of them: the exchange step of
// dqnhip_update_phase for learners that share a device (multi-agent layouts, and the one-GPU parity
// test of the dp_world > 1 code path).  Cross-device groups use dqnhip_dp_* (RCCL).
int dqnhip_reduce_gradients_local(dqnhip_handle* hs, int32_t n, int32_t net) {
  if (!hs || n < 1 || n > 8) return fail("reduce_gradients_local: 1..8 learners");
  if (net != DQNHIP_ACTOR && net != DQNHIP_CRITIC) return fail("net must be ACTOR or CRITIC");
  LocalReduce a{}; a.n = n;
  for (int i = 0; i < n; ++i) {
    if (!hs[i]) return fail("null handle");
    if (hs[i]->cfg.device != hs[0]->cfg.device || !same_nets(hs[i], hs[0])) return fail("reduce_gradients_local: learners must share a device and a shape");
    a.g[i] = hs[i]->g[net];
  }
  a.n4 = (layout_of(hs[0], net).arena + 4) / 4;
  HIPCHK(hipSetDevice(hs[0]->cfg.device));
  for (int i = 1; i < n; ++i) HIPCHK(hipStreamSynchronize(hs[i]->stream));   // their phase must be complete
  HIPCHK(launch(hs[0]->stream, k_local_reduce, dim3(1024), dim3(256), 0, a));
  HIPCHK(hipStreamSynchronize(hs[0]->stream));
  return 0;
}

// ---- .replaymemory files (src/dqn.cpp:1146-1226) --------------------------------------------
int dqnhip_snapshot_replay_memory(dqnhip_handle h, const char* filename) {
  if (!h || !filename) return fail("null argument");
  RC(snapshot_async_join(h, "dqnhip_snapshot_replay_memory"));
  HIPCHK(hipSetDevice(h->cfg.device));
  // one RingUse for the whole file: with a shared ring another agent's AddTransitions must not
  // move the head between chunks (the file would hold shifted / duplicated transitions)
  RingUse ring_use(h);
  RC(refresh_ring(h));
  gzFile f = gzopen(filename, "wb");
  if (!f) return fail("cannot open %s for writing", filename);
  const int32_t n = (int32_t)RO(h)->h_size;
  const size_t S = h->S;
  bool ok = gzwrite(f, &n, sizeof n) == (int)sizeof n;
  const int chunk = 65536;
  std::vector<float> s((size_t)chunk * S), a((size_t)chunk * kNO), r(chunk), mc(chunk);
  std::vector<uint8_t> term(chunk), rec;
  for (int first = 0; first < n && ok; first += chunk) {
    const int m = std::min(chunk, n - first);
    if (read_memory_impl(h, first, m, s.data(), a.data(), r.data(), mc.data(), nullptr, term.data())) { gzclose(f); return 1; }
    const size_t rb = S * 4 + kNO * 4 + 4 + 4 + 1;
    rec.resize((size_t)m * rb);
    for (int i = 0; i < m; ++i) {
      uint8_t* p = &rec[(size_t)i * rb];
      memcpy(p, &s[(size_t)i * S], S * 4); p += S * 4;
      memcpy(p, &a[(size_t)i * kNO], kNO * 4); p += kNO * 4;     // sizeof(ActorOutput)
      memcpy(p, &r[i], 4); p += 4;
      memcpy(p, &mc[i], 4); p += 4;
      *p = term[i] ? 1 : 0;                                       // sizeof(bool) == 1
    }
    ok = gzwrite(f, rec.data(), (unsigned)rec.size()) == (int)rec.size();
  }
  if (gzclose(f) != Z_OK || !ok) return fail("short write to %s", filename);
  return 0;
}

int dqnhip_load_replay_memory(dqnhip_handle h, const char* filename) {
  if (!h || !filename) return fail("null argument");
  RC(snapshot_async_join(h, "dqnhip_load_replay_memory"));
  RO(h)->epoch += 1;
  HIPCHK(hipSetDevice(h->cfg.device));
  gzFile f = gzopen(filename, "rb");
  if (!f) return fail("Invalid file: %s", filename);              // CHECK(is_regular_file), src/dqn.cpp:1181
  int32_t n = 0;
  if (gzread(f, &n, sizeof n) != (int)sizeof n || n < 0) { gzclose(f); return fail("%s: bad header", filename); }
  if (n > RO(h)->ring.cap) { gzclose(f); return fail("%s holds %d transitions, capacity is %d", filename, n, RO(h)->ring.cap); }
  RC(dqnhip_clear_memory(h));
  const size_t S = h->S, rb = S * 4 + kNO * 4 + 4 + 4 + 1;
  const int chunk = 65536;
  // one record of look-ahead: next state of the last row of a chunk is the first state of the next
  std::vector<uint8_t> rec((size_t)(chunk + 1) * rb);
  std::vector<float> s((size_t)chunk * S), nx((size_t)chunk * S), a((size_t)chunk * kNO), r(chunk), mc(chunk);
  std::vector<uint8_t> term(chunk);
  int have = 0;                       // records buffered in rec
  int done = 0;
  while (done < n) {
    const int want = std::min(chunk + 1, n - done) - have;
    if (want > 0) {
      const int got = gzread(f, &rec[(size_t)have * rb], (unsigned)((size_t)want * rb));
      if (got != (int)((size_t)want * rb)) { gzclose(f); return fail("%s: truncated", filename); }
      have += want;
    }
    const int m = std::min(chunk, n - done);
    for (int i = 0; i < m; ++i) {
      const uint8_t* p = &rec[(size_t)i * rb];
      memcpy(&s[(size_t)i * S], p, S * 4); p += S * 4;
      memcpy(&a[(size_t)i * kNO], p, kNO * 4); p += kNO * 4;
      memcpy(&r[i], p, 4); p += 4;
      memcpy(&mc[i], p, 4); p += 4;
      bool t = *p != 0;
      const bool has_next = done + i + 1 < n;
      if (!t && !has_next) t = true;                              // trailing non-terminal: next stays none
      term[i] = t ? 1 : 0;
      if (!t) memcpy(&nx[(size_t)i * S], &rec[(size_t)(i + 1) * rb], S * 4);
      else memset(&nx[(size_t)i * S], 0, S * 4);
    }
    if (add_host(h, s.data(), a.data(), r.data(), mc.data(), nx.data(), term.data(), m, 2)) { gzclose(f); return 1; }
    // keep the look-ahead record as the first record of the next chunk
    if (have > m) memmove(&rec[0], &rec[(size_t)m * rb], rb);
    have -= m;
    done += m;
  }
  gzclose(f);
  return 0;
}


// ---- prioritized replay (include/dqnhip.h; the kernels and the tree's definition: per_kernels.hip.h) -----------------------------------

}  // extern "C"

namespace dqnhip_host {

static PerTree per_tree(const PerHost* p) {
  PerTree t{};
  for (int k = 0; k < kPerMaxLevels; ++k) { t.lvl[k] = p->tree.lvl[k]; t.n[k] = p->tree.n[k]; }
  t.levels = p->tree.levels;
  return t;
}
int per_refuse(const H* h, const char* what) {
  return h->per ? fail("%s: not available on a learner with prioritized replay (dqnhip_per_enable) in this version", what) : 0;
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
// dqnhip_save_state / dqnhip_load_state (learner_state.hip, which launches nothing and does not see PerDev)
int per_read_p_max(H* h, float* p_max) {
  HIPCHK(hipMemcpyAsync(p_max, &((PerDev*)h->per->dev)->p_max, sizeof *p_max, hipMemcpyDeviceToHost, h->stream));
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
  if (h->ring_owner || h->sharers || h->ring_shared) return fail("dqnhip_per_enable: prioritized replay on a learner that shares a replay memory is not supported in this version");
  if (h->cfg.dp_world > 1 || h->comm || h->dp_half || h->dp_shard) return fail("dqnhip_per_enable: prioritized replay on a data-parallel learner (dp_world > 1, dqnhip_dp_init) is not supported in this version");
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

// brings the tree in step with the ring; the caller holds no RingUse (a prioritized learner shares no ring)
static int per_ready(dqnhip_handle h, const char* what) {
  if (!h) return fail("%s: null handle", what);
  if (!h->per) return fail("%s: prioritized replay is not enabled on this learner (dqnhip_per_enable)", what);
  HIPCHK(hipSetDevice(h->cfg.device));
  RC(per_sync_if_needed(h));
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

// ---- n-step returns (include/dqnhip.h; k_gather_n: small_kernels.hip.h, launched by learner.hip; k_nstep_validate: io_kernels.hip.h) ----

}  // extern "C"

namespace dqnhip_host {

int nstep_refuse(const H* h, const char* what) {
  return h->nstep ? fail("%s: not available on a learner with n-step returns (dqnhip_nstep_enable) in this version", what) : 0;
}
int smooth_refuse(const H* h, const char* what) {
  return h->tnoise ? fail("%s: not available on a learner with target smoothing (dqnhip_target_noise_enable) in this version", what) : 0;
}
void smooth_free(H* h) {
  TargetNoiseHost* p = h->tnoise;
  if (!p) return;
  hipFree(p->smoothed16); hipFree(p->z16); hipFree(p->counter);
  delete p;
  h->tnoise = nullptr;
}
void nstep_free(H* h) {
  NstepHost* p = h->nstep;
  if (!p) return;
  hipFree(p->disc); hipFree(p->steps); hipFree(p->viol);
  delete p;
  h->nstep = nullptr;
}

}  // namespace dqnhip_host

extern "C" {

int dqnhip_nstep_enable(dqnhip_handle h, int32_t n) {
  if (!h) return fail("dqnhip_nstep_enable: null handle (n-step returns are enabled on an existing learner)");
  if (n < 1 || n > kNstepMax) return fail("dqnhip_nstep_enable: n-step returns take n in [1, %d] (got %d)", kNstepMax, n);
  if (h->cfg.dp_world > 1 || h->comm || h->dp_half || h->dp_shard) return fail("dqnhip_nstep_enable: n-step returns on a data-parallel learner (dp_world > 1, dqnhip_dp_init) are not supported in this version");
  if (h->next_phase != 0) return fail("dqnhip_nstep_enable: a phased update is in progress (next phase %d)", h->next_phase);
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (!h->nstep) {
    NstepHost* p = new NstepHost();
    h->nstep = p;               // (from here on nstep_free releases whatever was allocated)
    const size_t B = h->B;
    auto alloc = [&](void** d, size_t bytes) -> int { HIPCHK(hipMalloc(d, bytes)); HIPCHK(hipMemset(*d, 0, bytes)); return 0; };
    if (alloc((void**)&p->disc, B * sizeof(double)) || alloc((void**)&p->steps, B * sizeof(int)) || alloc((void**)&p->viol, 2 * sizeof(unsigned long long))) { nstep_free(h); return 1; }
  }
  h->nstep->n = n;
  h->epoch += 1;
  drop_graphs(h);
  return 0;
}

// ---- target policy smoothing (include/dqnhip.h; k_target_smooth: head_kernels.hip.h, launched by learner.hip) ----
int dqnhip_target_noise_enable(dqnhip_handle h, const dqnhip_noise_config* cfg) {
  if (!h) return fail("dqnhip_target_noise_enable: null handle (target smoothing is enabled on an existing learner)");
  if (!cfg) { h->epoch += 1; HIPCHK(hipSetDevice(h->cfg.device)); HIPCHK(hipStreamSynchronize(h->stream)); smooth_free(h); drop_graphs(h); return 0; }
  if (cfg->struct_size != (int32_t)sizeof(dqnhip_noise_config)) return fail("dqnhip_target_noise_enable: dqnhip_noise_config.struct_size mismatch");
  NoiseCfg c{};
  c.sigma_logits = cfg->sigma_logits; c.sigma_params = cfg->sigma_params; c.theta = cfg->theta; c.clip = cfg->clip;
  c.clamp = cfg->clamp ? 1 : 0; c.seed = cfg->seed;
  char msg[256];
  if (noise_config_check(c, msg, sizeof msg)) return fail("dqnhip_target_noise_enable: %s", msg);
  if (c.theta != 1.0f) return fail("dqnhip_target_noise_enable: target smoothing draws white noise: theta must be 1 (got %g)", (double)c.theta);
  if (h->fp16) return fail("dqnhip_target_noise_enable: target smoothing on a learner with precision = DQNHIP_FP16 is not supported in this version");
  if (h->cfg.dp_world > 1 || h->comm || h->dp_half || h->dp_shard) return fail("dqnhip_target_noise_enable: target smoothing on a data-parallel learner (dp_world > 1, dqnhip_dp_init) is not supported in this version");
  if (h->w_owner || h->ring_owner || h->shared_fl[0] || h->shared_fl[1] || h->sharers) return fail("dqnhip_target_noise_enable: target smoothing on a learner that shares parameters or its replay memory is not supported in this version");
  if (h->next_phase != 0) return fail("dqnhip_target_noise_enable: a phased update is in progress (next phase %d)", h->next_phase);
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (!h->tnoise) {
    TargetNoiseHost* p = new TargetNoiseHost();
    h->tnoise = p;              // (from here on smooth_free releases whatever was allocated)
    const size_t n = (size_t)h->B * kAP * sizeof(float);
    auto alloc = [&](void** d, size_t bytes) -> int { HIPCHK(hipMalloc(d, bytes)); HIPCHK(hipMemset(*d, 0, bytes)); return 0; };
    if (alloc((void**)&p->smoothed16, n) || alloc((void**)&p->z16, n) || alloc((void**)&p->counter, sizeof(unsigned long long))) { smooth_free(h); return 1; }
  }
  h->tnoise->cfg = c;
  h->epoch += 1;
  drop_graphs(h);
  return 0;
}
int dqnhip_target_noise_get(dqnhip_handle h, int32_t* enabled, dqnhip_noise_config* cfg) {
  if (!h || !enabled) return fail("dqnhip_target_noise_get: null argument");
  *enabled = h->tnoise ? 1 : 0;
  if (cfg && h->tnoise) {
    const NoiseCfg& c = h->tnoise->cfg;
    *cfg = dqnhip_noise_config{(int32_t)sizeof(dqnhip_noise_config), c.clamp, c.sigma_logits, c.sigma_params, c.theta, c.clip, c.seed};
  }
  return 0;
}

int dqnhip_nstep_get(dqnhip_handle h, int32_t* n) {
  if (!h || !n) return fail("dqnhip_nstep_get: null argument");
  *n = h->nstep ? h->nstep->n : 0;
  return 0;
}

static int nstep_ready(dqnhip_handle h, const char* what, const char* name, const void* host) {
  if (!h || !name || !host) return fail("%s: null argument", what);
  if (!h->nstep) return fail("%s: n-step returns are not enabled on this learner (dqnhip_nstep_enable)", what);
  HIPCHK(hipSetDevice(h->cfg.device));
  return 0;
}
int dqnhip_nstep_debug_read(dqnhip_handle h, const char* name, float* host, size_t count) {
  RC(nstep_ready(h, "dqnhip_nstep_debug_read", name, host));
  const size_t B = h->B;
  const bool is_steps = !strcmp(name, "steps");
  if (!is_steps && strcmp(name, "reward")) return fail("dqnhip_nstep_debug_read: unknown buffer '%s' (reward|steps; \"disc\" is a double: dqnhip_nstep_debug_read_f64)", name);
  if (count < B) return fail("buffer too small for '%s': %zu < %zu", name, count, B);
  HIPCHK(hipMemcpyAsync(host, is_steps ? (const void*)h->nstep->steps : (const void*)h->mb_reward, B * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (is_steps) for (size_t i = 0; i < B; ++i) { int v; memcpy(&v, &host[i], sizeof v); host[i] = (float)v; }
  return 0;
}
int dqnhip_nstep_debug_read_f64(dqnhip_handle h, const char* name, double* host, size_t count) {
  RC(nstep_ready(h, "dqnhip_nstep_debug_read_f64", name, host));
  const size_t B = h->B;
  if (strcmp(name, "disc")) return fail("dqnhip_nstep_debug_read_f64: unknown buffer '%s' (disc)", name);
  if (count < B) return fail("buffer too small for '%s': %zu < %zu", name, count, B);
  HIPCHK(hipMemcpyAsync(host, h->nstep->disc, B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

int dqnhip_nstep_validate(dqnhip_handle h, int32_t first, int32_t n, int64_t* violations, int32_t* first_bad) {
  if (!h) return fail("dqnhip_nstep_validate: null handle");
  if (!violations || !first_bad) return fail("dqnhip_nstep_validate: null result pointer");
  HIPCHK(hipSetDevice(h->cfg.device));
  RingUse ring_use(h);
  RC(refresh_ring(h));
  const long long size = RO(h)->h_size;
  if (first < 0 || first > size || n < -1 || (n >= 0 && (long long)first + n > size))
    return fail("dqnhip_nstep_validate: the window [%d,%lld) lies outside the memory [0,%lld)", first, n < 0 ? size : (long long)first + n, size);
  if (n < 0) n = (int32_t)(size - first);
  *violations = 0; *first_bad = -1;
  if (n == 0) return 0;
  // (the scratch: the n-step learner's, or the staging buffer of a learner that only validates)
  unsigned long long* res = h->nstep ? h->nstep->viol : nullptr;
  HIPCHK(hipStreamSynchronize(h->stream));       // the staging buffer may still be in flight
  if (!res) { RC(ensure_stage(h, 2 * sizeof(unsigned long long))); res = (unsigned long long*)h->stage_dev; }
  const unsigned long long init[2] = {0ull, 0x7FFFFFFFull};
  HIPCHK(hipMemcpyAsync(res, init, sizeof init, hipMemcpyHostToDevice, h->stream));
  const H* o = RO(h);
  NstepValidateArgs a{o->ring, (const DevState*)o->st, first, n, res, (int*)(res + 1)};
  const int blocks = (int)std::max(1LL, std::min(4096LL, ((long long)n + 3) / 4));
  HIPCHK(launch(h->stream, k_nstep_validate, dim3(blocks), dim3(256), 0, a));
  unsigned long long out[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(out, res, sizeof out, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  *violations = (int64_t)out[0];
  if (out[0]) { int fb; memcpy(&fb, &out[1], sizeof fb); *first_bad = fb; }
  return 0;
}

// ---- parameters ----------------------------------------------------------------------

static float* arena_ptr(H* h, int net, int kind) {
  if (kind == DQNHIP_KIND_W) return (net >= 0 && net < 4) ? h->w[net] : nullptr;
  if (net != DQNHIP_ACTOR && net != DQNHIP_CRITIC) return nullptr;
  return kind == DQNHIP_KIND_M ? h->m[net] : kind == DQNHIP_KIND_V ? h->v[net] : kind == DQNHIP_KIND_G ? h->g[net] : nullptr;
}

int dqnhip_param_count(dqnhip_handle h, int32_t net, size_t* count) {
  if (!h || !count) return fail("null argument");
  if (net < 0 || net > 3) return fail("bad net %d", net);
  *count = layout_of(h, net).dense;
  return 0;
}

int dqnhip_get_params(dqnhip_handle h, int32_t net, int32_t kind, float* host, size_t count) {
  if (!h || !host) return fail("null argument");
  float* p = arena_ptr(h, net, kind);
  if (!p) return fail("bad (net,kind) = (%d,%d)", net, kind);
  const NetLayout& l = layout_of(h, net);
  if (count != l.dense) return fail("count %zu != parameter count %zu", count, l.dense);
  // sharded optimiser: this rank holds the Adam history of its own slice only until the group has gathered it — handing out
  // (or snapshotting: snapshot.cpp reads m, v through here) the stale rest would poison a later resume silently
  if (h->dp_shard && h->shard_stale && (kind == DQNHIP_KIND_M || kind == DQNHIP_KIND_V))
    return fail("dqnhip_get_params: the optimiser is sharded and updates ran since the last dqnhip_dp_gather_state — this rank holds the Adam "
                "history of its own slice only; call dqnhip_dp_gather_state on every rank first");
  HIPCHK(hipSetDevice(h->cfg.device));
  std::vector<float> arena(l.arena);
  const size_t sh = kind == DQNHIP_KIND_W ? h->shared_fl[net & 1] : 0;   // shared first layers: the owner's storage
  if (sh) HIPCHK(hipMemcpyAsync(arena.data(), h->w_owner->w[net], sh * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  if (sh < l.arena) HIPCHK(hipMemcpyAsync(arena.data() + sh, p + sh, (l.arena - sh) * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  arena_to_dense(l, arena, host);
  return 0;
}

int dqnhip_set_params(dqnhip_handle h, int32_t net, int32_t kind, const float* host, size_t count) {
  if (!h || !host) return fail("null argument");
  h->epoch += 1;
  float* p = arena_ptr(h, net, kind);
  if (!p) return fail("bad (net,kind) = (%d,%d)", net, kind);
  const NetLayout& l = layout_of(h, net);
  if (count != l.dense) return fail("count %zu != parameter count %zu", count, l.dense);
  HIPCHK(hipSetDevice(h->cfg.device));
  std::vector<float> arena;
  dense_to_arena(l, host, arena);
  const size_t sh = kind == DQNHIP_KIND_W ? h->shared_fl[net & 1] : 0;
  if (sh) HIPCHK(hipMemcpyAsync(h->w_owner->w[net], arena.data(), sh * sizeof(float), hipMemcpyHostToDevice, h->stream));
  if (sh < l.arena) HIPCHK(hipMemcpyAsync(p + sh, arena.data() + sh, (l.arena - sh) * sizeof(float), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (kind == DQNHIP_KIND_W) h->w16_dirty[net] = true;
  return 0;
}

int dqnhip_clone_to_target(dqnhip_handle h, int32_t net) {
  if (!h) return fail("null handle");
  h->epoch += 1;
  if (net != DQNHIP_ACTOR && net != DQNHIP_CRITIC) return fail("net must be ACTOR or CRITIC");
  HIPCHK(hipSetDevice(h->cfg.device));
  const size_t sh = h->shared_fl[net], n = layout_of(h, net).arena;
  if (sh) HIPCHK(hipMemcpyAsync(h->w_owner->w[net + 2], h->w_owner->w[net], sh * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
  if (sh < n) HIPCHK(hipMemcpyAsync(h->w[net + 2] + sh, h->w[net] + sh, (n - sh) * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
  h->w16_dirty[net + 2] = true;
  return 0;
}

// ---- multi-agent sharing (src/dqn.cpp:1036-1083, src/dqn_main.cpp:305-323) ------------------

}  // extern "C"
namespace dqnhip_host {
int pack_rows16_launch(hipStream_t st, const float* src, int n, int S, int ld_src, h16* dst, int rows, int k16) {
  HIPCHK(launch(st, k_pack_rows16, dim3(pack_blocks16(rows, k16)), dim3(256), 0, Pack16Args{src, nullptr, n, S, ld_src, dst, rows, k16}));
  return 0;
}
bool same_nets(const H* a, const H* b) {
  if (a->S != b->S || a->L != b->L) return false;
  for (int i = 0; i < a->L; ++i) if (a->cfg.hidden[i] != b->cfg.hidden[i]) return false;
  return true;
}
}  // namespace dqnhip_host
extern "C" {

// floats of the arena covered by the first `n` layers-with-blobs of a net (Caffe layer order:
// ip1..ipL, then action_layer, actionpara_layer / q_values_layer)
static int shared_prefix(const NetLayout& l, int n, size_t* fl) {
  const int heads = l.NH == kNO ? 2 : 1;
  if (n < 0 || n > l.L + heads) return fail("cannot share %d layers of a net with %d", n, l.L + heads);   // CHECK_LT, src/dqn.cpp:1060
  if (n < l.L) *fl = l.w_off[n];
  else if (n == l.L) *fl = l.hw_off;
  else if (n == l.L + heads) *fl = l.arena;
  else return fail("sharing action_layer without actionpara_layer is not supported (the two heads are one [10][H] matrix here)");
  return 0;
}

int dqnhip_share_parameters(dqnhip_handle owner, dqnhip_handle other, int32_t num_actor_layers, int32_t num_critic_layers) {
  if (!owner || !other || owner == other) return fail("ShareParameters needs two distinct learners");
  RC(smooth_refuse(owner, "dqnhip_share_parameters (owner)")); RC(smooth_refuse(other, "dqnhip_share_parameters (other)"));
  owner->epoch += 1; other->epoch += 1;
  if (owner->cfg.device != other->cfg.device) return fail("ShareParameters: both learners must live on the same device");
  if (!same_nets(owner, other)) return fail("ShareParameters: net shapes differ");
  if (owner->fp16 || other->fp16) return fail("ShareParameters is not supported in fp16 mode (each learner keeps private fp16 weight copies)");
  if (owner->w_owner) return fail("ShareParameters: the owner itself shares another learner's layers; share from the root");
  if (other->w_owner && other->w_owner != owner) return fail("ShareParameters: already sharing with a different owner");
  size_t fa = 0, fc = 0;
  RC(shared_prefix(owner->la, num_actor_layers, &fa));
  RC(shared_prefix(owner->lc, num_critic_layers, &fc));
  HIPCHK(hipSetDevice(owner->cfg.device));
  HIPCHK(hipStreamSynchronize(owner->stream));
  HIPCHK(hipStreamSynchronize(other->stream));
  if (!other->w_owner && (fa || fc)) owner->sharers += 1;
  if (other->w_owner && !(fa || fc)) owner->sharers -= 1;
  other->w_owner = (fa || fc) ? owner : nullptr;
  other->shared_fl[0] = fa; other->shared_fl[1] = fc;
  drop_graphs(other);                      // captured launches hold the old weight pointers
  return 0;
}

int dqnhip_share_replay_memory(dqnhip_handle owner, dqnhip_handle other) {
  if (!owner || !other || owner == other) return fail("ShareReplayMemory needs two distinct learners");
  RC(per_refuse(owner, "dqnhip_share_replay_memory (owner)")); RC(per_refuse(RO(owner), "dqnhip_share_replay_memory (owner)"));
  RC(per_refuse(other, "dqnhip_share_replay_memory (other)"));
  RC(smooth_refuse(owner, "dqnhip_share_replay_memory (owner)")); RC(smooth_refuse(other, "dqnhip_share_replay_memory (other)"));
  owner->epoch += 1; other->epoch += 1; RO(owner)->epoch += 1;
  if (owner->cfg.device != other->cfg.device) return fail("ShareReplayMemory: both learners must live on the same device");
  if (owner->S != other->S) return fail("ShareReplayMemory: state sizes differ");
  H* root = RO(owner);
  if (RO(other) == root) return 0;
  if (other->sharers && other->ring_shared) return fail("ShareReplayMemory: other learners already use this learner's memory");
  HIPCHK(hipSetDevice(owner->cfg.device));
  HIPCHK(hipStreamSynchronize(owner->stream));
  HIPCHK(hipStreamSynchronize(other->stream));
  if (other->ring_owner) other->ring_owner->sharers -= 1;
  if (!root->ring_ev) HIPCHK(hipEventCreateWithFlags(&root->ring_ev, hipEventDisableTiming));
  root->ring_shared = true;
  root->sharers += 1;
  other->ring_owner = root;                // other's deque is dropped: shared_ptr assignment, src/dqn.cpp:1081
  drop_graphs(other);
  return 0;
}

int dqnhip_get_iters(dqnhip_handle h, int32_t* actor_iter, int32_t* critic_iter) {
  if (!h) return fail("null handle");
  if (actor_iter) *actor_iter = h->h_actor_iter;
  if (critic_iter) *critic_iter = h->h_critic_iter;
  return 0;
}

int dqnhip_set_iters(dqnhip_handle h, int32_t actor_iter, int32_t critic_iter) {
  if (!h) return fail("null handle");
  h->epoch += 1;
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipStreamSynchronize(h->stream));
  int v[2] = {actor_iter, critic_iter};
  HIPCHK(hipMemcpy(&h->st->actor_iter, v, sizeof v, hipMemcpyHostToDevice));
  h->h_actor_iter = actor_iter; h->h_critic_iter = critic_iter;
  return 0;
}

// the rate net's next step will apply: lr_rate (lr_schedule.hip.h), host build, at the net's current iteration
int dqnhip_get_learning_rate(dqnhip_handle h, int32_t net, float* out) {
  if (!h || !out) return fail("null argument");
  if (net != DQNHIP_ACTOR && net != DQNHIP_CRITIC) return fail("net must be ACTOR or CRITIC");
  int32_t it[2] = {0, 0};
  RC(dqnhip_get_iters(h, &it[0], &it[1]));
  *out = lr_rate(schedule_of(h->cfg), net, it[net]);
  return 0;
}

// ---- introspection ----------------------------------------------------------------------

int dqnhip_debug_read(dqnhip_handle h, const char* name, float* host, size_t count) {
  if (!h || !name || !host) return fail("null argument");
  HIPCHK(hipSetDevice(h->cfg.device));
  const size_t B = h->B;
  const float* src = nullptr; size_t n = B; bool pad16 = false; bool is_int = false;
  if (!strcmp(name, "optimiser_launches")) {      // [k_adam_soft*, k_solver_soft<>, k_solver_soft_gather<>] enqueued or captured so far
    if (count < 3) return fail("buffer too small for '%s'", name);
    for (int k = 0; k < 3; ++k) host[k] = (float)h->opt_launches[k];
    return 0;
  }
  if (!strcmp(name, "sched_launches")) {          // [k_sched_soft<>, k_sched_soft_gather<>] enqueued or captured so far (a name of its own: "optimiser_launches" keeps its three words)
    if (count < 2) return fail("buffer too small for '%s'", name);
    for (int k = 0; k < 2; ++k) host[k] = (float)h->sched_launches[k];
    return 0;
  }
  if (!strcmp(name, "indexed_graph_launches")) {
    if (count < 1) return fail("buffer too small for '%s'", name);
    for (size_t k = 0; k < std::min(count, (size_t)kIxSizes); ++k) host[k] = (float)h->ix_nodes[k];      // [16, 8, 4, 2, 1 updates]
    return 0;
  }
  if (!strcmp(name, "q_target")) src = h->q_t;
  else if (!strcmp(name, "y")) src = h->y;
  else if (!strcmp(name, "q_train")) src = h->q1;
  else if (!strcmp(name, "q_policy")) src = h->q2;
  else if (!strcmp(name, "terminal")) src = h->mb_term;
  else if (!strcmp(name, "actor_out")) { src = h->aout16; pad16 = true; n = B * kNO; }
  else if (!strcmp(name, "dq_da")) { src = h->dA16; pad16 = true; n = B * kNO; }
  else if (!strcmp(name, "idx")) { src = (const float*)h->mb_idx; is_int = true; }
  else if (!strncmp(name, "act", 3) && name[3] >= '0' && name[3] <= '4' && name[4] == '_') {
    // "act<p>_<i>": the stored (post-ReLU, in place: src/dqn.cpp:409-410) tower activations of the last update's pass p
    // (0 actor_target(s'), 1 actor(s), 2 critic_target, 3 critic(s, a), 4 critic(s, mu(s))), layer i = 1 .. L, dense
    // [B][width].  Parity tests compare their SIGNS with the oracle's: an fp32 evaluation may put a pre-activation that
    // is within round-off of zero on the other side, which switches that unit's ReLU' between 1 and 0.01 for that row.
    const int p = name[3] - '0', i = atoi(name + 5);
    const NetLayout& l = layout_of(h, p >= 2);
    if (i < 1 || i > h->L) return fail("debug buffer '%s': layer out of range", name);
    const size_t W = l.dims[i];
    if (count < B * W) return fail("buffer too small for '%s': %zu < %zu", name, count, B * W);
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->fp16) {
      std::vector<h16> t16(B * W);
      HIPCHK(hipMemcpy(t16.data(), h->act16[p][i], t16.size() * sizeof(h16), hipMemcpyDeviceToHost));
      for (size_t e = 0; e < t16.size(); ++e) host[e] = (float)t16[e];
    } else HIPCHK(hipMemcpy(host, h->act[p][i], B * W * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
  }
  else if (!strncmp(name, "w16_", 4) && name[4] >= '0' && name[4] <= '3' && name[5] == 0) {
    // "w16_<net>": the fp16 mirror of a net's weight arena (the copy the fp16 GEMMs read; the optimiser pass writes it beside the fp32
    // master, host-side weight changes reach it with the next launch sequence: sync_dirty16), as stored, widened to float, in
    // dqnhip_get_params' dense Caffe order
    if (!h->fp16) return fail("debug buffer '%s': an fp32 learner keeps no fp16 weight mirror", name);
    const int net = name[4] - '0';
    const NetLayout& l = layout_of(h, net);
    if (count < l.dense) return fail("buffer too small for '%s': %zu < %zu", name, count, l.dense);
    HIPCHK(hipStreamSynchronize(h->stream));
    std::vector<h16> t16(l.arena);
    HIPCHK(hipMemcpy(t16.data(), h->w16a[net], t16.size() * sizeof(h16), hipMemcpyDeviceToHost));
    std::vector<float> arena(l.arena);
    for (size_t e = 0; e < t16.size(); ++e) arena[e] = (float)t16[e];
    arena_to_dense(l, arena, host);
    return 0;
  }
  else if (!strcmp(name, "dq")) src = h->dq;
  else if (!strcmp(name, "actor_target_out")) { src = h->aout_t16; pad16 = true; n = B * kNO; }
  else if (!strcmp(name, "actor_target_smoothed") || !strcmp(name, "target_noise_z") || !strcmp(name, "target_noise_counter")) {
    if (!h->tnoise) return fail("debug buffer '%s': target smoothing is not enabled on this learner (dqnhip_target_noise_enable)", name);
    if (!strcmp(name, "target_noise_counter")) {
      // the 64-bit counter through a float interface, exactly: [c mod 2^24, c / 2^24] (a counter below 2^48)
      if (count < 2) return fail("buffer too small for '%s'", name);
      unsigned long long c = 0;
      HIPCHK(hipStreamSynchronize(h->stream));
      HIPCHK(hipMemcpy(&c, h->tnoise->counter, sizeof c, hipMemcpyDeviceToHost));
      host[0] = (float)(c & 0xFFFFFFull); host[1] = (float)(c >> 24);
      return 0;
    }
    src = !strcmp(name, "target_noise_z") ? h->tnoise->z16 : h->tnoise->smoothed16; pad16 = true; n = B * kNO;
  }
  else if (!strcmp(name, "dz_c") || !strcmp(name, "dz_a")) {
    // the tower-top gradient the head-backward forms leave for the tower, dense [B][H] (the pitch the head kernels write with);
    // fp16 learner: the scaled fp16 panel, widened as stored
    const int kind = name[3] == 'c';
    const NetLayout& l = layout_of(h, kind);
    const size_t W = l.dims[h->L];
    if (count < B * W) return fail("buffer too small for '%s': %zu < %zu", name, count, B * W);
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->fp16) {
      std::vector<h16> t16(B * W);
      HIPCHK(hipMemcpy(t16.data(), h->dZ16[kind][h->L], t16.size() * sizeof(h16), hipMemcpyDeviceToHost));
      for (size_t e = 0; e < t16.size(); ++e) host[e] = (float)t16[e];
    } else HIPCHK(hipMemcpy(host, kind ? h->dZc[h->L] : h->dZa[h->L], B * W * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
  }
  else if (!strcmp(name, "dxc")) {
    if (plan_of(h).fuse_head) return fail("debug buffer 'dxc': this learner's plan fuses dQ/da into the actor heads' backward (k_dqda_head_bwd) and never writes it; create the learner with DQNHIP_TUNE_SEPARATE_ACTOR_HEAD_BWD");
    const size_t ld = h->lc.kp[0];
    if (count < B * kNO) return fail("buffer too small for '%s': %zu < %zu", name, count, B * (size_t)kNO);
    std::vector<float> t(B * ld);
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(t.data(), h->dZc[0], t.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t r = 0; r < B; ++r) for (int c = 0; c < kNO; ++c) host[r * kNO + c] = t[r * ld + h->S + c];
    return 0;
  }
  else return fail("unknown debug buffer '%s'", name);
  if (count < n) return fail("buffer too small for '%s': %zu < %zu", name, count, n);
  std::vector<float> tmp(pad16 ? B * kAP : B);
  HIPCHK(hipMemcpyAsync(tmp.data(), src, tmp.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (pad16) { for (size_t r = 0; r < B; ++r) for (int c = 0; c < kNO; ++c) host[r * kNO + c] = tmp[r * kAP + c]; }
  else if (is_int) { for (size_t r = 0; r < B; ++r) host[r] = (float)reinterpret_cast<const int*>(tmp.data())[r]; }
  else memcpy(host, tmp.data(), B * sizeof(float));
  return 0;
}

// ---- update diagnostics (include/dqnhip.h has the definitions; the kernels and the order of every sum: diag_kernels.hip.h) ---------

}  // extern "C"
namespace dqnhip_host {

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
  RC(sched_refuse(h, "dqnhip_diag_collect"));      // (k_diag_prep prices the step as lr x adam_correction)
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

// ---- replay sweep (include/dqnhip.h has the definitions; the row kernel, the finaliser and the order of every sum: sweep_kernels.hip.h;
// the forward launches of a chunk: sweep_forward, learner.hip) ------------------------------------------------------------------------

}  // extern "C"
namespace dqnhip_host {

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
  RC(nstep_refuse(h, what));
  if (h->next_phase != 0) return fail("%s: the replay sweep overwrites the update's panels, and a phased update is in progress (next phase %d)", what, h->next_phase);
  if (h->cfg.dp_world > 1 || h->comm || h->dp_half || h->dp_shard)
    return fail("%s: the replay sweep is not available on a data-parallel learner (dp_world > 1, dqnhip_dp_init) in this version", what);
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

int dqnhip_evaluate_memory(dqnhip_handle h, int32_t first, int32_t n, dqnhip_sweep_report* out, const dqnhip_sweep_rows* rows) {
  if (!h) return fail("dqnhip_evaluate_memory: null handle");
  if (!out) return fail("dqnhip_evaluate_memory: null report");
  return sweep_run(h, "dqnhip_evaluate_memory", false, first, n, out, rows);
}

int dqnhip_per_refresh(dqnhip_handle h, int32_t first, int32_t n, dqnhip_sweep_report* out) {
  if (!h) return fail("dqnhip_per_refresh: null handle");
  return sweep_run(h, "dqnhip_per_refresh", true, first, n, out, nullptr);
}

int dqnhip_get_stream(dqnhip_handle h, void** stream) {
  if (!h || !stream) return fail("null argument");
  *stream = (void*)h->stream;
  return 0;
}

int dqnhip_set_kernel_timing(dqnhip_handle h, int32_t enable) {
  if (!h) return fail("null handle");
  h->timing = enable != 0;
  return 0;
}

int dqnhip_get_kernel_timing(dqnhip_handle h, const char* family, float* avg_ms, int64_t* launches, int32_t reset) {
  if (!h || !family) return fail("null argument");
  HIPCHK(hipSetDevice(h->cfg.device));
  int fam = -1;
  std::string names;
  for (int i = 0; i < kNumFamily; ++i) { if (!strcmp(family, kFamily[i])) fam = i; names += (i ? "|" : ""); names += kFamily[i]; }
  if (fam < 0) return fail("unknown kernel family '%s' (%s)", family, names.c_str());
  HIPCHK(hipStreamSynchronize(h->stream));
  double total = 0; int64_t cnt = 0;
  for (auto& r : h->recs) {
    if (r.family != fam) continue;
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, r.a, r.b));
    total += ms; cnt += 1;
  }
  if (avg_ms) *avg_ms = cnt ? (float)(total / cnt) : 0.0f;
  if (launches) *launches = cnt;
  if (reset) {
    for (auto& r : h->recs) { hipEventDestroy(r.a); hipEventDestroy(r.b); }
    h->recs.clear();
  }
  return 0;
}

}  // extern "C"

// ---- asynchronous learner-state save: the launchers of state_kernels.hip.h (the host side: learner_save_async.hip) ----
namespace dqnhip_host {

int state_pack_params_launch(H* h, const dqnhip_state::PackSeg* segs_dev, int n_seg, dqnhip_state::StateRec* rec_dev) {
  const float* p_max = h->per ? &((const PerDev*)h->per->dev)->p_max : nullptr;
  HIPCHK(launch(h->stream, k_state_pack_params, dim3(64, n_seg + 1), dim3(256), 0, segs_dev, n_seg, (const DevState*)h->st, p_max, rec_dev));
  return 0;
}
int state_pack_ring_launch(H* h, const dqnhip_state::RingPackArgs& a) {
  if (a.cap < 1 || a.n_arr < 1 || a.n_arr > dqnhip_state::kRingArrays) return fail("state_pack_ring_launch: bad arguments");
  HIPCHK(launch(h->stream, k_state_pack_ring, dim3((a.cap + dqnhip_state::kPackRows - 1) / dqnhip_state::kPackRows, a.n_arr), dim3(256), 0, a));
  return 0;
}
int state_crc_launch(H* h, const dqnhip_state::CrcArgs& a) {
  if (a.n < 1 || a.n > dqnhip_state::kMaxCrcSections) return fail("state_crc_launch: bad arguments");
  if (a.total_chunks == 0) return 0;
  HIPCHK(launch(h->stream, k_state_crc, dim3((a.total_chunks + 255) / 256), dim3(256), 0, a));
  return 0;
}
// asynchronous Caffe snapshot (snapshot_kernels.hip.h): the ring's window as the `.replaymemory` stream at `stream_dev`, which has
// room for the stream of a full ring and, behind that (rounded up to a dword), the guard band this call fills and nothing else writes.
// The stream's first record (stream_dev + 4) lies on a 16-byte boundary.  64 records per workgroup measured fastest
// (profiles/snapshot_async_ab.md); fewer where the state is so long that 64 rows do not fit the LDS a launch gets without asking
int snap_pack_replay_launch(H* h, uint8_t* stream_dev) {
  const uint64_t max_dwords = dqnhip_snap::stream_dwords(h->S, (uint64_t)h->ring.cap);
  const size_t row_bytes = (size_t)dqnhip_snap::snap_lds_row_words(h->S) * sizeof(uint32_t);
  int K = 64;
  while (K > 16 && K * row_bytes > 48 * 1024) K /= 2;
  if (K * row_bytes > 48 * 1024) return fail("the asynchronous snapshot's pack kernel stages 16 records of %zu bytes in LDS: too long a state (S = %d)", row_bytes, h->S);
  if ((uintptr_t)(stream_dev + 4) % 16 != 0 || h->ring.cap < 1) return fail("snap_pack_replay_launch: bad arguments");
  HIPCHK(hipMemsetD32Async((hipDeviceptr_t)(stream_dev + 4 * max_dwords), (int)dqnhip_snap::kGuardWord, dqnhip_snap::kGuardWords, h->stream));
  HIPCHK(launch(h->stream, k_snap_pack_replay, dim3((unsigned)((h->ring.cap + K - 1) / K)), dim3(256), K * row_bytes, h->ring, (const DevState*)h->st,
                (uint32_t*)stream_dev, max_dwords, K));
  return 0;
}

}  // namespace dqnhip_host

extern "C" int dqnhip_state_crc32_device(dqnhip_handle h, const void* host_bytes, size_t bytes, int32_t misalign, uint32_t* crc) {
  using namespace dqnhip_state;
  if (!h || !crc || (!host_bytes && bytes)) return fail("dqnhip_state_crc32_device: null argument");
  if (misalign < 0 || misalign > 15) return fail("dqnhip_state_crc32_device: misalign %d is outside 0 ... 15", misalign);
  if (bytes > ((size_t)1 << 31)) return fail("dqnhip_state_crc32_device: %zu bytes are more than this door takes (2^31)", bytes);
  HIPCHK(hipSetDevice(h->cfg.device));
  const size_t chunks = (bytes + kCrcChunk - 1) / kCrcChunk, out_off = round_up_z((size_t)misalign + bytes, 16);
  RC(ensure_stage(h, out_off + chunks * sizeof(uint32_t) + 16));
  uint8_t* base = (uint8_t*)h->stage_dev;
  if (bytes) HIPCHK(hipMemcpyAsync(base + misalign, host_bytes, bytes, hipMemcpyHostToDevice, h->stream));
  CrcArgs a{};
  a.base = base; a.rec = nullptr; a.out = (uint32_t*)(base + out_off); a.n = 1; a.max_rows = 0; a.total_chunks = (uint32_t)chunks;
  a.sec[0] = CrcSection{(uint64_t)misalign, (uint64_t)bytes, 0u, 0u};
  RC(state_crc_launch(h, a));
  std::vector<uint32_t> raws(chunks);
  if (chunks) HIPCHK(hipMemcpyAsync(raws.data(), a.out, chunks * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  uint32_t op[32];
  std::vector<uint32_t> tab(kCrcTableWords);
  crc_zeros_op(op, kCrcChunk);
  crc_op_table(tab.data(), op);
  *crc = crc_fold_chunks(raws.data(), bytes, tab.data());
  return 0;
}
