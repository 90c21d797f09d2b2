// learner_state.hip — dqnhip_save_state / dqnhip_load_state: the native learner-state file (include/dqnhip.h; DESIGN.md 9 has the
// byte layout, state_codec.cpp the container).  Host only: copies between the learner's device state and the file's sections, no
// kernel of its own — the one launch a load may need, the priority tree's set pass, goes through per_restore (learner_io.hip).
#include "learner_internal.hip.h"
#include "state_codec.h"

using namespace dqnhip_state;

namespace {

// v1's limits, the same for save and load
int state_refuse(const H* h, const char* what) {
  if (h->ring_owner || h->ring_shared) return fail("%s: a learner that shares a replay memory (dqnhip_share_replay_memory) is not supported in this version", what);
  if (h->w_owner || h->sharers) return fail("%s: a learner that shares parameters or is shared from (dqnhip_share_parameters) is not supported in this version", what);
  if (h->cfg.dp_world > 1 || h->comm || h->dp_half || h->dp_shard) return fail("%s: a data-parallel learner (dp_world > 1, dqnhip_dp_init) is not supported in this version", what);
  if (h->next_phase != 0) return fail("%s: a phased update is in progress (next phase %d)", what, h->next_phase);
  if (h->timing) return fail("%s: kernel timing is on (dqnhip_set_kernel_timing)", what);
  return 0;
}

// the window [head, head + size) of a ring array with rows of `width` bytes at a pitch of `pitch` bytes <-> dense host rows, logical order
int window_copy(const H* h, void* dev, size_t pitch, void* host, size_t width, int head, int size, bool to_host) {
  const int cap = h->ring.cap;
  const int n0 = std::min(size, cap - head);
  for (int piece = 0; piece < 2; ++piece) {
    const int first = piece ? 0 : head, rows = piece ? size - n0 : n0, done = piece ? n0 : 0;
    if (rows <= 0) continue;
    char* d = (char*)dev + (size_t)first * pitch; char* s = (char*)host + (size_t)done * width;
    if (pitch == width) {                          // dense on both sides: one linear copy
      if (to_host) HIPCHK(hipMemcpy(s, d, (size_t)rows * width, hipMemcpyDeviceToHost));
      else HIPCHK(hipMemcpy(d, s, (size_t)rows * width, hipMemcpyHostToDevice));
    }
    else if (to_host) HIPCHK(hipMemcpy2D(s, width, d, pitch, width, (size_t)rows, hipMemcpyDeviceToHost));
    else HIPCHK(hipMemcpy2D(d, pitch, s, width, width, (size_t)rows, hipMemcpyHostToDevice));
  }
  return 0;
}

}  // namespace

extern "C" {

int dqnhip_save_state(dqnhip_handle h, const char* filename, int32_t flags, const void* user, size_t user_bytes) {
  if (!h || !filename) return fail("dqnhip_save_state: null argument");
  if (flags & ~DQNHIP_STATE_NO_MEMORY) return fail("dqnhip_save_state: unknown flags %d", flags);
  if (!user && user_bytes) return fail("dqnhip_save_state: user is null but user_bytes is %zu", user_bytes);
  RC(state_refuse(h, "dqnhip_save_state"));
  const bool with_mem = !(flags & DQNHIP_STATE_NO_MEMORY);
  HIPCHK(hipSetDevice(h->cfg.device));
  RC(per_sync_if_needed(h));
  HIPCHK(hipStreamSynchronize(h->stream));
  RC(ix_harvest_all(h));                           // (indexed updates: their scalars stay collectable, they are not part of the file)
  DevState st{};
  HIPCHK(hipMemcpy(&st, h->st, sizeof st, hipMemcpyDeviceToHost));
  h->h_head = st.ring_head; h->h_size = st.ring_size; h->ring_stale = false;     // (refresh_ring, from the copy at hand)

  std::vector<float> par[8];
  std::vector<Section> sec;
  for (int net = 0; net < 4; ++net) {
    par[net].resize(layout_of(h, net).dense);
    RC(dqnhip_get_params(h, net, DQNHIP_KIND_W, par[net].data(), par[net].size()));
    sec.push_back({kTagW[net], par[net].data(), par[net].size() * sizeof(float)});
  }
  for (int net = 0; net < 2; ++net) {
    std::vector<float>&m = par[4 + net], &v = par[6 + net];
    m.resize(layout_of(h, net).dense); v.resize(m.size());
    RC(dqnhip_get_params(h, net, DQNHIP_KIND_M, m.data(), m.size()));
    RC(dqnhip_get_params(h, net, DQNHIP_KIND_V, v.data(), v.size()));
    sec.push_back({kTagM[net], m.data(), m.size() * sizeof(float)});
    sec.push_back({kTagV[net], v.data(), v.size() * sizeof(float)});
  }
  const DevSection dev{st.actor_iter, st.critic_iter, st.update_counter, st.critic_loss, st.avg_q, st.flags, st.skipped_steps};
  sec.push_back({kTagDev, &dev, sizeof dev});
  const LossScaleSection ls{{st.ls_mult[0][0], st.ls_mult[1][0]}, {st.ls_good[0], st.ls_good[1]}, {st.ls_backoffs[0], st.ls_backoffs[1]},
                            {st.ls_growths[0], st.ls_growths[1]}};
  if (h->ls_dynamic) sec.push_back({kTagLossScale, &ls, sizeof ls});
  const HostSection host{h->sample_states_calls, h->cfg.seed};
  sec.push_back({kTagHost, &host, sizeof host});

  const int head = st.ring_head, size = st.ring_size, S = h->S;
  const RingSection ring{head, size};
  std::vector<float> s, nx, a, r, mc, leaves;
  std::vector<uint8_t> term;
  PerSection per{};
  if (with_mem) {
    if (head < 0 || head >= h->ring.cap || size < 0 || size > h->ring.cap) return fail("dqnhip_save_state: the ring's (head, size) = (%d, %d) is outside its capacity %d", head, size, h->ring.cap);
    s.resize((size_t)size * S); nx.resize((size_t)size * S); a.resize((size_t)size * kNO); r.resize(size); mc.resize(size); term.resize(size);
    const Ring& g = h->ring;
    RC(window_copy(h, g.state, (size_t)g.SP * 4, s.data(), (size_t)S * 4, head, size, true));
    RC(window_copy(h, g.next, (size_t)g.SP * 4, nx.data(), (size_t)S * 4, head, size, true));
    RC(window_copy(h, g.act, (size_t)kAP * 4, a.data(), (size_t)kNO * 4, head, size, true));
    RC(window_copy(h, g.reward, 4, r.data(), 4, head, size, true));
    RC(window_copy(h, g.mc, 4, mc.data(), 4, head, size, true));
    RC(window_copy(h, g.term, 1, term.data(), 1, head, size, true));
    sec.push_back({kTagRing, &ring, sizeof ring});
    sec.push_back({kTagStates, s.data(), s.size() * 4}); sec.push_back({kTagNext, nx.data(), nx.size() * 4});
    sec.push_back({kTagAct, a.data(), a.size() * 4}); sec.push_back({kTagReward, r.data(), r.size() * 4});
    sec.push_back({kTagMc, mc.data(), mc.size() * 4}); sec.push_back({kTagTerm, term.data(), term.size()});
    if (h->per) {
      const dqnhip_per_config& c = h->per->cfg;
      float p_max = 0.0f;
      RC(per_read_p_max(h, &p_max));
      per = PerSection{c.alpha, c.beta0, c.beta_anneal_iters, c.eps, c.seed, p_max, 0, (int64_t)h->per->syncs};
      leaves.resize(size);
      RC(window_copy(h, h->per->tree.lvl[0], 4, leaves.data(), 4, head, size, true));
      sec.push_back({kTagPerCfg, &per, sizeof per});
      sec.push_back({kTagPerLeaves, leaves.data(), leaves.size() * 4});
    }
  }
  if (user_bytes) sec.push_back({kTagUser, user, user_bytes});

  dqnhip_state_info_t info{};
  info.struct_size = (int32_t)sizeof info; info.version = (int32_t)kVersion; info.flags = flags;
  info.precision = h->cfg.precision; info.minibatch = h->cfg.minibatch; info.state_size = h->cfg.state_size; info.num_hidden = h->cfg.num_hidden;
  for (int i = 0; i < h->cfg.num_hidden; ++i) info.hidden[i] = h->cfg.hidden[i];
  info.replay_capacity = h->cfg.replay_capacity; info.memory_size = with_mem ? size : 0;
  info.actor_iter = st.actor_iter; info.critic_iter = st.critic_iter;
  info.has_memory = with_mem; info.has_per = with_mem && h->per; info.has_loss_scale = h->ls_dynamic;
  info.seed = h->cfg.seed; info.update_counter = st.update_counter;
  std::string err;
  if (write_file(filename, info, sec, &err)) return fail("dqnhip_save_state: %s", err.c_str());
  return 0;
}

int dqnhip_load_state(dqnhip_handle h, const char* filename) {
  if (!h || !filename) return fail("dqnhip_load_state: null argument");
  RC(state_refuse(h, (std::string("dqnhip_load_state: ") + filename).c_str()));
  // ---- everything that can fail for the file's sake, before the learner is touched ----
  Parsed p; std::string err;
  if (read_file(filename, &p, true, &err)) return fail("dqnhip_load_state: %s", err.c_str());
  const dqnhip_state_info_t& in = p.info;
  const int S = h->S;
  bool same = in.state_size == h->cfg.state_size && in.num_hidden == h->cfg.num_hidden;
  for (int i = 0; same && i < h->cfg.num_hidden; ++i) same = in.hidden[i] == h->cfg.hidden[i];
  if (!same) {
    std::string a, b;
    for (int i = 0; i < std::min(std::max(in.num_hidden, 0), kMaxL); ++i) a += (i ? "," : "") + std::to_string(in.hidden[i]);
    for (int i = 0; i < h->cfg.num_hidden; ++i) b += (i ? "," : "") + std::to_string(h->cfg.hidden[i]);
    return fail("dqnhip_load_state: %s: the file's nets (state_size %d, hidden %s) are not this learner's (state_size %d, hidden %s)", filename,
                in.state_size, a.c_str(), h->cfg.state_size, b.c_str());
  }
  const bool with_mem = in.has_memory != 0;
  // a section of exactly `bytes` bytes
  auto need = [&](uint32_t tag, uint64_t bytes, const uint8_t** out) -> int {
    const Entry* e = p.find(tag);
    if (!e) return fail("dqnhip_load_state: %s: section %s is missing", filename, tag_name(tag).c_str());
    if (e->bytes != bytes) return fail("dqnhip_load_state: %s: section %s holds %llu bytes, expected %llu", filename, tag_name(tag).c_str(),
                                       (unsigned long long)e->bytes, (unsigned long long)bytes);
    *out = p.at(e);
    return 0;
  };
  const uint8_t *q_ring = nullptr, *q_s = nullptr, *q_nx = nullptr, *q_a = nullptr, *q_r = nullptr, *q_mc = nullptr, *q_t = nullptr, *q_pc = nullptr, *q_pl = nullptr;
  RingSection ring{}; PerSection per{};
  if (with_mem) {
    if (in.replay_capacity != h->ring.cap) return fail("dqnhip_load_state: %s: the file's replay capacity %d is not this learner's %d", filename, in.replay_capacity, h->ring.cap);
    if ((in.has_per != 0) != (h->per != nullptr))
      return fail(in.has_per ? "dqnhip_load_state: %s: the file holds priorities, this learner samples uniformly (dqnhip_per_enable first, or save with DQNHIP_STATE_NO_MEMORY)"
                             : "dqnhip_load_state: %s: the file holds no priorities, this learner has prioritized replay enabled", filename);
    if (in.has_per) {
      RC(need(kTagPerCfg, sizeof per, &q_pc));
      memcpy(&per, q_pc, sizeof per);
      if (__builtin_bit_cast(uint32_t, per.alpha) != __builtin_bit_cast(uint32_t, h->per->cfg.alpha))
        return fail("dqnhip_load_state: %s: the file's priorities were stored with alpha %g, this learner's alpha is %g", filename, (double)per.alpha, (double)h->per->cfg.alpha);
    }
    RC(need(kTagRing, sizeof ring, &q_ring));
    memcpy(&ring, q_ring, sizeof ring);
    const int cap = h->ring.cap;
    if (ring.ring_size < 0 || ring.ring_size > cap || ring.ring_head < 0 || ring.ring_head >= cap || ring.ring_size != in.memory_size)
      return fail("dqnhip_load_state: %s: (ring_head, ring_size) = (%d, %d) does not fit the capacity %d / the header's memory_size %d", filename,
                  ring.ring_head, ring.ring_size, cap, in.memory_size);
    const uint64_t n = (uint64_t)ring.ring_size;
    RC(need(kTagStates, n * S * 4, &q_s)); RC(need(kTagNext, n * S * 4, &q_nx)); RC(need(kTagAct, n * kNO * 4, &q_a));
    RC(need(kTagReward, n * 4, &q_r)); RC(need(kTagMc, n * 4, &q_mc)); RC(need(kTagTerm, n, &q_t));
    if (in.has_per) {
      RC(need(kTagPerLeaves, n * 4, &q_pl));
      if (!(per.p_max >= 0.0f) || !std::isfinite(per.p_max) || !(per.beta0 >= 0.0f && per.beta0 <= 1.0f) || per.beta_anneal_iters < 0 || !(per.eps >= 0.0f) || !std::isfinite(per.eps))
        return fail("dqnhip_load_state: %s: section PERC holds values outside their ranges", filename);
      for (uint64_t i = 0; i < n; ++i) {
        float v; memcpy(&v, q_pl + 4 * i, 4);
        if (!std::isfinite(v) || v < 0.0f) return fail("dqnhip_load_state: %s: priority %llu = %g is not finite and >= 0", filename, (unsigned long long)i, (double)v);
      }
    }
  }
  const uint8_t* q_par[8] = {nullptr};
  for (int net = 0; net < 4; ++net) RC(need(kTagW[net], (uint64_t)layout_of(h, net).dense * 4, &q_par[net]));
  for (int net = 0; net < 2; ++net) {
    RC(need(kTagM[net], (uint64_t)layout_of(h, net).dense * 4, &q_par[4 + net]));
    RC(need(kTagV[net], (uint64_t)layout_of(h, net).dense * 4, &q_par[6 + net]));
  }
  const uint8_t *q_dev = nullptr, *q_host = nullptr, *q_ls = nullptr;
  DevSection dev{}; HostSection host{}; LossScaleSection ls{};
  RC(need(kTagDev, sizeof dev, &q_dev)); memcpy(&dev, q_dev, sizeof dev);
  RC(need(kTagHost, sizeof host, &q_host)); memcpy(&host, q_host, sizeof host);
  if (dev.actor_iter != in.actor_iter || dev.critic_iter != in.critic_iter || dev.update_counter != in.update_counter || host.seed != in.seed)
    return fail("dqnhip_load_state: %s: the header and the DEVS / HOST sections disagree", filename);
  const bool apply_ls = in.has_loss_scale && h->ls_dynamic;
  if (in.has_loss_scale) { RC(need(kTagLossScale, sizeof ls, &q_ls)); memcpy(&ls, q_ls, sizeof ls); }
  if (apply_ls)
    for (int i = 0; i < 2; ++i) {
      if (!is_pow2(ls.mult[i])) return fail("dqnhip_load_state: %s: loss-scale multiplier %g is not a power of two", filename, (double)ls.mult[i]);
      if (ls.mult[i] < h->cfg.loss_scale_min_mult || ls.mult[i] > h->cfg.loss_scale_max_mult)
        return fail("dqnhip_load_state: %s: loss-scale multiplier %g is outside this learner's [loss_scale_min_mult, loss_scale_max_mult] = [%g, %g]", filename,
                    (double)ls.mult[i], (double)h->cfg.loss_scale_min_mult, (double)h->cfg.loss_scale_max_mult);
    }

  // ---- the learner ----
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipStreamSynchronize(h->stream));
  RC(ix_harvest_all(h));
  h->epoch += 1;                                   // a chain ends here
  h->chain_valid = false;
  std::vector<float> tmp;
  auto put_params = [&](int net, int kind, const uint8_t* q) -> int {
    tmp.resize(layout_of(h, net).dense);
    memcpy(tmp.data(), q, tmp.size() * 4);         // (the sections are packed back to back: not aligned)
    return dqnhip_set_params(h, net, kind, tmp.data(), tmp.size());     // W: marks the net's fp16 mirror dirty
  };
  for (int net = 0; net < 4; ++net) RC(put_params(net, DQNHIP_KIND_W, q_par[net]));
  for (int net = 0; net < 2; ++net) { RC(put_params(net, DQNHIP_KIND_M, q_par[4 + net])); RC(put_params(net, DQNHIP_KIND_V, q_par[6 + net])); }
  DevState st{};
  HIPCHK(hipMemcpy(&st, h->st, sizeof st, hipMemcpyDeviceToHost));      // (adam_corr, soft_now, gbase_*: per-update scratch, left as they are)
  st.actor_iter = dev.actor_iter; st.critic_iter = dev.critic_iter; st.update_counter = dev.update_counter;
  st.critic_loss = dev.critic_loss; st.avg_q = dev.avg_q; st.flags = dev.flags; st.skipped_steps = dev.skipped_steps;
  if (apply_ls)
    for (int i = 0; i < 2; ++i) {
      st.ls_mult[i][0] = ls.mult[i]; st.ls_mult[i][1] = 1.0f / ls.mult[i];
      st.ls_good[i] = ls.good[i]; st.ls_backoffs[i] = ls.backoffs[i]; st.ls_growths[i] = ls.growths[i];
    }
  if (with_mem) { st.ring_head = ring.ring_head; st.ring_size = ring.ring_size; }
  HIPCHK(hipMemcpy(h->st, &st, sizeof st, hipMemcpyHostToDevice));
  h->h_actor_iter = dev.actor_iter; h->h_critic_iter = dev.critic_iter;
  h->h_head = st.ring_head; h->h_size = st.ring_size; h->ring_stale = false;
  h->sample_states_calls = host.sample_states_calls;
  h->cfg.seed = host.seed;
  // what dqnhip_read_stats reads: the last update's pair and the sticky flags, as the device now holds them
  h->pinned_stats[0] = dev.critic_loss; h->pinned_stats[1] = dev.avg_q; memcpy(&h->pinned_stats[2], &dev.flags, sizeof dev.flags);
  h->ix_prev_flags = dev.flags;
  if (with_mem) {
    const int head = ring.ring_head, size = ring.ring_size;
    const Ring& g = h->ring;
    // (pad columns of the ring's rows are zero from create on and no writer touches them: only the S / 10 real columns move)
    RC(window_copy(h, g.state, (size_t)g.SP * 4, (void*)q_s, (size_t)S * 4, head, size, false));
    RC(window_copy(h, g.next, (size_t)g.SP * 4, (void*)q_nx, (size_t)S * 4, head, size, false));
    RC(window_copy(h, g.act, (size_t)kAP * 4, (void*)q_a, (size_t)kNO * 4, head, size, false));
    RC(window_copy(h, g.reward, 4, (void*)q_r, 4, head, size, false));
    RC(window_copy(h, g.mc, 4, (void*)q_mc, 4, head, size, false));
    RC(window_copy(h, g.term, 1, (void*)q_t, 1, head, size, false));
    if (h->per) {
      dqnhip_per_config& c = h->per->cfg;
      c.beta0 = per.beta0; c.beta_anneal_iters = per.beta_anneal_iters; c.eps = per.eps; c.seed = per.seed;
      tmp.resize((size_t)size);
      if (size) memcpy(tmp.data(), q_pl, (size_t)size * 4);
      RC(per_restore(h, tmp.data(), head, size, per.p_max, (long long)per.syncs));
    }
  }
  drop_graphs(h);
  return 0;
}

}  // extern "C"
