// learner_state.hip — dqnhip_save_state / dqnhip_load_state: the native learner-state file (include/dqnhip.h; DESIGN.md 9 has the
// byte layout, state_codec.cpp the container and the manifest: which sections, in which order).  Host only: copies between the
// learner's device state and the file's sections, no kernel of its own — the one launch a load may need, the priority tree's set
// pass, goes through per_restore (learner_per.hip).  The save takes its bytes through dqnhip_get_params and plain copies of the ring's
// window: it shares the manifest with dqnhip_save_state_async (learner_save_async.hip) and nothing of that one's device path, so
// either checks the other.
#include "learner_state.hip.h"

using namespace dqnhip_state;

namespace dqnhip_host {

int state_refuse(const H* h, const char* what) {
  if (shares_ring(h)) return fail("%s: a learner that shares a replay memory (dqnhip_share_replay_memory) is not supported in this version", what);
  if (shares_params(h)) return fail("%s: a learner that shares parameters or is shared from (dqnhip_share_parameters) is not supported in this version", what);
  if (dp_grouped(h)) return fail("%s: a data-parallel learner (dp_world > 1, dqnhip_dp_init) is not supported in this version", what);
  if (h->next_phase != 0) return fail("%s: a phased update is in progress (next phase %d)", what, h->next_phase);
  if (h->timing) return fail("%s: kernel timing is on (dqnhip_set_kernel_timing)", what);
  return 0;
}

StateShape state_shape_of(const H* h, bool with_mem, int ring_size, size_t user_bytes) {
  StateShape s;
  for (int net = 0; net < 4; ++net) s.dense[net] = layout_of(h, net).dense;
  s.state_size = h->S;
  s.has_solver = h->cfg.solver_type != DQNHIP_SOLVER_ADAM;
  s.has_lr = has_policy(h) || has_decay(h);
  s.has_loss_scale = h->ls_dynamic;
  s.with_memory = with_mem; s.has_per = with_mem && h->per;
  s.ring_size = with_mem ? ring_size : 0;
  s.user_bytes = user_bytes;
  return s;
}

FixedSections state_fixed_of(const H* h) {
  const dqnhip_config& c = h->cfg;
  FixedSections f;
  f.solver = SolverSection{c.solver_type, c.rms_decay, {0, 0}};
  // LRSC: the schedule's words (only the stepvalues in use: what lies behind them is not the learner's), decay, kind
  const LrSchedule s = schedule_of(c);
  LrSection& o = f.lr;
  o.policy = s.policy; o.base_lr[0] = s.base_lr[0]; o.base_lr[1] = s.base_lr[1]; o.gamma = s.gamma; o.power = s.power;
  o.stepsize = s.stepsize; o.max_iter = s.max_iter; o.n_stepvalue = s.n_stepvalue;
  for (int i = 0; i < s.n_stepvalue && i < kLrMaxStepvalues; ++i) o.stepvalue[i] = s.stepvalue[i];
  o.weight_decay = c.weight_decay; o.regularization_type = c.regularization_type;
  f.host = HostSection{h->sample_states_calls, c.seed};
  if (h->per) {
    const dqnhip_per_config& pc = h->per->cfg;
    f.per = PerSection{pc.alpha, pc.beta0, pc.beta_anneal_iters, pc.eps, pc.seed, 0.0f, 0, (int64_t)h->per->syncs};
  }
  return f;
}

int ring_arrays_of(const H* h, RingDev out[kRingArrays]) {
  const Ring& g = h->ring;
  void* const ptr[kRingArrays] = {g.state, g.next, g.act, g.reward, g.mc, g.term, h->per ? h->per->tree.lvl[0] : nullptr};
  const int pitch[kRingArrays] = {g.SP, g.SP, kAP, 1, 1, 1, 1};
  for (int i = 0; i < kRingArrays; ++i) out[i] = RingDev{ptr[i], pitch[i], (int32_t)ring_width(i, h->S), (int32_t)kRingArray[i].elem_bytes};
  return ring_arrays(h->per != nullptr);
}

}  // namespace dqnhip_host

namespace {

// the window [head, head + size) of a ring array <-> dense host rows, logical order
int window_copy(const H* h, const RingDev& g, void* host, int head, int size, bool to_host) {
  const size_t pitch = (size_t)g.pitch * g.elem, width = (size_t)g.width * g.elem;
  const int cap = h->ring.cap;
  const int n0 = std::min(size, cap - head);
  for (int piece = 0; piece < 2; ++piece) {
    const int first = piece ? 0 : head, rows = piece ? size - n0 : n0, done = piece ? n0 : 0;
    if (rows <= 0) continue;
    char* d = (char*)g.ptr + (size_t)first * pitch; char* s = (char*)host + (size_t)done * width;
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
  RC(state_async_join(h, "dqnhip_save_state"));    // (an asynchronous save in flight finishes first)
  const bool with_mem = !(flags & DQNHIP_STATE_NO_MEMORY);
  HIPCHK(hipSetDevice(h->cfg.device));
  RC(per_sync_if_needed(h));
  HIPCHK(hipStreamSynchronize(h->stream));
  RC(ix_harvest_all(h));                           // (indexed updates: their scalars stay collectable, they are not part of the file)
  DevState st{};
  HIPCHK(hipMemcpy(&st, h->st, sizeof st, hipMemcpyDeviceToHost));
  h->h_head = st.ring_head; h->h_size = st.ring_size; h->ring_stale = false;     // (refresh_ring, from the copy at hand)
  const int head = st.ring_head, size = st.ring_size;
  const std::string bad = with_mem ? ring_range_error(head, size, h->ring.cap) : "";
  if (!bad.empty()) return fail("dqnhip_save_state: %s", bad.c_str());

  const StateShape shape = state_shape_of(h, with_mem, size, user_bytes);
  FixedSections fixed = state_fixed_of(h);
  fixed.user = user;
  fixed.dev = DevSection{st.actor_iter, st.critic_iter, st.update_counter, st.critic_loss, st.avg_q, st.flags, st.skipped_steps};
  fixed.ls = LossScaleSection{{st.ls_mult[0][0], st.ls_mult[1][0]}, {st.ls_good[0], st.ls_good[1]}, {st.ls_backoffs[0], st.ls_backoffs[1]},
                              {st.ls_growths[0], st.ls_growths[1]}};
  fixed.ring = RingSection{head, size};
  // the manifest's sections; the parameters and the ring's arrays through host copies of this call's own
  RingDev ring[kRingArrays];
  ring_arrays_of(h, ring);
  const std::vector<ManifestEntry> man = manifest(shape);
  std::vector<std::vector<float>> own(man.size());
  for (size_t k = 0; k < man.size(); ++k)          // (all of the host's buffers before the first copy: the copies then follow one another)
    if (man[k].src == Src::Par || man[k].src == Src::RingArray) own[k].resize((size_t)((man[k].bytes + 3) / 4));
  std::vector<Section> sec;
  for (size_t k = 0; k < man.size(); ++k) {
    const ManifestEntry& e = man[k];
    const void* data = fixed.of(e.src);
    if (e.src == Src::PerCfg) RC(per_read_p_max(h, &fixed.per.p_max));
    if (e.src == Src::Par || e.src == Src::RingArray) {
      if (e.src == Src::Par) RC(dqnhip_get_params(h, par_net(e.index), par_kind(e.index), own[k].data(), (size_t)(e.bytes / 4)));
      else RC(window_copy(h, ring[e.index], own[k].data(), head, size, true));
      data = own[k].data();
    }
    sec.push_back({e.tag, data, e.bytes});
  }
  std::string err;
  if (write_file(filename, info_of(h->cfg, flags, shape, st.actor_iter, st.critic_iter, st.update_counter), sec, &err)) return fail("dqnhip_save_state: %s", err.c_str());
  return 0;
}

int dqnhip_load_state(dqnhip_handle h, const char* filename) {
  if (!h || !filename) return fail("dqnhip_load_state: null argument");
  RC(state_refuse(h, (std::string("dqnhip_load_state: ") + filename).c_str()));
  RC(state_async_join(h, "dqnhip_load_state"));
  RC(snapshot_async_join(h, "dqnhip_load_state"));
  // ---- everything that can fail for the file's sake, before the learner is touched ----
  Parsed p; std::string err;
  if (read_file(filename, &p, true, &err)) return fail("dqnhip_load_state: %s", err.c_str());
  const dqnhip_state_info_t& in = p.info;
  bool same = in.state_size == h->cfg.state_size && in.num_hidden == h->cfg.num_hidden;
  for (int i = 0; same && i < h->cfg.num_hidden; ++i) same = in.hidden[i] == h->cfg.hidden[i];
  if (!same) {
    std::string a, b;
    for (int i = 0; i < std::min(std::max(in.num_hidden, 0), kMaxL); ++i) a += (i ? "," : "") + std::to_string(in.hidden[i]);
    for (int i = 0; i < h->cfg.num_hidden; ++i) b += (i ? "," : "") + std::to_string(h->cfg.hidden[i]);
    return fail("dqnhip_load_state: %s: the file's nets (state_size %d, hidden %s) are not this learner's (state_size %d, hidden %s)", filename,
                in.state_size, a.c_str(), h->cfg.state_size, b.c_str());
  }
  if (in.solver_type != h->cfg.solver_type)
    return fail("dqnhip_load_state: %s: the file was written by a learner with the %s solver, this learner's solver is %s (the histories mean something else)", filename,
                dqnhip_solver_name(in.solver_type), dqnhip_solver_name(h->cfg.solver_type));
  // What this learner's nets and the file's header say the sections are: every expected size comes from here.  (The optional
  // sections are all listed, for their sizes; which of them the file must hold is decided below.  The sections are found by tag:
  // the file's order is the container's business.)
  const bool with_mem = in.has_memory != 0;
  StateShape shape = state_shape_of(h, with_mem, in.memory_size, 0);
  shape.has_lr = shape.has_loss_scale = true; shape.has_per = with_mem && in.has_per;
  const std::vector<ManifestEntry> man = manifest(shape);
  // a section of exactly the manifest's bytes
  auto need = [&](uint32_t tag, const uint8_t** out) -> int {
    uint64_t bytes = 0;
    for (const ManifestEntry& m : man) if (m.tag == tag) bytes = m.bytes;
    const Entry* e = p.find(tag);
    if (!e) return fail("dqnhip_load_state: %s: section %s is missing", filename, tag_name(tag).c_str());
    if (e->bytes != bytes) return fail("dqnhip_load_state: %s: section %s holds %llu bytes, expected %llu", filename, tag_name(tag).c_str(),
                                       (unsigned long long)e->bytes, (unsigned long long)bytes);
    *out = p.at(e);
    return 0;
  };
  // ... into one of the fixed structs (the sections are packed back to back: not aligned)
  auto need_as = [&](uint32_t tag, auto* out) -> int { const uint8_t* q = nullptr; RC(need(tag, &q)); memcpy(out, q, sizeof *out); return 0; };
  // the schedule and the decay: both sides must agree, in either direction (the rate of every later step depends on them)
  {
    const bool theirs_has = p.find(kTagLrSched) != nullptr, mine = has_policy(h) || has_decay(h);
    LrSection theirs{};
    if (theirs_has) RC(need_as(kTagLrSched, &theirs));
    const LrSection ours = state_fixed_of(h).lr;
    if (theirs_has != mine || (theirs_has && memcmp(&theirs, &ours, sizeof ours) != 0)) {
      const char* tn = theirs_has ? dqnhip_lr_policy_name(theirs.policy) : "fixed";
      return fail("dqnhip_load_state: %s: the file was written by a learner with lr_policy %s / weight_decay %g, this learner has lr_policy %s / weight_decay %g "
                  "(or another parameter of the schedule, the base rates or the kind of decay differs)", filename, tn ? tn : "?", theirs_has ? (double)theirs.weight_decay : 0.0,
                  dqnhip_lr_policy_name(h->cfg.lr_policy), (double)h->cfg.weight_decay);
    }
  }
  const uint8_t* q_arr[kRingArrays] = {nullptr};
  const uint8_t*& q_pl = q_arr[kRingArrays - 1];
  RingSection ring{}; PerSection per{};
  if (with_mem) {
    if (in.replay_capacity != h->ring.cap) return fail("dqnhip_load_state: %s: the file's replay capacity %d is not this learner's %d", filename, in.replay_capacity, h->ring.cap);
    if ((in.has_per != 0) != (h->per != nullptr))
      return fail(in.has_per ? "dqnhip_load_state: %s: the file holds priorities, this learner samples uniformly (dqnhip_per_enable first, or save with DQNHIP_STATE_NO_MEMORY)"
                             : "dqnhip_load_state: %s: the file holds no priorities, this learner has prioritized replay enabled", filename);
    if (in.has_per) {
      RC(need_as(kTagPerCfg, &per));
      if (__builtin_bit_cast(uint32_t, per.alpha) != __builtin_bit_cast(uint32_t, h->per->cfg.alpha))
        return fail("dqnhip_load_state: %s: the file's priorities were stored with alpha %g, this learner's alpha is %g", filename, (double)per.alpha, (double)h->per->cfg.alpha);
    }
    RC(need_as(kTagRing, &ring));
    const int cap = h->ring.cap;
    if (ring.ring_size < 0 || ring.ring_size > cap || ring.ring_head < 0 || ring.ring_head >= cap || ring.ring_size != in.memory_size)
      return fail("dqnhip_load_state: %s: (ring_head, ring_size) = (%d, %d) does not fit the capacity %d / the header's memory_size %d", filename,
                  ring.ring_head, ring.ring_size, cap, in.memory_size);
    for (int i = 0; i < ring_arrays(shape.has_per); ++i) RC(need(kRingArray[i].tag, &q_arr[i]));
    if (in.has_per) {
      if (!(per.p_max >= 0.0f) || !std::isfinite(per.p_max) || !(per.beta0 >= 0.0f && per.beta0 <= 1.0f) || per.beta_anneal_iters < 0 || !(per.eps >= 0.0f) || !std::isfinite(per.eps))
        return fail("dqnhip_load_state: %s: section PERC holds values outside their ranges", filename);
      for (uint64_t i = 0; i < (uint64_t)ring.ring_size; ++i) {
        float v; memcpy(&v, q_pl + 4 * i, 4);
        if (!std::isfinite(v) || v < 0.0f) return fail("dqnhip_load_state: %s: priority %llu = %g is not finite and >= 0", filename, (unsigned long long)i, (double)v);
      }
    }
  }
  const uint8_t* q_par[kParSections] = {nullptr};
  for (int i = 0; i < kParSections; ++i) RC(need(kTagPar[i], &q_par[i]));
  DevSection dev{}; HostSection host{}; LossScaleSection ls{};
  RC(need_as(kTagDev, &dev));
  RC(need_as(kTagHost, &host));
  if (dev.actor_iter != in.actor_iter || dev.critic_iter != in.critic_iter || dev.update_counter != in.update_counter || host.seed != in.seed)
    return fail("dqnhip_load_state: %s: the header and the DEVS / HOST sections disagree", filename);
  const bool apply_ls = in.has_loss_scale && h->ls_dynamic;
  if (in.has_loss_scale) RC(need_as(kTagLossScale, &ls));
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
  for (int i = 0; i < kParSections; ++i) {
    tmp.resize(layout_of(h, par_net(i)).dense);
    memcpy(tmp.data(), q_par[i], tmp.size() * 4);  // (the sections are packed back to back: not aligned)
    RC(dqnhip_set_params(h, par_net(i), par_kind(i), tmp.data(), tmp.size()));     // W: marks the net's fp16 mirror dirty
  }
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
    // (pad columns of the ring's rows are zero from create on and no writer touches them: only the S / 10 real columns move)
    RingDev arr[kRingArrays];
    ring_arrays_of(h, arr);
    for (int i = 0; i < ring_arrays(false); ++i) RC(window_copy(h, arr[i], (void*)q_arr[i], head, size, false));
    if (h->per) {                                  // the leaves: through the tree's set pass
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
