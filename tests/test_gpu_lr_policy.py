"""Caffe's lr policies and weight decay in every form an update launches the optimiser pass, element by element against the float64
rules (tests/sched_ref.py: rates, the regularised gradient, bounds and their derivation; cases: tests/sched_forms_lib.py — schedules and
decay chosen on the CPU by tests/test_sched_ref_host.py so that a dropped decay, the wrong kind, a decay scaled by the clip,
sign(0) = 1, a stale rate, a missing bias correction and a rate off by 1 % are each rejected on every case they apply to).

The frame is tests/test_gpu_solvers.py's: WARMUP updates, snapshot (w, history 1, history 2, w') of both nets, ONE update the way the
case says, the gradient the pass consumed read back with KIND_G, sched_ref.check on every element of both nets; then
dqnhip_get_learning_rate against the reference rate of the next iteration.  Every update of a multi-update case has another rate, so a
wrong DevState::adam_corr slot fails.  Each case asserts its plan (policy and "regularised" reported; the rider forms present on an Adam
learner with a policy and no decay, absent on every other) and, from the host's launch counters, which kernels stepped: the Adam
kernels and none of k_sched_soft<>, or k_sched_soft<> / k_sched_soft_gather<> and nothing else.

Without a reference, bit for bit: step with gamma 1 and a multistep whose first value lies beyond the run are the fixed learner; an SGD
learner with momentum 0 and the clip off lands on fl(w - fl(rate g)); sixteen single updates and one sixteen-update graph agree; a
non-finite gradient norm skips the whole step, decay included; a learner created from a config of the old struct_size and one with
every new field zero are one learner."""
import ctypes as C
import time

import numpy as np
import pytest

import adam_ref as A
import optimizer_forms_lib as L
import sched_forms_lib as SF
import sched_ref as SR
import solver_ref as R

pytestmark = pytest.mark.gpu

F32 = np.float32
RIDER_FORMS = ("critic_l0_rides", "early_gather_l0")


def make(pkg, sc, inp, **kw):
    case = sc.case
    args = dict(minibatch=case.B, hidden=case.hidden, memory=2 * L.REPLAY, seed=1, precision=case.precision, loss_scale=case.loss_scale,
                use_graph=case.mode in ("graph", "indexed", "chained"), clip_grad=case.clip, soft_update_freq=case.freq, tau=case.tau,
                loss_scale_mode=case.loss_mode)
    args.update(SF.dqn_kwargs(sc))
    args.update(kw)
    d = pkg.DQN(case.S, **args)
    for net in range(4):
        d.set_params(net, inp["w"][net])
    d.add_transitions_arrays(inp["s"], inp["a"], inp["r"], inp["mc"], inp["nx"], inp["term"])
    if sc.per:
        d.enable_prioritized_replay(alpha=0.6, beta0=0.4)
    return d


def plant_zeros(d, sc):
    """L1: exact zeros among the weights of both online nets, so that sign(0) is asked for (not under sharing: the prefix is the owner's)"""
    if sc.kind == "L1" and sc.decay and sc.case.mode != "shared":
        for net in (0, 1):
            w = d.get_params(net)
            w[::97] = 0
            d.set_params(net, w)
            assert (d.get_params(net) == 0).sum() >= w.size // 97


def one_update(d, case, idx):
    if case.mode == "graph":
        d.update_async(idx); d.read_stats()
    else:
        d.UpdateActorCritic(idx)


def snapshot(pkg, d):
    return {net: A.State(d.get_params(net), d.get_params(net, pkg.KIND_M), d.get_params(net, pkg.KIND_V), d.get_params(net + 2)) for net in (0, 1)}


def layouts(case):
    fp16 = case.precision == "fp16"
    return {0: A.layout(case.S, case.hidden, True, fp16), 1: A.layout(case.S + L.NO, case.hidden, False, fp16)}


def counters(d):
    return np.concatenate([d.debug_read("optimiser_launches"), d.debug_read("sched_launches")])


def assert_plan(d, sc, lays):
    plan = d.update_plan()
    assert plan["solver"] == sc.solver == d.solver, (sc.name, plan)
    assert plan["lr_policy"] == sc.sched.policy and plan["regularised"] == bool(sc.decay), (sc.name, plan)
    if sc.family == "sched":
        for f in RIDER_FORMS:
            assert f not in plan["forms"], (sc.name, "a rider form on a learner that steps with k_sched_soft<>", plan)
    for f in sc.case.want:
        assert f in plan["forms"], (sc.name, f, plan)
    assert ("prioritized" in plan["forms"]) == sc.per
    for net in (0, 1):
        assert d.param_count(net) == lays[net].dense, (sc.name, net)
    return plan


def assert_launches(d, sc, tag, base, want_gather=None):
    """every optimiser launch enqueued or captured since `base` (behind assert_plan: the plan's own captures count too)"""
    adam, plain, gather, s_plain, s_gather = counters(d) - base
    assert plain == 0 and gather == 0, (tag, "k_solver_soft<> on a learner with a policy or a decay", plain, gather)
    if sc.family == "adam":
        assert adam > 0 and s_plain == 0 and s_gather == 0, (tag, adam, s_plain, s_gather)
    else:
        assert adam == 0 and s_plain + s_gather > 0, (tag, adam, s_plain, s_gather)
        if want_gather is not None:
            assert (s_gather > 0) == want_gather, (tag, s_plain, s_gather)


def compare(pkg, d, sc, lays, before, iters, tag):
    case = sc.case
    after = snapshot(pkg, d)
    hp = SF.hypers(sc)
    soft = A.soft_switch(hp[0], iters[0], iters[1])
    for net in (0, 1):
        g = d.get_params(net, pkg.KIND_G)
        ds = A.delta_s(A.depth_update(lays[net], case.precision))
        s_ref, nrm = A.clip_scale(hp[net], g)
        assert s_ref < 1.0, (tag, net, "the clip is not active: ||g|| =", nrm, "clip", case.clip)
        assert A.uncovered_blobs(lays[net], g, ds) == [], (tag, net, "blobs below 50 delta_s of sum g^2", ds)
        r = SR.check("%s net %d" % (tag, net), sc.solver, hp[net], sc.sched, sc.decay, sc.kind, lays[net], before[net], g, after[net], iters[net], soft, ds)
        print("SCHEDFORMS %-44s net %d it %d soft %d  h %.3f h2 %.3f step %.3f target %.3f  rate %.4e s_ref %.4e ds %.2e"
              % (tag, net, iters[net], soft, r["h"], r["h2"], r["step"], r["target"], r["rate"], r["s_ref"], r["ds"]))
        assert before[net].m.any() and (sc.solver not in R.TWO_HISTORIES or before[net].v.any()), (tag, net, "the histories before the tested update are real")
        if sc.solver not in R.TWO_HISTORIES:
            assert not after[net].v.view(np.uint32).any(), (tag, net, "history 2 of a single-history solver")
    assert d.skipped_steps() == 0, tag
    if case.precision == "fp16":
        for net in range(4):
            A.check_mirror(tag, "w16_%d" % net, d.debug_read("w16_%d" % net), d.get_params(net))
    return after, soft


def check_rates(d, sc, tag):
    """dqnhip_get_learning_rate: the rate the next step applies, within 1 ulp of the reference"""
    hp = SF.hypers(sc)
    for net, it in ((0, d.actor_iter()), (1, d.critic_iter())):
        got, want = F32(d.learning_rate(net)), SR.rate(sc.sched, hp[net].lr, it)
        assert SR.ulps32(got, want) <= SR.RATE_ULP, (tag, net, it, float(got), float(want))


def run_plain(pkg, sc, inp, lays):
    case = sc.case
    d = make(pkg, sc, inp)
    try:
        assert_plan(d, sc, lays)
        base = counters(d)
        check_rates(d, sc, sc.name)
        for row in inp["warm"]:
            one_update(d, case, row)
            check_rates(d, sc, sc.name)
        softs = []
        for u, row in enumerate(inp["idx"]):
            plant_zeros(d, sc)
            before, iters = snapshot(pkg, d), (d.actor_iter(), d.critic_iter())
            assert iters == (L.WARMUP + u, L.WARMUP + u)
            one_update(d, case, row)
            softs.append(compare(pkg, d, sc, lays, before, iters, "%s[%d]" % (sc.name, u))[1])
            check_rates(d, sc, sc.name)
        assert_launches(d, sc, sc.name, base, want_gather=False)
        return softs
    finally:
        d.close()


def run_indexed(pkg, sc, inp, lays):
    """update k of update_indexed_n(idx[:k]) against the rule applied to a sequential twin's state after k - 1 updates"""
    case = sc.case
    twin = make(pkg, sc, inp)
    states, softs = [], []
    try:
        for row in inp["warm"]:
            twin.UpdateActorCritic(row)
        plant_zeros(twin, sc)
        for row in inp["idx"]:
            states.append(snapshot(pkg, twin))
            twin.UpdateActorCritic(row)
    finally:
        twin.close()
    for k in range(1, case.n_updates + 1):
        d = make(pkg, sc, inp)
        try:
            assert_plan(d, sc, lays)
            base = counters(d)
            for row in inp["warm"]:
                d.UpdateActorCritic(row)
            plant_zeros(d, sc)
            d.update_indexed_n(inp["idx"][:k])
            assert len(d.collect_stats()) == k
            assert d.actor_iter() == L.WARMUP + k
            it = L.WARMUP + k - 1
            softs.append(compare(pkg, d, sc, lays, states[k - 1], (it, it), "%s[k=%d]" % (sc.name, k))[1])
            check_rates(d, sc, sc.name)
            # a graph of two or more updates carries the next update's gather — whose scalars block writes the next rate — in an optimiser launch
            assert_launches(d, sc, "%s[k=%d]" % (sc.name, k), base, want_gather=k >= 2)
        finally:
            d.close()
    return softs


def run_chained(pkg, sc, inp, lays):
    case = sc.case
    d = make(pkg, sc, inp)
    try:
        assert_plan(d, sc, lays)
        base = counters(d)
        for row in inp["warm"]:
            d.UpdateActorCritic(row)
        plant_zeros(d, sc)
        softs, idx = [], inp["idx"]
        for u in range(case.n_updates):
            before, iters = snapshot(pkg, d), (d.actor_iter(), d.critic_iter())
            d.UpdateActorCriticChained(idx[u], idx[u + 1] if u + 1 < len(idx) else idx[0])
            softs.append(compare(pkg, d, sc, lays, before, iters, "%s[%d]" % (sc.name, u))[1])
            check_rates(d, sc, sc.name)
        assert_launches(d, sc, sc.name, base)
        return softs
    finally:
        d.close()


def run_shared(pkg, sc, inp, lays):
    """the sharer's step lands in the OWNER's arena for the shared first layer of each net — and its decay reads the owner's w there"""
    owner, other = make(pkg, sc, inp), make(pkg, sc, inp)
    try:
        # the sharer's own copy of the prefix is NOT what the decay may read: make it differ from the owner's (the copy is unreachable
        # once the layers are shared: the pair computes what the unshared inputs compute)
        for net in range(4):
            w = inp["w"][net].copy()
            cut = lays[net & 1].blobs[2][1]
            w[:cut] *= F32(1.5)
            other.set_params(net, w)
        owner.ShareParameters(other, 1, 1)
        assert_plan(other, sc, lays)
        base = counters(other)
        for row in inp["warm"]:
            other.UpdateActorCritic(row)
        before, iters = snapshot(pkg, other), (other.actor_iter(), other.critic_iter())
        own0 = {net: owner.get_params(net) for net in range(4)}
        other.UpdateActorCritic(inp["idx"][0])
        after, soft = compare(pkg, other, sc, lays, before, iters, sc.name)
        for net in (0, 1):
            cut = lays[net].blobs[2][1]
            for n, mine in ((net, after[net].w), (net + 2, after[net].wt)):
                own1 = owner.get_params(n)
                np.testing.assert_array_equal(own1[:cut], mine[:cut])
                np.testing.assert_array_equal(own1[cut:], own0[n][cut:])
            np.testing.assert_array_equal(before[net].w[:cut], own0[net][:cut])           # what `before` read of the prefix was the owner's
        assert_launches(other, sc, sc.name, base)
        return [soft]
    finally:
        other.close(); owner.close()


RUN = {"eager": run_plain, "graph": run_plain, "indexed": run_indexed, "chained": run_chained, "shared": run_shared}


@pytest.mark.parametrize("name", [c.name for c in SF.CASES])
def test_lr_policy_form(pkg, gpu, name):
    sc = SF.CASE_BY_NAME[name]
    case = sc.case
    t0 = time.time()
    inp = L.make_inputs(case)
    lays = layouts(case)
    softs = RUN[case.mode](pkg, sc, inp, lays)
    if case.freq > 1:
        assert True in softs and False in softs, (name, "the soft switch must be seen on and off", softs)
    print("%s: %.2f s" % (name, time.time() - t0))


# ---- without a reference ---------------------------------------------------------------------------------------------------------------------------
def _case_of(solver, policy="fixed", form="eager", decay=0.0, kind="L2", sched=None, **case_kw):
    mode, B, S, hidden, kw = SF.FORMS[form]
    kw = dict(kw, **case_kw)
    kw.pop("want", None)
    return SF.SchedCase("bits", solver, L._case("bits", mode, B, S, hidden, seed=SF.SEED[form], **kw), False, sched or SF.SCHEDULES[policy], decay, kind,
                        "sched" if (decay or solver != "Adam") else "adam")


def _bits(pkg, d):
    return [d.get_params(net).view(np.uint32) for net in range(4)] + [d.get_params(net, k).view(np.uint32) for net in (0, 1) for k in (pkg.KIND_M, pkg.KIND_V)]


def _five_updates(pkg, sc, inp, **kw):
    d = make(pkg, sc, inp, **kw)
    try:
        rows = list(inp["warm"]) + [inp["idx"][0]] * 3
        out = [d.UpdateActorCritic(row) for row in rows[:5]]
        return np.asarray(out, F32).view(np.uint32), _bits(pkg, d), tuple(counters(d))
    finally:
        d.close()


def _same(a, b):
    assert np.array_equal(a[0], b[0])
    for x, y in zip(a[1], b[1]):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("solver", ["Adam", "SGD"])
def test_policies_that_never_move_the_rate_are_the_fixed_learner(pkg, gpu, solver):
    fixed = _case_of(solver)
    inp = L.make_inputs(fixed.case)
    ref = _five_updates(pkg, fixed, inp)
    # today's kernels on the fixed learner: the Adam family, or k_solver_soft<>; none of the new family
    assert ref[2] == ((10, 0, 0, 0, 0) if solver == "Adam" else (0, 10, 0, 0, 0))
    for sched in (SR.schedule("step", gamma=1.0, stepsize=1), SR.schedule("step", gamma=1.0, stepsize=3), SR.schedule("multistep", gamma=0.1, stepvalues=(50, 60))):
        got = _five_updates(pkg, _case_of(solver, sched=sched), inp)
        _same(ref, got)
        assert got[2] == ((10, 0, 0, 0, 0) if solver == "Adam" else (0, 0, 0, 10, 0)), (solver, sched, got[2])


def test_old_struct_size_and_zero_fields_are_one_learner(pkg, gpu):
    """a learner created through the Python constructor with every new field zero, and one created from a config of the struct_size
    before the fields existed, end five updates on identical bits"""
    sc = _case_of("Adam")
    case = sc.case
    inp = L.make_inputs(case)
    ref = _five_updates(pkg, sc, inp)
    d = make(pkg, sc, inp)
    try:
        raw = bytes(d.cfg)
        a, b = pkg.capi.Config.lr_policy.offset, pkg.capi.Config.tuning_flags.offset
        assert not any(raw[a:b])
        old = bytearray(raw[:a] + raw[b:])
        old[0:4] = np.array([len(old)], np.int32).tobytes()
        buf = (C.c_char * len(old)).from_buffer(old)
        h = pkg.capi.H()
        lib = d.lib
        lib.dqnhip_create.argtypes = [C.c_void_p, C.POINTER(pkg.capi.H)]
        try:
            assert lib.dqnhip_create(C.addressof(buf), C.byref(h)) == 0, lib.dqnhip_last_error()
        finally:
            lib.dqnhip_create.argtypes = [C.POINTER(pkg.capi.Config), C.POINTER(pkg.capi.H)]
        mine, d.h = d.h, h                       # the wrapper drives the old-size learner; its own handle is destroyed below
        try:
            for net in range(4):
                d.set_params(net, inp["w"][net])
            d.add_transitions_arrays(inp["s"], inp["a"], inp["r"], inp["mc"], inp["nx"], inp["term"])
            rows = list(inp["warm"]) + [inp["idx"][0]] * 3
            out = np.asarray([d.UpdateActorCritic(row) for row in rows[:5]], F32).view(np.uint32)
            _same(ref, (out, _bits(pkg, d)))
            assert tuple(counters(d)) == (10, 0, 0, 0, 0)
            assert d.update_plan()["lr_policy"] == "fixed" and not d.update_plan()["regularised"]
        finally:
            assert lib.dqnhip_destroy(h) == 0
            d.h = mine
    finally:
        d.close()


def test_sgd_without_momentum_and_clip_is_one_fma_order(pkg, gpu):
    """w1 == fl(w0 - fl(rate g)) to the bit (sched_ref.sgd_plain32 states the order); step with gamma 0.5: every rate is exact"""
    sched = SR.schedule("step", gamma=0.5, stepsize=1)
    sc = _case_of("SGD", sched=sched, clip=-1.0)
    inp = L.make_inputs(sc.case)
    d = make(pkg, sc, inp, momentum=0.0)
    try:
        for u, row in enumerate(list(inp["warm"]) + [inp["idx"][0]]):
            w0 = {net: d.get_params(net) for net in (0, 1)}
            d.UpdateActorCritic(row)
            for net in (0, 1):
                base = F32(SF.HYPER["SGD"]["actor_lr" if net == 0 else "critic_lr"])
                rate = SR.rate(sched, base, u)
                assert rate == F32(float(base) * 0.5 ** u)
                g = d.get_params(net, pkg.KIND_G)
                h1, w1 = SR.sgd_plain32(rate, w0[net], g)
                # (values, not bit patterns: a zero product takes its sign from the fma's zero addend)
                assert np.array_equal(d.get_params(net, pkg.KIND_M), h1) and np.isfinite(h1).all(), (u, net)
                assert np.array_equal(d.get_params(net).view(np.uint32), w1.view(np.uint32)), (u, net)
                assert (w1 != w0[net]).any()
        assert tuple(counters(d)) == (0, 0, 0, 6, 0)
    finally:
        d.close()


@pytest.mark.parametrize("solver", ["Adam", "RMSProp"])
def test_sixteen_singles_equal_one_sixteen_update_graph(pkg, gpu, solver):
    """exp policy, decay on: the sixteen-update graph's riders hand every update its own rate through the two DevState slots"""
    sc = _case_of(solver, "exp", "graph", SF.DECAY, "L2", sched=SR.schedule("exp", gamma=0.8))
    inp = L.make_inputs(sc.case)
    ends = []
    for graph in (False, True):
        d = make(pkg, sc, inp, use_graph=graph)
        try:
            base = counters(d)
            if graph:
                d.update_async_n(16); d.read_stats()
            else:
                for _ in range(16):
                    d.UpdateActorCritic(None)
            assert d.actor_iter() == 16
            ends.append(_bits(pkg, d))
            adam, plain, gather, s_plain, s_gather = counters(d) - base
            # sixteen eager updates enqueue 32 launches; the graph is captured once: 17 plain launches and 15 that carry the next gather
            assert (adam, plain, gather) == (0, 0, 0) and s_plain + s_gather == 32 and s_gather == (15 if graph else 0), (graph, s_plain, s_gather)
        finally:
            d.close()
    for x, y in zip(*ends):
        assert np.array_equal(x, y)
    assert (ends[0][0] != inp["w"][0].view(np.uint32)).any()


def test_adam_policy_sixteen_singles_equal_one_graph_on_the_tuned_kernels(pkg, gpu):
    sc = _case_of("Adam", "exp", "graph", sched=SR.schedule("exp", gamma=0.8))
    inp = L.make_inputs(sc.case)
    ends = []
    for graph in (False, True):
        d = make(pkg, sc, inp, use_graph=graph)
        try:
            assert "early_gather_l0" in d.update_plan()["forms"]
            if graph:
                d.update_async_n(16); d.read_stats()
            else:
                for _ in range(16):
                    d.UpdateActorCritic(None)
            ends.append(_bits(pkg, d))
            assert tuple(d.debug_read("sched_launches")) == (0, 0)
        finally:
            d.close()
    for x, y in zip(*ends):
        assert np.array_equal(x, y)


def test_non_finite_norm_skips_the_step_decay_included(pkg, gpu):
    """an fp16 SGD learner with an oversized static loss scale and a decay: both norms are not finite, both steps are skipped whole —
    the decay alone would have moved every weight"""
    sc = _case_of("SGD", "exp", "fp16_static", SF.DECAY, "L2")
    inp = L.make_inputs(sc.case)
    d = make(pkg, sc, inp, loss_scale=2.0 ** 20)
    try:
        before = _bits(pkg, d)
        with pytest.raises(pkg.DQNFatal, match="Gradient norm not finite"):
            d.UpdateActorCritic(inp["idx"][0])
        assert d.skipped_steps() == 2
        for x, y in zip(before, _bits(pkg, d)):
            assert np.array_equal(x, y)
        assert tuple(counters(d)) == (0, 0, 0, 2, 0)
    finally:
        d.close()


@pytest.mark.parametrize("kw,needle", [(dict(policy="exp"), "lr_policy exp"), (dict(decay=1e-3), "weight_decay 0.001")])
def test_v1_refusals_name_the_policy_or_the_decay(pkg, gpu, kw, needle, tmp_path):
    sc = _case_of("Adam", **kw)
    inp = L.make_inputs(sc.case)
    with pytest.raises(pkg.DQNFatal, match=needle):
        make(pkg, sc, inp, dp_world=2, dp_rank=0)
    d = make(pkg, sc, inp)
    try:
        d.UpdateActorCritic(inp["idx"][0])
        before = _bits(pkg, d)
        for call in (lambda: d.dp_init(pkg.DQN.dp_unique_id()), lambda: d.dp_init_file(str(tmp_path / "rendezvous"), timeout_s=5),
                     lambda: d.diag_collect_raw(), lambda: d.apply_update(pkg.CRITIC), lambda: d.apply_update_sharded(pkg.CRITIC, 2)):
            with pytest.raises(pkg.DQNFatal, match=needle):
                call()
        for x, y in zip(before, _bits(pkg, d)):
            assert np.array_equal(x, y)
        assert (d.actor_iter(), d.critic_iter()) == (1, 1)
    finally:
        d.close()
