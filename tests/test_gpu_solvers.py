"""Caffe's other solvers (SGD, Nesterov, AdaGrad, RMSProp, AdaDelta) in every form an update launches their pass, element by element
against the float64 rules (tests/solver_ref.py: rules, bounds and their derivation; cases and hyper-parameters:
tests/solver_forms_lib.py; inputs: tests/optimizer_forms_lib.py).  The frame is tests/test_gpu_optimizer_forms.py's: WARMUP updates,
snapshot (w, history 1, history 2, w') of both nets, ONE update the way the case says, the gradient the pass consumed read back with
KIND_G, solver_ref.check on every element of both nets.  Each case asserts its plan (the solver is reported, no first-layer rider
form) and — from the host's launch counters (debug_read("optimiser_launches")), and in the eager cases from kernel timing mode, whose
"adam" family times these launches — that the optimiser launches it made were k_solver_soft<> / k_solver_soft_gather<> and no Adam kernel.

Without a reference: history 2 of a single-history solver stays all-zero bits; Nesterov at momentum 0 is SGD at momentum 0 bit for
bit; solver_type 0 and an explicit Adam are one learner; a non-finite gradient norm skips the whole step; the v1 refusals."""
import ctypes as C
import time

import numpy as np
import pytest

import adam_ref as A
import optimizer_forms_lib as L
import solver_forms_lib as SL
import solver_ref as R

pytestmark = pytest.mark.gpu

RIDER_FORMS = ("critic_l0_rides", "early_gather_l0")


def make(pkg, sc, inp, **kw):
    case = sc.case
    args = dict(minibatch=case.B, hidden=case.hidden, memory=2 * L.REPLAY, seed=1, precision=case.precision, loss_scale=case.loss_scale,
                use_graph=case.mode in ("graph", "indexed", "chained"), clip_grad=case.clip, soft_update_freq=case.freq, tau=case.tau,
                loss_scale_mode=case.loss_mode, solver=sc.solver)
    args.update(SL.HYPER[sc.solver])
    args.update(kw)
    d = pkg.DQN(case.S, **args)
    for net in range(4):
        d.set_params(net, inp["w"][net])
    d.add_transitions_arrays(inp["s"], inp["a"], inp["r"], inp["mc"], inp["nx"], inp["term"])
    if sc.per:
        d.enable_prioritized_replay(alpha=0.6, beta0=0.4)
    return d


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


def assert_plan(d, sc, lays):
    plan = d.update_plan()
    assert plan["solver"] == sc.solver == d.solver, (sc.name, plan)
    for f in RIDER_FORMS:
        assert f not in plan["forms"], (sc.name, "a rider form on a learner whose solver is not Adam", plan)
    for f in sc.case.want:
        assert f in plan["forms"], (sc.name, f, plan)
    assert ("prioritized" in plan["forms"]) == sc.per
    for net in (0, 1):
        assert d.param_count(net) == lays[net].dense, (sc.name, net)
    return plan


def assert_launches(d, tag, base, want_gather=None):
    """every optimiser launch this learner enqueued or captured since `base` was read (behind assert_plan: the plan's own captures
    count too) was one of the new kernels"""
    adam, plain, gather = d.debug_read("optimiser_launches") - base
    assert d.debug_read("optimiser_launches")[0] == 0 and adam == 0 and plain + gather > 0, (tag, adam, plain, gather)
    if want_gather is not None:
        assert (gather > 0) == want_gather, (tag, adam, plain, gather)
    return plain, gather


def compare(pkg, d, sc, lays, before, iters, tag):
    case = sc.case
    after = snapshot(pkg, d)
    hp = SL.hypers(sc)
    soft = A.soft_switch(hp[0], iters[0], iters[1])
    for net in (0, 1):
        g = d.get_params(net, pkg.KIND_G)
        ds = A.delta_s(A.depth_update(lays[net], case.precision))
        s_ref, nrm = A.clip_scale(hp[net], g)
        if 0 <= case.clip < 1e3:
            assert s_ref < 1.0, (tag, net, "the clip is not active: ||g|| =", nrm, "clip", case.clip)
            assert A.uncovered_blobs(lays[net], g, ds) == [], (tag, net, "blobs below 50 delta_s of sum g^2", ds)
        else:
            assert s_ref == 1.0, (tag, net, nrm)
        r = R.check("%s net %d" % (tag, net), sc.solver, hp[net], lays[net], before[net], g, after[net], soft, ds)
        print("SOLVERFORMS %-36s net %d soft %d  h %.3f h2 %.3f step %.3f target %.3f  s_ref %.4e s_err %.2e ds %.2e noise %.1e"
              % (tag, net, soft, r["h"], r["h2"], r["step"], r["target"], r["s_ref"], r.get("s_err", -1.0), r["ds"], r.get("s_noise", 0.0)))
        assert before[net].m.any() and (sc.solver != "AdaDelta" or before[net].v.any()), (tag, net, "the histories before the tested update are real")
        if sc.solver not in R.TWO_HISTORIES:
            assert not after[net].v.view(np.uint32).any(), (tag, net, "history 2 of a single-history solver")
    assert d.skipped_steps() == 0, tag
    if case.precision == "fp16":
        for net in range(4):
            A.check_mirror(tag, "w16_%d" % net, d.debug_read("w16_%d" % net), d.get_params(net))
    return after, soft


def run_plain(pkg, sc, inp, lays):
    case = sc.case
    d = make(pkg, sc, inp)
    try:
        assert_plan(d, sc, lays)
        base = d.debug_read("optimiser_launches")
        for row in inp["warm"]:
            one_update(d, case, row)
        softs = []
        for u, row in enumerate(inp["idx"]):
            before, iters = snapshot(pkg, d), (d.actor_iter(), d.critic_iter())
            assert iters == (L.WARMUP + u, L.WARMUP + u)
            one_update(d, case, row)
            softs.append(compare(pkg, d, sc, lays, before, iters, "%s[%d]" % (sc.name, u))[1])
        plain, gather = assert_launches(d, sc.name, base, want_gather=False)
        if case.mode == "eager":
            # kernel timing mode: the two optimiser launches of one more update are timed under the optimiser family, and both are new kernels
            d.set_kernel_timing(True)
            d.UpdateActorCritic(inp["idx"][0])
            ms, n = d.kernel_timing("adam")
            d.set_kernel_timing(False)
            assert n == 2 and ms > 0, (sc.name, ms, n)
            assert tuple(d.debug_read("optimiser_launches") - base) == (0, plain + 2, 0), sc.name
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
        for row in inp["idx"]:
            states.append(snapshot(pkg, twin))
            twin.UpdateActorCritic(row)
    finally:
        twin.close()
    for k in range(1, case.n_updates + 1):
        d = make(pkg, sc, inp)
        try:
            assert_plan(d, sc, lays)
            base = d.debug_read("optimiser_launches")
            for row in inp["warm"]:
                d.UpdateActorCritic(row)
            d.update_indexed_n(inp["idx"][:k])
            assert len(d.collect_stats()) == k
            nodes = d.debug_read("indexed_graph_launches")[:5]       # kernel nodes of the [16, 8, 4, 2, 1]-update graphs
            assert [n > 0 for n in nodes] == [False, False, k == 4, k in (2, 3), k in (1, 3)], (sc.name, k, nodes)
            assert d.actor_iter() == L.WARMUP + k
            it = L.WARMUP + k - 1
            softs.append(compare(pkg, d, sc, lays, states[k - 1], (it, it), "%s[k=%d]" % (sc.name, k))[1])
            # a graph of two or more updates carries the next update's gather in every update's last launch but the last one's
            assert_launches(d, "%s[k=%d]" % (sc.name, k), base, want_gather=k >= 2)
        finally:
            d.close()
    return softs


def run_chained(pkg, sc, inp, lays):
    """dqnhip_update_chained on a learner without the rider forms: the plain update, twice"""
    case = sc.case
    d = make(pkg, sc, inp)
    try:
        assert_plan(d, sc, lays)
        base = d.debug_read("optimiser_launches")
        for row in inp["warm"]:
            d.UpdateActorCritic(row)
        softs, idx = [], inp["idx"]
        for u in range(case.n_updates):
            before, iters = snapshot(pkg, d), (d.actor_iter(), d.critic_iter())
            d.UpdateActorCriticChained(idx[u], idx[u + 1] if u + 1 < len(idx) else idx[0])
            softs.append(compare(pkg, d, sc, lays, before, iters, "%s[%d]" % (sc.name, u))[1])
        assert_launches(d, sc.name, base)
        return softs
    finally:
        d.close()


def run_shared(pkg, sc, inp, lays):
    """the sharer's step lands in the OWNER's arena for the shared first layer of each net and in its own beyond it"""
    owner, other = make(pkg, sc, inp), make(pkg, sc, inp)
    try:
        owner.ShareParameters(other, 1, 1)
        assert_plan(other, sc, lays)
        base = other.debug_read("optimiser_launches")
        for row in inp["warm"]:
            other.UpdateActorCritic(row)
        before, iters = snapshot(pkg, other), (other.actor_iter(), other.critic_iter())
        own0 = {net: owner.get_params(net) for net in range(4)}
        other.UpdateActorCritic(inp["idx"][0])
        after, soft = compare(pkg, other, sc, lays, before, iters, sc.name)
        for net in (0, 1):
            cut = lays[net].blobs[2][1]              # dense index of the first element behind layer 0's weights and biases
            assert lays[net].arena_index[cut] == lays[net].w_off[1] and lays[net].w_off[1] % 4 == 0
            for n, mine in ((net, after[net].w), (net + 2, after[net].wt)):
                own1 = owner.get_params(n)
                np.testing.assert_array_equal(own1[:cut], mine[:cut])                       # the prefix IS the owner's storage ...
                # (a step may be smaller than a weight's ulp under SGD: "moved" is asked of the float4 as a whole, and of every history element)
                assert (own1[cut - 4:cut] != own0[n][cut - 4:cut]).any(), (n, "last float4 of the prefix")
                np.testing.assert_array_equal(own1[cut:], own0[n][cut:])                    # ... and nothing behind it is
            assert (after[net].w[cut:cut + 4] != before[net].w[cut:cut + 4]).any(), (net, "first float4 behind the prefix: the sharer's own arena")
            assert (after[net].m[cut - 4:cut + 4] != before[net].m[cut - 4:cut + 4]).all(), (net, "history 1 on both sides of the cut")
        assert_launches(other, sc.name, base)
        return [soft]
    finally:
        other.close(); owner.close()


RUN = {"eager": run_plain, "graph": run_plain, "indexed": run_indexed, "chained": run_chained, "shared": run_shared}


@pytest.mark.parametrize("name", [c.name for c in SL.CASES])
def test_solver_form(pkg, gpu, name):
    sc = SL.CASE_BY_NAME[name]
    case = sc.case
    t0 = time.time()
    inp = L.make_inputs(case)
    lays = layouts(case)
    if name.endswith("second_round"):
        for net in (0, 1):
            n4 = lays[net].arena // 4
            assert 1536 * 256 < n4 < 2 * 1536 * 256 and n4 % 256 != 0, (net, n4)
    softs = RUN[case.mode](pkg, sc, inp, lays)
    if case.freq > 1:
        assert True in softs and False in softs, (name, "the soft switch must be seen on and off", softs)
    print("%s: %.2f s" % (name, time.time() - t0))


# ---- without a reference ---------------------------------------------------------------------------------------------------------------------------
BASE = SL.CASE_BY_NAME["SGD_eager"]


def _bits(pkg, d):
    return [d.get_params(net).view(np.uint32) for net in range(4)] + [d.get_params(net, k).view(np.uint32) for net in (0, 1) for k in (pkg.KIND_M, pkg.KIND_V)]


def _five_updates(pkg, inp, **kw):
    d = make(pkg, BASE, inp, **kw)
    try:
        rows = list(inp["warm"]) + [inp["idx"][0]] * 3
        out = [d.UpdateActorCritic(row) for row in rows[:5]]
        launches = tuple(d.debug_read("optimiser_launches"))          # (before update_plan: its captures are counted too)
        return out, _bits(pkg, d), d.update_plan(), launches
    finally:
        d.close()


@pytest.mark.parametrize("solver", [s for s in SL.NEW if s not in R.TWO_HISTORIES])
def test_second_history_stays_zero(pkg, gpu, solver):
    inp = L.make_inputs(BASE.case)
    kw = dict(SL.HYPER[solver], solver=solver)
    _, bits, _, launches = _five_updates(pkg, inp, **kw)
    assert launches == (0, 10, 0)
    for net in (0, 1):
        assert bits[4 + 2 * net].any() and not bits[5 + 2 * net].any(), (solver, net)


def test_nesterov_without_momentum_is_sgd(pkg, gpu):
    inp = L.make_inputs(BASE.case)
    a = _five_updates(pkg, inp, solver="SGD", momentum=0.0)
    b = _five_updates(pkg, inp, solver="Nesterov", momentum=0.0)
    assert np.array_equal(np.asarray(a[0], np.float32).view(np.uint32), np.asarray(b[0], np.float32).view(np.uint32))
    for x, y in zip(a[1], b[1]):
        assert np.array_equal(x, y)
    assert a[2]["solver"] == "SGD" and b[2]["solver"] == "Nesterov"


def test_zero_solver_type_is_adam(pkg, gpu):
    """a learner created with solver_type left 0 and one that names Adam are one learner, on today's plan and Adam's kernels"""
    inp = L.make_inputs(BASE.case)
    adam_kw = dict(solver="Adam", actor_lr=1e-5, critic_lr=1e-3, momentum=0.95)
    named = _five_updates(pkg, inp, **adam_kw)
    lib = pkg.capi.load()
    cfg = pkg.capi.Config()
    lib.dqnhip_default_config(C.byref(cfg), 59)
    assert cfg.solver_type == 0
    zero = _five_updates(pkg, inp, rms_decay=0.0, **adam_kw)            # (rms_decay zero-filled as well: an Adam learner reads neither)
    assert np.array_equal(np.asarray(named[0], np.float32).view(np.uint32), np.asarray(zero[0], np.float32).view(np.uint32))
    for x, y in zip(named[1], zero[1]):
        assert np.array_equal(x, y)
    assert named[2] == zero[2] and named[2]["solver"] == "Adam"
    assert "critic_l0_rides" in named[2]["forms"]                       # today's plan: the first-layer rider of the critic's optimiser launch
    assert named[3] == zero[3] == (10, 0, 0)


def test_non_finite_norm_skips_the_step(pkg, gpu):
    """an fp16 SGD learner with an oversized static loss scale: the dZ panels overflow, both nets' norms are not finite, both steps are
    skipped whole and reported"""
    sc = SL.CASE_BY_NAME["SGD_fp16_static"]
    inp = L.make_inputs(sc.case)
    d = make(pkg, sc, inp, loss_scale=2.0 ** 20)
    try:
        before, base = _bits(pkg, d), d.debug_read("optimiser_launches")
        with pytest.raises(pkg.DQNFatal, match="Gradient norm not finite"):
            d.UpdateActorCritic(inp["idx"][0])
        assert d.skipped_steps() == 2
        for x, y in zip(before, _bits(pkg, d)):
            assert np.array_equal(x, y)
        for net in range(4):
            A.check_mirror("skipped", "w16_%d" % net, d.debug_read("w16_%d" % net), d.get_params(net))
        assert_launches(d, "skipped", base)
    finally:
        d.close()


@pytest.mark.parametrize("solver", ["SGD", "AdaDelta"])
def test_refusals_name_the_solver(pkg, gpu, solver, tmp_path):
    inp = L.make_inputs(BASE.case)
    kw = dict(SL.HYPER[solver], solver=solver)
    with pytest.raises(pkg.DQNFatal, match=solver):
        make(pkg, BASE, inp, dp_world=2, dp_rank=0, **kw)
    d = make(pkg, BASE, inp, **kw)
    try:
        d.UpdateActorCritic(inp["idx"][0])
        before = _bits(pkg, d)
        with pytest.raises(pkg.DQNFatal, match=solver):
            d.dp_init(pkg.DQN.dp_unique_id())
        with pytest.raises(pkg.DQNFatal, match=solver):
            d.dp_init_file(str(tmp_path / "rendezvous"), timeout_s=5)
        with pytest.raises(pkg.DQNFatal, match=solver):
            d.diag_collect_raw()
        with pytest.raises(pkg.DQNFatal, match=solver):
            d.apply_update_sharded(pkg.CRITIC, 2)
        for x, y in zip(before, _bits(pkg, d)):
            assert np.array_equal(x, y)
        # the unsharded form runs, on the new kernel
        n0 = d.debug_read("optimiser_launches")
        d.apply_update(pkg.CRITIC)
        assert tuple(d.debug_read("optimiser_launches") - n0) == (0, 1, 0)
        assert d.critic_iter() == 2 and d.actor_iter() == 1
    finally:
        d.close()
