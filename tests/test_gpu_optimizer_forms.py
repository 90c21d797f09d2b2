"""The optimiser pass in every form a real update launches it, element by element against float64 Adam (rules, bounds and the
derivation of the clip scale's error bound: tests/adam_ref.py; cases and inputs: tests/optimizer_forms_lib.py).

tests/test_gpu_optimizer_pass.py pins dqnhip_apply_update — plain k_adam_soft, no riders, its own correction, the clip norm from
k_sumsq.  Inside an update the pass is k_adam_soft_fwd1<1|2> (the critic's first layer stepped by rider workgroups, the strided pass
starting behind it), k_adam_soft_fwd1_gather<1|2> + k_adam_soft_l0 or k_adam_soft_gather (multi-update graphs: correction and soft
switch written one update ahead into DevState slot pos & 1), and the clip norm comes from the partial sums the backward's workgroups
left behind.  Here each case asserts the form through update_plan() (and the first panel's width, which selects <1> or <2>),
snapshots (w, m, v, w') of both nets, runs ONE update the way the case says, reads the gradient the pass consumed (it stays in the
arena) and the state after, and calls adam_ref.check for both nets: m, v, the step and the target per element, the APPLIED clip scale
(least squares over the whole net) against clip / ||g|| within the derived delta_s, the target bit-identical when the switch is off.
The coverage condition (every blob holds at least 50 delta_s of sum g^2, so that a dropped partial of ANY blob moves the applied scale
by more than the check allows) is asserted on the gradient read back; tests/test_adam_ref_host.py shows it on the CPU beforehand.

fp16 learner: the same comparator on the fp32 masters, and after every update the fp16 mirrors (debug_read("w16_<net>")) must be
float16(master) bit for bit — online nets and targets, switch on and off.

docs/MEASUREMENTS.md has the worst observed error / bound per case.
"""
import time

import numpy as np
import pytest

import adam_ref as A
import optimizer_forms_lib as L

pytestmark = pytest.mark.gpu


def make(pkg, case, inp, **kw):
    args = dict(minibatch=case.B, hidden=case.hidden, memory=2 * L.REPLAY, seed=1, precision=case.precision, loss_scale=case.loss_scale,
                tuning=case.tuning, use_graph=case.mode in ("graph", "indexed", "chained"), clip_grad=case.clip, soft_update_freq=case.freq, tau=case.tau,
                loss_scale_mode=case.loss_mode)
    if case.mode == "dp":
        args.update(dp_world=1, dp_rank=0)
    args.update(kw)
    d = pkg.DQN(case.S, **args)
    for net in range(4):
        d.set_params(net, inp["w"][net])
    d.add_transitions_arrays(inp["s"], inp["a"], inp["r"], inp["mc"], inp["nx"], inp["term"])
    return d


def one_update(d, case, idx):
    if case.mode == "dp":
        d.dp_update(idx); d.read_stats()
    elif case.mode == "graph":
        d.update_async(idx); d.read_stats()
    else:
        d.UpdateActorCritic(idx)


def snapshot(pkg, d, case):
    if case.dp == "shard":
        d.dp_gather_state()
    return {net: A.State(d.get_params(net), d.get_params(net, pkg.KIND_M), d.get_params(net, pkg.KIND_V), d.get_params(net + 2)) for net in (0, 1)}


def layouts(case):
    fp16 = case.precision == "fp16"
    return {0: A.layout(case.S, case.hidden, True, fp16), 1: A.layout(case.S + L.NO, case.hidden, False, fp16)}


def hypers(d, case):
    return {0: A.hyper(d.cfg.actor_lr, clip=case.clip, tau=case.tau, soft_update_freq=case.freq),
            1: A.hyper(d.cfg.critic_lr, clip=case.clip, tau=case.tau, soft_update_freq=case.freq)}


def assert_plan(d, case, lays):
    forms = d.update_plan()["forms"]
    for f in case.want:
        assert f in forms, (case.name, "the plan no longer takes", f, forms)
    for f in case.forbid:
        assert f not in forms, (case.name, "the plan now takes", f, forms)
    for net in (0, 1):
        assert d.param_count(net) == lays[net].dense, (case.name, net)
    return forms


def compare(pkg, d, case, lays, forms, before, iters, tag):
    """both nets of the update that ran last against float64 Adam of (before, the gradient in the arena); iters: (actor, critic)
    iterations before that update"""
    after = snapshot(pkg, d, case)
    hp = hypers(d, case)
    soft = A.soft_switch(hp[0], iters[0], iters[1])
    out = {}
    for net in (0, 1):
        g = d.get_params(net, pkg.KIND_G)
        if "data_parallel" in forms:
            ds = A.delta_s(A.depth_arena(lays[net], sharded=case.dp == "shard"))
        else:
            ds = A.delta_s(A.depth_update(lays[net], case.precision))
        s_ref, nrm = A.clip_scale(hp[net], g)
        if case.clip >= 0 and case.clip < 1e3:
            assert s_ref < 1.0, (tag, net, "the clip is not active: ||g|| =", nrm, "clip", case.clip)
            assert A.uncovered_blobs(lays[net], g, ds) == [], (tag, net, "blobs below 50 delta_s of sum g^2", ds)
        else:
            assert s_ref == 1.0, (tag, net, nrm)
        r = A.check("%s net %d" % (tag, net), hp[net], lays[net], before[net], g, after[net], iters[net] + 1, soft, ds)
        print("ADAMFORMS %-34s net %d t %d soft %d  m %.3f v %.3f step %.3f target %.3f  s_ref %.4e s_err %.2e ds %.2e noise %.1e"
              % (tag, net, iters[net] + 1, soft, r["m"], r["v"], r["step"], r["target"], r["s_ref"], r.get("s_err", -1.0), r["ds"], r.get("s_noise", 0.0)))
        out[net] = r
    assert d.skipped_steps() == 0, tag
    if case.precision == "fp16":
        for net in range(4):
            A.check_mirror(tag, "w16_%d" % net, d.debug_read("w16_%d" % net), d.get_params(net))
    return after, soft


def run_plain(pkg, case, inp, lays):
    """eager / graph / dp: WARMUP updates, then n_updates compared ones, one after the other"""
    d = make(pkg, case, inp)
    try:
        if case.mode == "dp":
            d.dp_init(pkg.DQN.dp_unique_id(), half_grads=case.dp == "half", shard_opt=case.dp == "shard")
        forms = assert_plan(d, case, lays)
        for row in inp["warm"]:
            one_update(d, case, row)
        softs = []
        for u, row in enumerate(inp["idx"]):
            before, iters = snapshot(pkg, d, case), (d.actor_iter(), d.critic_iter())
            assert iters == (L.WARMUP + u, L.WARMUP + u)
            one_update(d, case, row)
            softs.append(compare(pkg, d, case, lays, forms, before, iters, "%s[%d]" % (case.name, u))[1])
        if case.mode == "dp":
            d.dp_gather_state(); d.dp_destroy()
        return softs
    finally:
        d.close()


def run_indexed(pkg, case, inp, lays):
    """update k of update_indexed_n(idx[:k]) against float64 Adam of a sequential twin's state after k - 1 updates"""
    twin = make(pkg, case, inp)
    states, softs = [], []
    try:
        for row in inp["warm"]:
            twin.UpdateActorCritic(row)
        for row in inp["idx"]:
            states.append(snapshot(pkg, twin, case))
            twin.UpdateActorCritic(row)
    finally:
        twin.close()
    for k in range(1, case.n_updates + 1):
        d = make(pkg, case, inp)
        try:
            forms = assert_plan(d, case, lays)
            for row in inp["warm"]:
                d.UpdateActorCritic(row)
            d.update_indexed_n(inp["idx"][:k])
            assert len(d.collect_stats()) == k
            # the k updates ran as captured multi-update graphs (without use_graph, or after a failed capture, the call falls back to
            # one eager update after the other — the plain forms): kernel nodes of the [16, 8, 4, 2, 1]-update graphs
            nodes = d.debug_read("indexed_graph_launches")[:5]
            assert [n > 0 for n in nodes] == [False, False, k == 4, k in (2, 3), k in (1, 3)], (case.name, k, nodes)
            assert d.actor_iter() == L.WARMUP + k
            it = L.WARMUP + k - 1
            softs.append(compare(pkg, d, case, lays, forms, states[k - 1], (it, it), "%s[k=%d]" % (case.name, k))[1])
        finally:
            d.close()
    return softs


def run_chained(pkg, case, inp, lays):
    d = make(pkg, case, inp)
    try:
        forms = assert_plan(d, case, lays)
        assert d.cfg.use_graph and "early_gather_l0" in forms      # what dqnhip_update_chained needs to chain at all (else it is dqnhip_update)
        for row in inp["warm"]:
            d.UpdateActorCritic(row)
        softs = []
        idx = inp["idx"]
        for u in range(case.n_updates):
            before, iters = snapshot(pkg, d, case), (d.actor_iter(), d.critic_iter())
            d.UpdateActorCriticChained(idx[u], idx[u + 1] if u + 1 < len(idx) else idx[0])      # the second call's scalars were left by the first one's rider (ahead == -2)
            softs.append(compare(pkg, d, case, lays, forms, before, iters, "%s[%d]" % (case.name, u))[1])
        return softs
    finally:
        d.close()


def run_shared(pkg, case, inp, lays):
    """the sharer's step lands in the OWNER's arena for the shared first layer of each net and in its own beyond it"""
    owner, other = make(pkg, case, inp), make(pkg, case, inp)
    try:
        owner.ShareParameters(other, 1, 1)
        forms = assert_plan(other, case, lays)
        assert "critic_l0_rides" not in forms        # a shared first layer is stepped by the strided pass (w_sh / n4_sh)
        for row in inp["warm"]:
            other.UpdateActorCritic(row)
        before, iters = snapshot(pkg, other, case), (other.actor_iter(), other.critic_iter())
        own0 = {net: owner.get_params(net) for net in range(4)}
        other.UpdateActorCritic(inp["idx"][0])
        after, soft = compare(pkg, other, case, lays, forms, before, iters, case.name)
        for net in (0, 1):
            cut = lays[net].blobs[2][1]              # dense index of the first element behind layer 0's weights and biases
            assert lays[net].arena_index[cut] == lays[net].w_off[1] and lays[net].w_off[1] % 4 == 0
            for n, mine in ((net, after[net].w), (net + 2, after[net].wt)):
                own1 = owner.get_params(n)
                np.testing.assert_array_equal(own1[:cut], mine[:cut])                       # the prefix IS the owner's storage ...
                assert (own1[cut - 4:cut] != own0[n][cut - 4:cut]).all(), (n, "last float4 of the prefix")
                np.testing.assert_array_equal(own1[cut:], own0[n][cut:])                    # ... and nothing behind it is
            assert (after[net].w[cut:cut + 4] != before[net].w[cut:cut + 4]).all(), (net, "first float4 behind the prefix: the sharer's own arena")
        return [soft]
    finally:
        other.close(); owner.close()


RUN = {"eager": run_plain, "graph": run_plain, "dp": run_plain, "indexed": run_indexed, "chained": run_chained, "shared": run_shared}


@pytest.mark.parametrize("name", [c.name for c in L.CASES])
def test_optimizer_form(pkg, gpu, name):
    case = L.CASE_BY_NAME[name]
    t0 = time.time()
    inp = L.make_inputs(case)
    lays = layouts(case)
    if name.startswith("fwd1_k64") or name.startswith("indexed_k64"):
        assert lays[1].kp[0] == 64          # FirstLayerRider::Kp == 64: k_adam_soft_fwd1<1> / k_adam_soft_fwd1_gather<1>
    if name.startswith("fwd1_k128") or name.startswith("indexed_k128") or name == "chained_k128":
        assert lays[1].kp[0] == 128         # <2>
    if "riders" in name:
        assert lays[1].dims[1] // 16 == int(name.split("_")[2][:-6])
    if name == "second_round":
        # more float4 behind the riders' slice than 1536 workgroups x 256 threads take in one round, and less than two rounds
        for net in (0, 1):
            n4 = lays[net].arena // 4 - lays[net].w_off[1] // 4
            assert 1536 * 256 < n4 < 2 * 1536 * 256 and n4 % 256 != 0, (net, n4)
    softs = RUN[case.mode](pkg, case, inp, lays)
    if case.freq > 1:
        assert True in softs and False in softs, (name, "the soft switch must be seen on and off", softs)
    print("%s: %.2f s" % (name, time.time() - t0))
