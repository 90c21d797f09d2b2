"""Dynamic loss scaling of the fp16 learner (cfg.loss_scale_mode = DQNHIP_LOSS_SCALE_DYNAMIC): two power-of-two multipliers in device
memory that the optimiser launches halve on a non-finite gradient norm and double after a run of finite steps.

What is checked, at the smallest shapes that reach every kernel that consumes a loss scale (SHAPES; each case asserts from
dqnhip_get_update_plan that it reached them):
  1. a dynamic learner whose multipliers are pinned at 2^k IS a static learner with cfg.loss_scale = 2^k: parameters of the four nets,
     Adam's m and v, the gradient arenas and (loss, avg_q), bit for bit (array_equal — powers of two commute with every rounding, so
     this is exactness, not a tolerance), eager and under graph replay; with mixed multipliers the critic follows the critic's;
  2. the dynamic learner's update plan (forms and launch counts) is the static learner's;
  3. backoff and recovery at a user scale 2^U that makes the static learner fail; 4. the floor; 5. growth and the cap;
  6. a sixteen-update graph, a chain and an indexed burst behave as sixteen single calls; 7. the refusals that need a device.

Two figures differ from the issue that asked for this test, because the issue contradicts its own rules there:
  - floor: the decision table raises the flag when the norm is not finite WHILE the multiplier is at min_mult, so with min_mult = 2^-1
    ONE update is skipped in silence (1 -> 2^-1) and the second reports, not the third.  The test runs min_mult = 2^-1 (one silent
    skip) and 2^-2 (two silent skips, the third update reports) and asserts the table's behaviour for both.
  - growth: max_mult = 2^-2 is refused by the validator (1 must lie inside [min, max]: the multipliers start at 1), so the sequence is
    the issue's times four: 2^-2 through update 4, 2^-1 through update 8, 1 (the cap) from then on.
"""
import numpy as np
import pytest

from synth import synth_replay

pytestmark = pytest.mark.gpu

S, N_REPLAY = 59, 2048
# user scale of the backoff cases: the critic's tower-top gradient panel holds 16 x user x (q - y) x w_head; with |q - y| of order 1
# (rewards up to +5) and head weights of sigma 0.01 that is ~0.1 x user against fp16's largest finite value 65504, and the dQ/da
# pass's seed panel holds 4096 x user x w_head: 2^20 overflows both by orders of magnitude, 2^20 x 2^-20 is the built-in scale.
U = 20

# name -> (minibatch, hidden, tuning bit name or None)
SHAPES = {
    "b128": (128, (128, 128), None),                                   # below kGroupMinRows: per-layer wgrads on 64x64 split-K tiles
    "b512": (512, (256, 256), None),                                   # grouped wgrad, HeadWsum, fuse_q, k_dqda_head_bwd<true>
    "b512_per_layer": (512, (256, 256), "TUNE_FP16_WGRAD_PER_LAYER"),
    "b512_sep_head": (512, (256, 256), "TUNE_SEPARATE_ACTOR_HEAD_BWD"),
    "b1024": (1024, (256, 256), None),                                 # head_backward_big, the seed_scale epilogue
}
RIDES = {"head_wgrad_rides_critic", "head_wgrad_rides_actor", "q_train_in_dgrad"}


def _make(pkg, shape, dynamic, use_graph=False, **kw):
    B, hidden, tune = SHAPES[shape]
    if dynamic:
        kw.setdefault("loss_scale_growth_interval", 0)
        kw["loss_scale_mode"] = "dynamic"
    d = pkg.DQN(S, minibatch=B, hidden=hidden, memory=2 * N_REPLAY, seed=3, precision="fp16", use_graph=use_graph,
                tuning=getattr(pkg.capi, tune) if tune else 0, **kw)
    d.add_transitions_arrays(*_replay())
    return d


_cache = {}


def _replay():
    if "replay" not in _cache:
        _cache["replay"] = synth_replay(np.random.default_rng(5), N_REPLAY, S)
    return _cache["replay"]


def _indices(B, n):
    return np.random.default_rng(7).integers(0, N_REPLAY, (n, B)).astype(np.int32)


def _state(pkg, d):
    """params of the four nets, m, v and the gradient arena of both trained nets"""
    return [d.get_params(n) for n in range(4)] + [d.get_params(n, k) for n in (0, 1) for k in (pkg.KIND_M, pkg.KIND_V, pkg.KIND_G)]


def _net_state(pkg, d, net):
    """what a skipped step of `net` must leave untouched: its params, m, v and its target"""
    return [d.get_params(net), d.get_params(net, pkg.KIND_M), d.get_params(net, pkg.KIND_V), d.get_params(net + 2)]


def _assert_reached(pkg, shape, plan):
    """the plan says that this shape reaches the consumers of a scale it is in the list for"""
    B, hidden, tune = SHAPES[shape]
    forms = set(plan["forms"])
    assert "fp16" in forms and "head_seed_fused" in forms, plan            # HGemm::seed_scale in the top forward layer's epilogue
    if shape == "b1024":
        assert not (RIDES & forms) and "dqda_head_bwd" not in forms, plan  # head_backward_big writes the scaled panels
    else:
        assert RIDES <= forms, plan                                        # k_head_q_train writes the critic's scaled panel, HeadWsum the heads' dW / db
        assert ("dqda_head_bwd" in forms) == (tune != "TUNE_SEPARATE_ACTOR_HEAD_BWD"), plan
    # grouped wgrads (>= kGroupMinRows = 512 rows) against one launch per layer: the tuning bit changes nothing at 128 rows, where both
    # are the per-layer form
    if shape in ("b128", "b512"):
        key = ("per_layer_plan", shape)
        if key not in _cache:
            d = pkg.DQN(S, minibatch=B, hidden=hidden, memory=2 * N_REPLAY, seed=3, precision="fp16", tuning=pkg.capi.TUNE_FP16_WGRAD_PER_LAYER)
            d.add_transitions_arrays(*_replay())
            _cache[key] = d.update_plan(); d.close()
        per_layer = _cache[key]
        if shape == "b128":
            assert per_layer == plan, (plan, per_layer)
        else:                                                              # (a two-layer tower: the grouped form saves no launch, it only changes the tiles)
            assert per_layer["forms"] == plan["forms"] and per_layer["launches_single"] >= plan["launches_single"], (plan, per_layer)


def _static_run(pkg, shape, k, use_graph, n_up=3):
    key = ("static", shape, k, use_graph, n_up)
    if key not in _cache:
        d = _make(pkg, shape, False, use_graph, loss_scale=2.0 ** k)
        stats = [d.UpdateActorCritic(i) for i in _indices(SHAPES[shape][0], n_up)]
        _cache[key] = (stats, _state(pkg, d), d.update_plan(), d.skipped_steps())
        d.close()
    return _cache[key]


CASES1 = [(s, k, g) for s in SHAPES for k in (-2, 0) for g in (False, True)] + [("b512", 3, False), ("b512", 3, True)]


@pytest.mark.parametrize("shape,k,use_graph", CASES1, ids=["%s-k%d-%s" % (s, k, "graph" if g else "eager") for s, k, g in CASES1])
def test_pinned_multiplier_is_a_static_scale(pkg, gpu, shape, k, use_graph):
    """cases 1 and 2"""
    stats_s, state_s, plan_s, skipped_s = _static_run(pkg, shape, k, use_graph)
    assert skipped_s == 0
    d = _make(pkg, shape, True, use_graph, loss_scale_max_mult=max(1.0, 2.0 ** k))
    d.set_loss_scale(2.0 ** k, 2.0 ** k)
    plan = d.update_plan()
    _assert_reached(pkg, shape, plan)
    assert plan == plan_s, (plan, plan_s)                                  # same forms, same launch counts, stand-alone and in-graph
    stats = [d.UpdateActorCritic(i) for i in _indices(SHAPES[shape][0], 3)]
    assert stats == stats_s, (stats, stats_s)
    for got, want in zip(_state(pkg, d), state_s):
        np.testing.assert_array_equal(got, want)
    ls = d.loss_scale_state()
    assert (ls["mode"], ls["mult_critic"], ls["mult_actor"], ls["good_critic"], ls["good_actor"]) == ("dynamic", 2.0 ** k, 2.0 ** k, 3, 3), ls
    assert ls["skipped_steps"] == ls["backoffs_critic"] == ls["backoffs_actor"] == ls["growths_critic"] == ls["growths_actor"] == 0, ls
    assert d.update_plan() == plan_s
    d.close()


@pytest.mark.parametrize("kc,ka", [(-3, -1), (-1, -3)])
def test_mixed_multipliers_critic_follows_the_critic(pkg, gpu, kc, ka):
    """case 1, mixed: after the FIRST update the critic's params, m and v are the static 2^kc learner's (a critic / actor mix-up
    would give the static 2^ka learner's)"""
    shape = "b512"
    key = ("static1", kc)
    if key not in _cache:
        s = _make(pkg, shape, False, loss_scale=2.0 ** kc)
        s.UpdateActorCritic(_indices(512, 1)[0])
        _cache[key] = [s.get_params(1), s.get_params(1, pkg.KIND_M), s.get_params(1, pkg.KIND_V)]
        s.close()
    d = _make(pkg, shape, True)
    d.set_loss_scale(2.0 ** kc, 2.0 ** ka)
    d.UpdateActorCritic(_indices(512, 1)[0])
    for got, want in zip([d.get_params(1), d.get_params(1, pkg.KIND_M), d.get_params(1, pkg.KIND_V)], _cache[key]):
        np.testing.assert_array_equal(got, want)
    ls = d.loss_scale_state()
    assert (ls["mult_critic"], ls["mult_actor"]) == (2.0 ** kc, 2.0 ** ka)
    d.close()


def _controls(pkg, shape, n):
    """the static twin at 2^U fails at once, for both nets; the default-scale static learner takes every step on these inputs"""
    key = ("controls", shape, n)
    if key in _cache:
        return
    idx = _indices(SHAPES[shape][0], n)
    s = _make(pkg, shape, False, loss_scale=2.0 ** U)
    with pytest.raises(pkg.DQNFatal, match="Gradient norm not finite"):
        s.UpdateActorCritic(idx[0])
    assert s.skipped_steps() == 2                                          # the critic's step and the actor's
    s.close()
    s = _make(pkg, shape, False)
    for i in idx:
        loss, q = s.UpdateActorCritic(i)
        assert np.isfinite(loss) and np.isfinite(q)
    assert s.skipped_steps() == 0
    s.close()
    _cache[key] = True


@pytest.mark.parametrize("shape", ["b128", "b512"])
def test_backoff_and_recovery(pkg, gpu, shape):
    """case 3"""
    B = SHAPES[shape][0]
    n_max = U + 1 + 5
    _controls(pkg, shape, n_max)
    idx = _indices(B, n_max)
    d = _make(pkg, shape, True, loss_scale=2.0 ** U, loss_scale_min_mult=2.0 ** -U)
    ls = d.loss_scale_state()
    skips = {0: 0, 1: 0}
    first_step = {0: None, 1: None}
    mult_name = {0: "mult_actor", 1: "mult_critic"}
    t = 0
    clean_run = 0
    while clean_run < 5:
        assert t < n_max, (skips, ls)
        before = {net: _net_state(pkg, d, net) for net in (0, 1)}
        loss, q = d.UpdateActorCritic(idx[t])                              # no update call may fail
        after = d.loss_scale_state()
        skipped_now = 0
        for net in (0, 1):
            now = _net_state(pkg, d, net)
            m0, m1 = ls[mult_name[net]], after[mult_name[net]]
            if m1 != m0:                                                   # skipped: halved, everything of the net bit-unchanged
                assert m1 == m0 / 2, (t, net, m0, m1)
                for x, y in zip(before[net], now):
                    np.testing.assert_array_equal(x, y)
                skips[net] += 1; skipped_now += 1
                assert first_step[net] is None, "net %d skipped a step after it had recovered (update %d): %r" % (net, t, after)
            else:                                                          # taken: the multiplier is unchanged, the net moved
                assert not np.array_equal(before[net][0], now[0]), (t, net)
                if first_step[net] is None:
                    first_step[net] = t
        assert after["skipped_steps"] == ls["skipped_steps"] + skipped_now, (t, ls, after)
        print("update", t, "loss", loss, "avg_q", q, after)
        clean_run = clean_run + 1 if (first_step[0] is not None and first_step[1] is not None and skipped_now == 0) else 0
        if clean_run:
            assert np.isfinite(loss) and np.isfinite(q)
        ls = after
        t += 1
    # each net took a step after at most U skips: there the total scale is the built-in one, which the control shows to be in range
    assert 1 <= skips[0] <= U and 1 <= skips[1] <= U, skips
    assert ls["backoffs_actor"] == skips[0] and ls["backoffs_critic"] == skips[1] and ls["skipped_steps"] == skips[0] + skips[1], (ls, skips)
    assert ls["mult_actor"] == 2.0 ** -skips[0] and ls["mult_critic"] == 2.0 ** -skips[1]
    d.read_stats()                                                         # clean flags
    d.close()


@pytest.mark.parametrize("floor_log2", [1, 2])
def test_floor_reports_as_static_mode_does(pkg, gpu, floor_log2):
    """case 4 (see the module docstring): floor_log2 silent skips take the multipliers to the floor; the next update finds them there
    and reports — once — and they stay."""
    shape = "b128"
    _controls(pkg, shape, U + 1 + 5)
    idx = _indices(SHAPES[shape][0], floor_log2 + 2)
    d = _make(pkg, shape, True, loss_scale=2.0 ** U, loss_scale_min_mult=2.0 ** -floor_log2)
    w0 = _state(pkg, d)[:4]
    for t in range(floor_log2):
        d.UpdateActorCritic(idx[t])                                        # skipped in silence
    ls = d.loss_scale_state()
    assert ls["mult_critic"] == ls["mult_actor"] == 2.0 ** -floor_log2 and ls["skipped_steps"] == 2 * floor_log2, ls
    with pytest.raises(pkg.DQNFatal, match="Gradient norm not finite"):
        d.UpdateActorCritic(idx[floor_log2])
    d.read_stats()                                                         # reported exactly once: the flag is clear again
    ls = d.loss_scale_state()
    assert ls["mult_critic"] == ls["mult_actor"] == 2.0 ** -floor_log2, ls
    assert ls["skipped_steps"] == 2 * floor_log2 + 2 and ls["backoffs_critic"] == ls["backoffs_actor"] == floor_log2, ls
    for got, want in zip(_state(pkg, d)[:4], w0):                          # every step so far was skipped
        np.testing.assert_array_equal(got, want)
    assert d.actor_iter() == floor_log2 + 1                                # the iterations tick on a skipped step
    d.close()


def test_growth_and_cap(pkg, gpu):
    """case 5 (see the module docstring for the factor of four)"""
    shape = "b128"
    idx = _indices(SHAPES[shape][0], 13)
    d = _make(pkg, shape, True, loss_scale_growth_interval=4, loss_scale_max_mult=1.0)
    d.set_loss_scale(0.25, 0.25)
    for t in range(1, 14):
        d.UpdateActorCritic(idx[t - 1])
        ls = d.loss_scale_state()
        assert ls["skipped_steps"] == 0, "a step was skipped on these inputs (update %d): %r" % (t, ls)
        want = 0.25 if t < 4 else 0.5 if t < 8 else 1.0
        assert ls["mult_critic"] == ls["mult_actor"] == want, (t, ls)
        assert ls["good_critic"] == ls["good_actor"] == t % 4, (t, ls)
        assert ls["growths_critic"] == ls["growths_actor"] == min(t // 4, 2), (t, ls)
    d.close()


def _single_calls(pkg, shape, idx):
    """sixteen single calls on a dynamic learner at user scale 2^U: explicit indices (idx [16, B]) or device sampling (None)"""
    key = ("singles", shape, idx is None)
    if key not in _cache:
        d = _make(pkg, shape, True, loss_scale=2.0 ** U, loss_scale_min_mult=2.0 ** -U)
        stats = [d.UpdateActorCritic(None if idx is None else idx[t]) for t in range(16)]
        _cache[key] = (stats, _state(pkg, d), d.loss_scale_state())
        d.close()
    return _cache[key]


def _assert_backoffs_then_steps(ls):
    """the sixteen updates cover, for each net, backoffs AND steps taken after them (else the comparison would be of untouched nets)"""
    for net in ("critic", "actor"):
        assert 1 <= ls["backoffs_" + net] < 16 and ls["good_" + net] == 16 - ls["backoffs_" + net] > 0, ls


def test_inside_a_graph_as_outside(pkg, gpu):
    """case 6: one dqnhip_update_async_n(16) against sixteen single calls, device sampling; the backoffs fall inside the graph"""
    shape = "b128"
    stats_s, state_s, ls_s = _single_calls(pkg, shape, None)
    _assert_backoffs_then_steps(ls_s)
    d = _make(pkg, shape, True, loss_scale=2.0 ** U, loss_scale_min_mult=2.0 ** -U)
    d.update_async_n(16)
    assert d.read_stats() == stats_s[-1]
    for got, want in zip(_state(pkg, d), state_s):
        np.testing.assert_array_equal(got, want)
    assert d.loss_scale_state() == ls_s
    d.close()


@pytest.mark.parametrize("how", ["chained", "indexed_n"])
def test_chained_and_indexed_bursts_as_single_calls(pkg, gpu, how):
    """case 6, host indices: dqnhip_update_chained and dqnhip_update_indexed_n"""
    shape = "b128"
    idx = _indices(SHAPES[shape][0], 16)
    stats_s, state_s, ls_s = _single_calls(pkg, shape, idx)
    _assert_backoffs_then_steps(ls_s)
    d = _make(pkg, shape, True, use_graph=True, loss_scale=2.0 ** U, loss_scale_min_mult=2.0 ** -U)
    if how == "chained":
        stats = [d.UpdateActorCriticChained(idx[t], idx[t + 1] if t + 1 < 16 else None) for t in range(16)]
    else:
        d.update_indexed_n(idx)
        stats = d.collect_stats()
    assert [tuple(s) for s in stats] == [tuple(s) for s in stats_s]
    for got, want in zip(_state(pkg, d), state_s):
        np.testing.assert_array_equal(got, want)
    assert d.loss_scale_state() == ls_s
    d.close()


def test_refusals_that_need_a_device(pkg, gpu, tmp_path):
    """case 7"""
    shape = "b128"
    s = _make(pkg, shape, False)
    with pytest.raises(pkg.DQNFatal, match="static"):
        s.set_loss_scale(1.0, 1.0)
    ls = s.loss_scale_state()
    assert (ls["mode"], ls["mult_critic"], ls["mult_actor"]) == ("static", 1.0, 1.0)
    s.close()
    d = _make(pkg, shape, True, loss_scale_min_mult=2.0 ** -4, loss_scale_max_mult=2.0)
    for c, a, what in ((0.3, 1.0, "mult_critic.*power of two"), (1.0, 3.0, "mult_actor.*power of two"), (0.0, 1.0, "power of two"), (-1.0, 1.0, "power of two"),
                       (2.0 ** -5, 1.0, "mult_critic.*outside"), (1.0, 4.0, "mult_actor.*outside")):
        with pytest.raises(pkg.DQNFatal, match=what):
            d.set_loss_scale(c, a)
    d.set_loss_scale(2.0 ** -4, 2.0)
    assert (d.loss_scale_state()["mult_critic"], d.loss_scale_state()["mult_actor"]) == (2.0 ** -4, 2.0)
    d.set_loss_scale(1.0, 1.0)
    with pytest.raises(pkg.DQNFatal, match="dynamic"):
        d.dp_init_file(str(tmp_path / "rendezvous"), timeout_s=5)
    with pytest.raises(pkg.DQNFatal, match="dynamic"):
        d.dp_init(pkg.DQN.dp_unique_id())
    # dqnhip_apply_update with an inf in the gradient arena behaves as static mode: skips, reports, leaves the multiplier alone
    d.UpdateActorCritic(_indices(SHAPES[shape][0], 1)[0])
    for net in (pkg.CRITIC, pkg.ACTOR):
        g = d.get_params(net, pkg.KIND_G)
        g[5] = np.inf
        d.set_params(net, g, pkg.KIND_G)
        before = _net_state(pkg, d, net)
        ls0 = d.loss_scale_state()
        d.apply_update(net)
        with pytest.raises(pkg.DQNFatal, match="Gradient norm not finite"):
            d.read_stats()
        ls1 = d.loss_scale_state()
        assert ls1["skipped_steps"] == ls0["skipped_steps"] + 1
        assert {k: v for k, v in ls1.items() if k != "skipped_steps"} == {k: v for k, v in ls0.items() if k != "skipped_steps"}
        for x, y in zip(before, _net_state(pkg, d, net)):
            np.testing.assert_array_equal(x, y)
    d.close()
