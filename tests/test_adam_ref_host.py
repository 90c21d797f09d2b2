"""tests/adam_ref.py without a GPU: the float64 reference and its bounds accept the C oracle's Solver::ApplyUpdate and a float32 numpy
evaluation of the kernel's own sequence, the comparator rejects every fault tests/test_gpu_optimizer_forms.py relies on it to catch
(each message carries its margin), and every case of that file has a gradient whose blobs are all large enough for the clip-scale
check to see (the C oracle's gradients, same shapes, seeds and inputs)."""
import numpy as np
import pytest

import adam_ref as A
import optimizer_forms_lib as L
from oracle import c_oracle, torch_ref

F32 = np.float32
S, HIDDEN = 59, (256, 128, 64, 64)
KIND_M, KIND_V = c_oracle.KIND_M, c_oracle.KIND_V


def load(rng, net, gnorm, cover=False):
    """tests/test_gpu_optimizer_pass.py's _load: (w, wt, g, m, v) of one net; cover: every blob's share of sum g^2 raised to 1e-3 at least"""
    actor = net == 0
    lay = A.layout(S if actor else S + 10, HIDDEN, actor)
    n = lay.dense
    w = (torch_ref.init_params_np(rng, S, HIDDEN, actor) * 3 + rng.normal(0, 1e-3, n)).astype(F32)
    wt = (w + rng.normal(0, 1e-2, n)).astype(F32)
    g = rng.normal(0, 1, n).astype(F32)
    if cover:
        for _, a, b in lay.blobs:
            share = float((g[a:b].astype(np.float64) ** 2).sum() / (g.astype(np.float64) ** 2).sum())
            if share < 1e-3:
                g[a:b] *= F32(np.sqrt(1e-3 / share))
    g *= F32(gnorm / np.linalg.norm(g.astype(np.float64)))
    g[rng.integers(0, n, n // 50)] = 0.0
    m = rng.normal(0, 1e-3, n).astype(F32)
    v = (rng.uniform(0, 1, n) ** 4 * 1e-4).astype(F32)
    return lay, A.State(w, m, v, wt), g


@pytest.mark.parametrize("net", [0, 1])
@pytest.mark.parametrize("t", [1, 2, 1000])
@pytest.mark.parametrize("gnorm,clip", [(3.0, 10.0), (250.0, 10.0), (250.0, -1.0)])     # clip inactive / active / disabled
def test_reference_accepts_the_oracle(net, t, gnorm, clip):
    rng = np.random.default_rng(100 * net + t + int(gnorm))
    lay, before, g = load(rng, net, gnorm)
    o = c_oracle.Oracle(B=32, S=S, hidden=HIDDEN, capacity=64, clip=clip)
    try:
        assert o.param_count(net) == lay.dense
        o.set_params(net, before.w); o.set_params(net + 2, before.wt)
        o.set_params(net, before.m, KIND_M); o.set_params(net, before.v, KIND_V)
        it = t - 1
        it_a, it_c = (it, it + 5) if net == 0 else (it + 3, it)
        o.set_iters(it_a, it_c)
        o.grad_view(net)[:] = g
        o.apply_update(net)
        after = A.State(o.get_params(net), o.get_params(net, KIND_M), o.get_params(net, KIND_V), o.get_params(net + 2))
    finally:
        o.close()
    hp = A.hyper(1e-5 if net == 0 else 1e-3, clip=clip)
    # (the oracle sums each blob's squares in double and adds the blobs in float: a shorter chain than any the kernel has)
    r = A.check("oracle net %d" % net, hp, lay, before, g, after, t, A.soft_switch(hp, it_a, it_c), A.delta_s(A.depth_arena(lay)))
    assert (r["s_ref"] == 1.0) == (clip < 0 or gnorm <= clip)
    assert r["still"] == 0 and max(r["m"], r["v"], r["step"], r["target"]) <= 1.0


def test_layout_restates_the_arena():
    for fp16 in (False, True):
        lay = A.layout(69, (64, 128), False, fp16)
        kp0 = 128
        assert lay.kp[0] == kp0 and lay.w_off[1] == 64 * kp0 + 64 and lay.dense == 64 * 69 + 64 + 128 * 64 + 128 + 128 + 1
        assert lay.arena == lay.w_off[1] + 128 * 64 + 128 + 128 + 64 and lay.arena % 64 == 0
        assert list(A.dense_of_arena(lay, lay.w_off[1] // 4 - 1)) == [64 * 69 + 60 + i for i in range(4)]      # the last four biases of layer 0
        assert [n for n, _, _ in lay.blobs] == ["W0", "b0", "W1", "b1", "q.W", "q.b"]
    lay = A.layout(54, (64, 128), True)
    assert lay.kp[0] == 64 and lay.hb_off == lay.hw_off + 1280 and lay.blobs[-1][2] == lay.dense
    # the actor's heads: action.W, action.b, actionpara.W, actionpara.b in dense order; one [10][H] matrix and one bias line in the arena
    assert lay.arena_index[lay.blobs[5][1]] == lay.hb_off and lay.arena_index[lay.blobs[6][1]] == lay.hw_off + 4 * 128
    assert lay.arena_index[lay.blobs[7][1]] == lay.hb_off + 4


# ---- planted faults -------------------------------------------------------------------------------------------------------------------------
def _base(net=1, t=2, soft=True, seed=5):
    rng = np.random.default_rng(seed)
    lay, before, g = load(rng, net, 250.0, cover=True)
    hp = A.hyper(1e-5 if net == 0 else 1e-3, clip=10.0, tau=0.25, soft_update_freq=1 if soft else 1000)
    ds = A.delta_s(A.depth_update(lay))
    assert A.uncovered_blobs(lay, g, ds) == []
    return lay, before, g, hp, ds, t


def _unstep(after, before, idx):
    out = A.State(*(x.copy() for x in after))
    for a, b in zip(out, before):
        a[idx] = b[idx]
    return out


def _expect(fault, lay, hp, before, g, after, t, soft, ds, what):
    with pytest.raises(AssertionError, match="margin") as e:
        A.check(fault, hp, lay, before, g, after, t, soft, ds)
    assert what in str(e.value), (fault, str(e.value))
    print("%-40s %s" % (fault, str(e.value).splitlines()[0]))


def test_simulated_kernel_is_accepted():
    for net in (0, 1):
        for soft in (True, False):
            lay, before, g, hp, ds, t = _base(net=net, soft=soft)
            after = A.simulate32(hp, before, g, t, soft, A.scale32(hp, g))
            r = A.check("simulated", hp, lay, before, g, after, t, soft, ds)
            assert r["s_ref"] < 1 and r["still"] == 0 and r["s_err"] < 0.2 * ds
    # a zero gradient on zero history leaves the weight alone, and the comparator counts such elements
    lay, before, g, hp, ds, t = _base()
    g = g.copy(); g[:100] = 0
    before = before._replace(m=before.m.copy(), v=before.v.copy()); before.m[:100] = 0; before.v[:100] = 0
    after = A.simulate32(hp, before, g, t, True, A.scale32(hp, g))
    assert A.check("zeros", hp, lay, before, g, after, t, True, ds)["still"] == 100
    bad = A.State(after.w.copy(), after.m, after.v, after.wt); bad.w[7] = np.nextafter(bad.w[7], F32(np.inf))
    _expect("w moved with g == m == v == 0", lay, hp, before, g, bad, t, True, ds, "g == m == v == 0")


def test_planted_faults_are_rejected():
    lay, before, g, hp, ds, t = _base()
    good = A.simulate32(hp, before, g, t, True, A.scale32(hp, g))
    A.check("good", hp, lay, before, g, good, t, True, ds)
    twice = A.simulate32(hp, good, g, t, True, A.scale32(hp, g))
    # one bias element of the first layer left unstepped (a rider's adam_apply1)
    b0 = lay.blobs[1]
    _expect("first-layer bias unstepped", lay, hp, before, g, _unstep(good, before, [b0[1] + 17]), t, True, ds, "step")
    # the float4 in front of the strided pass's start (skip4 = w_off[1] / 4) unstepped, the first one behind it stepped twice
    last, first = A.dense_of_arena(lay, lay.w_off[1] // 4 - 1), A.dense_of_arena(lay, lay.w_off[1] // 4)
    assert len(last) == 4 and len(first) == 4 and last[-1] + 1 == first[0]
    _expect("float4 skip4 - 1 unstepped", lay, hp, before, g, _unstep(good, before, last), t, True, ds, "step")
    _expect("float4 skip4 stepped twice", lay, hp, before, g, _unstep(good, twice, first), t, True, ds, "step")
    # the last, ragged float4 of the arena that holds parameters (the critic's one head bias)
    ragged = A.dense_of_arena(lay, int(lay.arena_index.max()) // 4)
    assert 1 <= len(ragged) < 4
    _expect("last ragged float4 unstepped", lay, hp, before, g, _unstep(good, before, ragged), t, True, ds, "step")
    # the soft update against its switch
    off = A.simulate32(hp, before, g, t, False, A.scale32(hp, g))
    _expect("target moved, switch off", lay, hp._replace(soft_update_freq=1000), before, g, good, t, False, ds, "while the switch is off")
    _expect("target not moved, switch on", lay, hp, before, g, off, t, True, ds, "target")
    one = A.State(off.w, off.m, off.v, off.wt.copy()); one.wt[5] = good.wt[5]
    _expect("one target element moved, switch off", lay, hp._replace(soft_update_freq=1000), before, g, one, t, False, ds, "while the switch is off")
    # the bias correction of another iteration
    for tt in (1, 2, 1000):
        _expect("t off by one (t = %d)" % tt, lay, hp, before, g, A.simulate32(hp, before, g, tt + 1, True, A.scale32(hp, g)), tt, True, ds, "step")
    # eps inside the square root
    _expect("eps inside the square root", lay, hp, before, g, A.simulate32(hp, before, g, t, True, A.scale32(hp, g), eps_inside_sqrt=True), t, True, ds, "step")
    # the clip scale off by 4 delta_s, either way
    for sign in (1, -1):
        s = F32(np.float64(A.scale32(hp, g)) * (1 + sign * 4 * ds))
        _expect("scale off by %+d x 4 delta_s" % sign, lay, hp, before, g, A.simulate32(hp, before, g, t, True, s), t, True, ds, "applied clip scale")
    # the smallest blob's partial dropped from the norm
    name, share = min(A.blob_shares(lay, g), key=lambda x: x[1])
    a, b = next((a, b) for n, a, b in lay.blobs if n == name)
    assert share >= A.COVER * ds
    _expect("partial of %s (share %.1e) dropped" % (name, share), lay, hp, before, g, A.simulate32(hp, before, g, t, True, A.scale32(hp, g, leave_out=(a, b))), t, True, ds,
            "applied clip scale")
    # ... and the same at the smallest share the coverage condition admits: 50 delta_s moves the scale by 25 delta_s
    s = F32(np.float64(A.scale32(hp, g)) / np.sqrt(1 - A.COVER * ds))
    _expect("a partial worth 50 delta_s dropped", lay, hp, before, g, A.simulate32(hp, before, g, t, True, s), t, True, ds, "applied clip scale")


def test_stale_mirror_is_rejected():
    lay, before, g, hp, ds, t = _base()
    good = A.simulate32(hp, before, g, t, True, A.scale32(hp, g))
    A.check_mirror("mirror", "w16_1", good.w.astype(np.float16).astype(F32), good.w)
    with pytest.raises(AssertionError, match="margin"):
        A.check_mirror("mirror one step stale", "w16_1", before.w.astype(np.float16).astype(F32), good.w)
    with pytest.raises(AssertionError, match="margin"):       # a target mirror that missed one soft update
        A.check_mirror("target mirror one step stale", "w16_3", before.wt.astype(np.float16).astype(F32), good.wt)
    one = good.w.astype(np.float16); one[3] = np.nextafter(one[3], np.float16(np.inf))
    with pytest.raises(AssertionError, match="margin"):
        A.check_mirror("one element one fp16 ulp off", "w16_1", one.astype(F32), good.w)


def test_delta_s_is_what_the_module_derives():
    u = 2.0 ** -24
    lay = A.layout(69, (64, 128), False)
    assert lay.n_part == 2 * 4 + 1 * 2 + max(2, 16) + 1 + 2
    assert A.depth_update(lay) == 28 + 1 + 8 and A.depth_arena(lay) == 4 + 8 + 4 + 8
    assert abs(A.delta_s(37) / (20.5 * u) - 1) < 1e-5
    big = A.layout(69, (1024, 1024, 512), False, True)
    assert A.depth_update(big, "fp16") == 142 + 3 + 8


# ---- the coverage condition of every GPU case, on the C oracle's gradients -------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in L.CASES])
def test_every_blob_of_every_gpu_case_is_covered(name):
    case = L.CASE_BY_NAME[name]
    inp = L.make_inputs(case)
    fp16 = case.precision == "fp16"
    lays = {0: A.layout(case.S, case.hidden, True, fp16), 1: A.layout(case.S + L.NO, case.hidden, False, fp16)}
    hp = {0: A.hyper(1e-5, clip=case.clip), 1: A.hyper(1e-3, clip=case.clip)}
    o = c_oracle.Oracle(B=case.B, S=case.S, hidden=case.hidden, capacity=2 * L.REPLAY, clip=case.clip, soft_update_freq=case.freq, tau=case.tau)
    try:
        for net in range(4):
            o.set_params(net, inp["w"][net])
        o.add_transitions(inp["s"], inp["a"], inp["r"], inp["mc"], inp["nx"], inp["term"])
        for row in inp["warm"]:
            o.update(row)
        for u, row in enumerate(inp["idx"]):
            g = {}
            o.update_phase(0, row); g[1] = o.grad_view(1).copy()
            o.update_phase(1, row); g[0] = o.grad_view(0).copy()
            o.update_phase(2, row)
            for net in (0, 1):
                # the larger of the two derived bounds a case of this shape can meet (partials inside the update; the arena under data parallelism)
                ds = max(A.delta_s(A.depth_update(lays[net], case.precision)), A.delta_s(A.depth_arena(lays[net])))
                s_ref, nrm = A.clip_scale(hp[net], g[net])
                shares = A.blob_shares(lays[net], g[net])
                print("%s[%d] net %d: ||g|| %.3e s_ref %.3e, smallest share %s, needs %.2e" % (name, u, net, nrm, s_ref, min(shares, key=lambda x: x[1]), A.COVER * ds))
                if 0 <= case.clip < 1e3:
                    assert s_ref < 1.0, (name, u, net, nrm)
                    assert A.uncovered_blobs(lays[net], g[net], ds) == [], (name, u, net, A.COVER * ds)
                else:
                    assert s_ref == 1.0
    finally:
        o.close()
