"""tests/per_ref.py, the numpy restatement the prioritized-replay GPU tests compare against, checked on its own without a GPU:
(a) its float32 tree descent agrees with a brute-force float64 inverse-CDF sampler on every draw that is not within float32 rounding
    of a leaf boundary (and the share of draws excused on that ground stays below 1 %),
(b) its draws reproduce p / total in frequency,
(c) its check_* functions reject the faults they exist for.
And the entry points that need no device: dqnhip_per_default_config, dqnhip_per_enable's argument checks."""
import ctypes as C

import numpy as np
import pytest

import per_ref as R

F = np.float32


LIVE = 1000      # live slots of the 5000: a window that wraps, [4500, 5000) + [0, 500)


def _priorities(rng, cap, kind):
    if kind == "ramp":
        v = np.arange(1, LIVE + 1, dtype=F)
    elif kind == "lognormal":
        v = rng.lognormal(0.0, 1.5, LIVE).astype(F)
    else:
        v = np.full(LIVE, 1.0, F)     # a spike among ones, and a zero gap
        v[LIVE // 3] = 500.0
        v[LIVE // 2:LIVE // 2 + 70] = 0.0
    p = np.zeros(cap, F)
    p[(4500 + np.arange(LIVE)) % cap] = v
    return p


@pytest.mark.parametrize("kind", ["ramp", "lognormal", "spike"])
def test_descent_agrees_with_float64_inverse_cdf(kind):
    rng = np.random.default_rng(3)
    cap, B = 5000, 64
    leaves = _priorities(rng, cap, kind)
    levels = R.build_levels(leaves)
    total32 = levels[-1][0]
    cdf = np.cumsum(leaves.astype(np.float64))
    assert abs(float(total32) - cdf[-1]) <= 1e-5 * cdf[-1]
    # float32 rounding of a position in [0, total): per level six additions of the scan, six of a node's sum and one subtraction, each
    # within half an ulp of a value <= total -> 3 x 13 x 0.5 = 19.5 ulp(total) at three levels; 32 taken.  A draw is excused when it
    # lies that close to a boundary between two leaves: with LIVE boundaries a share of about 2 x 32 x 2^-24 x LIVE = 0.4 %
    slack = 32 * float(np.spacing(total32))
    excused = draws = 0
    for ctr in range(40):
        idx, slot, prob, u = R.sample(levels, 0xABCDEF, ctr, B, head=0, cap=cap)
        R.check_sample(levels, slot, prob)
        # u carries total32's scale: map onto the float64 CDF's
        pos = u.astype(np.float64) * (cdf[-1] / float(total32))
        brute = np.searchsorted(cdf, pos, side="right")
        for j in range(B):
            draws += 1
            lo = cdf[brute[j] - 1] if brute[j] > 0 else 0.0
            near = min(pos[j] - lo, cdf[min(brute[j], cap - 1)] - pos[j]) <= slack
            if near:
                excused += 1
                continue
            assert slot[j] == brute[j], (kind, ctr, j, slot[j], brute[j], u[j])
        # every u_j lies in its stratum
        edges = np.arange(B + 1, dtype=np.float64) / B * float(total32)
        assert (u >= edges[:-1] * (1 - 1e-6)).all() and (u <= edges[1:] * (1 + 1e-6)).all()
    assert excused < 0.01 * draws, (kind, excused, draws)


def test_frequencies_follow_the_priorities():
    """64 live slots with priorities 1 .. 64, 200 minibatches of 32: |count - expected| <= 5 sqrt(expected) per slot (stratification only
    narrows the spread) — the bound and the seed tests/test_gpu_per_sample.py uses on the device"""
    cap, B, n = 5000, 32, 200
    leaves = np.zeros(cap, F)
    leaves[:64] = np.arange(1, 65, dtype=F)
    levels = R.build_levels(leaves)
    count = np.zeros(cap, np.int64)
    for ctr in range(n):
        _, slot, _, _ = R.sample(levels, 77, ctr, B, 0, cap)
        np.add.at(count, slot, 1)
    assert count[64:].sum() == 0
    expected = n * B * leaves[:64].astype(np.float64) / leaves.sum(dtype=np.float64)
    assert (np.abs(count[:64] - expected) <= 5 * np.sqrt(expected)).all(), (count[:64], expected)


def test_sync_restated():
    cap = 300
    leaves = np.zeros(cap, F)
    leaves = R.sync_leaves(leaves, (0, 0), (0, 250), 1.0)
    assert (leaves[:250] == 1).all() and (leaves[250:] == 0).all()
    leaves[10:20] = 3.0
    # 120 appended into a window of 250: AddTransitions pops 250 + 120 - 300 + 1 = 71
    leaves2 = R.sync_leaves(leaves, (0, 250), (71, 299), 3.0)
    R.check_window(leaves2, 71, 299, R.build_levels(leaves2)[-1][0])
    R.check_fresh(leaves2, 71, 299 - 120, 120, 3.0)
    assert (leaves2[71:250] == leaves[71:250]).all() and (leaves2[:70] == 3.0).all() and leaves2[70] == 0


def test_checks_reject_what_they_exist_for():
    rng = np.random.default_rng(5)
    cap = 5000
    leaves = np.zeros(cap, F)
    head, size = 4000, 3000                                   # a window that wraps
    live = (head + np.arange(size)) % cap
    leaves[live] = rng.uniform(0.1, 2.0, size).astype(F)
    levels = R.build_levels(leaves)
    R.check_tree(levels)
    R.check_window(leaves, head, size, levels[-1][0])
    # a stale parent node
    stale = [l.copy() for l in levels]
    stale[1][7] = np.nextafter(stale[1][7], F(np.inf))
    with pytest.raises(AssertionError, match="level 1"):
        R.check_tree(stale)
    stale = [l.copy() for l in levels]
    stale[0][live[5]] *= F(2)                                  # a leaf changed, nothing above recomputed
    with pytest.raises(AssertionError, match="level 1"):
        R.check_tree(stale)
    # a non-zero leaf outside the window
    bad = leaves.copy()
    bad[(head + size + 3) % cap] = 0.5
    with pytest.raises(AssertionError, match="outside the window"):
        R.check_window(bad, head, size, levels[-1][0])
    with pytest.raises(AssertionError):
        R.check_window(np.zeros(cap, F), 0, 10, F(0))          # total > 0 iff size > 0
    # a leaf not reset after the slot was refilled
    fresh = R.sync_leaves(leaves, (head, size), ((head + 100) % cap, size), 2.5)
    R.check_fresh(fresh, (head + 100) % cap, size - 100, 100, 2.5)
    fresh[(head + 100 + size - 1) % cap] = 0.7
    with pytest.raises(AssertionError, match="refilled"):
        R.check_fresh(fresh, (head + 100) % cap, size - 100, 100, 2.5)
    # a weight with the wrong exponent sign
    prob = rng.uniform(1e-4, 1e-2, 32).astype(F)
    w = R.weights(prob, 0.7).astype(F)
    assert R.check_weights(w, prob, 0.7, 1) <= 1 and w.max() == 1.0
    with pytest.raises(AssertionError, match="weight"):
        R.check_weights(((prob.astype(np.float64) / prob.min()) ** 0.7).astype(F), prob, 0.7, 16)
    # a write-back that skipped eps
    td = np.abs(rng.normal(0, 1e-3, 32)).astype(F)
    td[3] = 0.0
    R.check_write_back(R.write_back(td, 1e-6, 0.6).astype(F), td, 1e-6, 0.6, 1)
    with pytest.raises(AssertionError, match="leaf"):
        R.check_write_back((td.astype(np.float64) ** 0.6).astype(F), td, 1e-6, 0.6, 16)
    # a sampled zero-priority slot
    idx, slot, prob, u = R.sample(levels, 9, 0, 32, head, cap)
    R.check_sample(levels, slot, prob)
    slot[4] = (head + size + 1) % cap
    with pytest.raises(AssertionError, match="priority is zero"):
        R.check_sample(levels, slot, prob)


def test_philox_matches_the_oracle():
    """the restated generator is the library's: oracle/c_oracle.philox_indices reproduces the uniform sampler's indices from it"""
    from oracle import c_oracle
    size, B = 1000, 32
    want = c_oracle.philox_indices(3, 5, B, size)
    got = (R.philox_u32(3, 5, np.arange(B)).astype(np.uint64) * np.uint64(size)) >> np.uint64(32)
    assert np.array_equal(np.asarray(want, np.int64), got.astype(np.int64))


def test_enable_argument_checks(pkg):
    """no device needed: the defaults (the paper's customary values), a null handle, a config of another size"""
    lib = pkg.capi.load()
    c = pkg.capi.PerConfig()
    lib.dqnhip_per_default_config(C.byref(c))
    assert c.struct_size == C.sizeof(pkg.capi.PerConfig)
    assert (round(c.alpha, 6), round(c.beta0, 6), c.beta_anneal_iters, round(c.eps, 12)) == (0.6, 0.4, 0, 1e-6)
    assert lib.dqnhip_per_enable(None, C.byref(c)) != 0
    assert b"dqnhip_per_enable: null handle" in lib.dqnhip_last_error()
    c.struct_size += 4
    assert lib.dqnhip_per_enable(None, C.byref(c)) != 0
    assert b"dqnhip_per_config.struct_size" in lib.dqnhip_last_error()
    assert lib.dqnhip_per_enable(None, None) != 0
    assert b"null config" in lib.dqnhip_last_error()
    s = pkg.capi.PerState()
    s.struct_size = C.sizeof(pkg.capi.PerState)
    assert lib.dqnhip_per_get_state(None, C.byref(s)) != 0
    assert lib.dqnhip_per_sample(None, 0, 1, None, None) != 0
    assert b"dqnhip_per_sample: null handle" in lib.dqnhip_last_error()
