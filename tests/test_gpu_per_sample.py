"""Prioritized replay: the stratified sampler (k_per_sample) against tests/per_ref.py — the same Philox draw, the same float32 u_j, the
same Hillis-Steele descent on the tree read back, so slots, indices and probabilities agree exactly.  Priorities are set through
dqnhip_per_set_priorities.  No reference counterpart (the reference samples uniformly, src/dqn.cpp:501-509)."""
import numpy as np
import pytest

import per_ref as R
from synth import synth_replay

pytestmark = pytest.mark.gpu

CAP, B, S, HID = 5000, 32, 58, (64, 64)
SEED = 77
F = np.float32


def _make(pkg, n_fill, seed=SEED, wrap=False, **kw):
    rng = np.random.default_rng(4)
    d = pkg.DQN(S, minibatch=B, hidden=HID, memory=CAP, seed=3, **kw)
    d.enable_prioritized_replay(seed=seed, alpha=0.6, beta0=0.4)
    head = 0
    if wrap:      # 4000 + 3000: AddTransitions pops 4000 + 3000 - 5000 + 1 = 2001, the window becomes [2001, 2001 + 4999) and wraps
        d.add_transitions_arrays(*synth_replay(rng, 4000, S, mean_len=10))
        d.add_transitions_arrays(*synth_replay(rng, 3000, S, mean_len=10))
        head, n_fill = 2001, 4999
    else:
        d.add_transitions_arrays(*synth_replay(rng, n_fill, S, mean_len=10))
    assert d.memory_size() == n_fill
    return d, head, n_fill


def _levels(d):
    return [d.per_debug_read("level%d" % k) for k in range(4)]


CASES = {"ramp": lambda n: np.arange(1, n + 1, dtype=F),
         "spike": lambda n: np.where(np.arange(n) == n // 3, F(1000), F(0.01)).astype(F)}


@pytest.mark.parametrize("case", ["ramp", "spike", "wrap"])
def test_sampler_is_the_reference_exactly(pkg, gpu, case):
    d, head, size = _make(pkg, 3000, wrap=case == "wrap")
    pr = CASES["ramp" if case == "wrap" else case](size)
    d.set_per_priorities(0, pr)
    lv = _levels(d)
    R.check_tree(lv)
    R.check_window(lv[0], head, size, lv[-1][0])
    assert np.array_equal(d.per_priorities(0, size), pr) and np.array_equal(lv[0][(head + np.arange(size)) % CAP], pr)
    st = d.per_state()
    assert st["p_max"] == max(1.0, pr.max()) and st["total"] == lv[-1][0]
    ctr = st["next_counter"]
    # the sampler alone, three minibatches ...
    idx3, prob3 = d.per_sample(ctr, 3)
    for k in range(3):
        idx, slot, prob, u = R.sample(lv, SEED, ctr + k, B, head, CAP)
        assert np.array_equal(idx3[k], idx), (case, k)
        assert np.array_equal(prob3[k].view(np.uint32), prob.view(np.uint32)), (case, k)
    # ... and inside an update: u, slot, idx, prob of the update equal the reference's on the tree as it was
    idx, slot, prob, u = R.sample(lv, SEED, ctr, B, head, CAP)
    d.UpdateActorCritic()
    assert np.array_equal(d.per_debug_read("u").view(np.uint32), u.view(np.uint32)), case
    assert np.array_equal(d.per_debug_read("slot"), slot), case
    assert np.array_equal(d.debug_read("idx").astype(np.int64), idx), case
    assert np.array_equal(d.per_debug_read("prob").view(np.uint32), prob.view(np.uint32)), case
    R.check_sample(lv, slot, prob)
    # every u_j lies in its stratum [j, j + 1) / B x total (float32 products: within an ulp of the edges)
    total = float(lv[-1][0])
    lo, hi = np.arange(B) / B * total, (np.arange(B) + 1) / B * total
    assert (u >= lo * (1 - 2e-7)).all() and (u <= hi * (1 + 2e-7)).all()
    if case == "spike":
        assert (slot == (head + size // 3) % CAP).sum() >= B // 2      # p / total = 1000 / 1030
    assert d.per_state()["next_counter"] == ctr + 1
    d.close()


def test_prediction_and_seeds(pkg, gpu):
    """dqnhip_per_sample(next_counter, 1) is what the next update draws; one seed draws identically, another differently"""
    a, _, size = _make(pkg, 2000)
    b, _, _ = _make(pkg, 2000)
    c, _, _ = _make(pkg, 2000, seed=SEED + 1)
    pr = np.random.default_rng(8).uniform(0.01, 3.0, size).astype(F)
    for d in (a, b, c):
        d.set_per_priorities(0, pr)
    for it in range(3):
        ctr = a.per_state()["next_counter"]
        want, _ = a.per_sample(ctr, 1)
        a.UpdateActorCritic()
        assert np.array_equal(a.debug_read("idx").astype(np.int32), want[0]), it
        b.UpdateActorCritic()
        assert np.array_equal(b.debug_read("idx"), a.debug_read("idx")), it
        assert np.array_equal(b.per_debug_read("level0"), a.per_debug_read("level0")), it
    ia, _ = a.per_sample(7, 2)
    ic, _ = c.per_sample(7, 2)
    assert not np.array_equal(ia, ic)
    for d in (a, b, c):
        d.close()


def test_frequencies(pkg, gpu):
    """200 sample-only minibatches over 64 live slots with priorities 1 .. 64: |count - expected| <= 5 sqrt(expected) per slot
    (stratification only narrows the spread; tests/test_per_ref_host.py checks that the reference alone meets this for this seed)"""
    d, head, size = _make(pkg, 64)
    d.set_per_priorities(0, np.arange(1, 65, dtype=F))
    idx, prob = d.per_sample(0, 200)
    assert idx.min() >= 0 and idx.max() < 64
    count = np.bincount(idx.ravel(), minlength=64)
    expected = 200 * B * np.arange(1, 65) / (64 * 65 / 2)
    print("largest |count - expected| / sqrt(expected):", (np.abs(count - expected) / np.sqrt(expected)).max())
    assert (np.abs(count - expected) <= 5 * np.sqrt(expected)).all(), (count, expected)
    assert np.array_equal(prob.ravel(), (np.arange(1, 65, dtype=F) / F(2080))[idx.ravel()])
    d.close()


def test_argument_checks(pkg, gpu):
    d, _, size = _make(pkg, 100)
    with pytest.raises(pkg.DQNFatal, match="outside"):
        d.set_per_priorities(90, np.ones(11, F))
    with pytest.raises(pkg.DQNFatal, match="not finite and >= 0"):
        d.set_per_priorities(0, np.array([1.0, -1.0], F))
    with pytest.raises(pkg.DQNFatal, match="not finite and >= 0"):
        d.set_per_priorities(0, np.array([np.inf], F))
    with pytest.raises(pkg.DQNFatal, match="unknown buffer"):
        d.per_debug_read("nonesuch")
    plain = pkg.DQN(S, minibatch=B, hidden=HID, memory=CAP, seed=3)
    assert plain.per_state()["enabled"] == 0
    with pytest.raises(pkg.DQNFatal, match="not enabled"):
        plain.per_sample(0, 1)
    plain.close(); d.close()
