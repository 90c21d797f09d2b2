"""N-step returns: what k_gather_n leaves behind every sampled index — the window's length, discounted reward sum, discount, the
bootstrap row's terminal flag and next state — against tests/nstep_ref.py, bit for bit; the target k_head_q_train_n forms from it;
and dqnhip_nstep_validate's contiguity check.  No reference counterpart (the reference's target is one step, src/dqn.cpp:892-900)."""
import numpy as np
import pytest

import nstep_ref as R
from synth import det_indices, synth_replay

pytestmark = pytest.mark.gpu

B, S, HID, CAP, N = 32, 58, (64, 64), 4096, 2048
F = np.float32
GAMMA, BETA = 0.99, 0.5          # the learner's defaults


def _replay(S=S, n=N, seed=5):
    return synth_replay(np.random.default_rng(seed), n, S, mean_len=10)


def _make(pkg, replay, n_step, S=S, cap=CAP):
    d = pkg.DQN(S, minibatch=B, hidden=HID, memory=cap, seed=3)
    d.add_transitions_arrays(*replay)
    if n_step is not None:
        d.enable_n_step(n_step)
    return d


def _check_update(d, memory, idx, n):
    """one update on idx; memory: the ring's content in logical order (s, a, r, mc, nx, term)"""
    s, a, r, mc, nx, term = memory
    idx = np.asarray(idx, np.int64)
    d.UpdateActorCritic(idx)
    want = R.gather(r, term, idx, n, GAMMA)
    steps, rew, disc = d.n_step_debug_read("steps"), d.n_step_debug_read("reward"), d.n_step_debug_read("disc")
    print("n", n, "steps", np.bincount(steps, minlength=n + 1)[1:], "R", rew.min(), rew.max())
    assert np.array_equal(steps, want["steps"]), (n, steps, want["steps"])
    assert np.array_equal(rew.view(np.uint32), want["reward"].view(np.uint32)), (n, rew, want["reward"])
    assert np.array_equal(disc.view(np.uint64), want["disc"].view(np.uint64)), (n, disc, want["disc"])
    assert np.array_equal(d.debug_read("terminal"), want["terminal"])
    assert np.array_equal(d.debug_read("idx").astype(np.int64), idx)
    # the target: the 1-step expressions with disc in gamma's place and R in r's, on the q' the device formed
    y = R.target(rew, disc, d.debug_read("q_target"), want["terminal"], mc[idx], BETA)
    assert np.array_equal(d.debug_read("y").view(np.uint32), y.view(np.uint32))
    return want


@pytest.fixture(scope="module")
def replay():
    return _replay()


@pytest.mark.parametrize("n", [1, 3, 16, 64])
def test_window_reward_discount_and_target(pkg, gpu, replay, n):
    d = _make(pkg, replay, n)
    assert d.n_step() == n
    idx = det_indices(17, 1, B, N)[0]
    idx[:3] = (N - 1, N - 2, 0)                  # the memory's last transitions and its first
    want = _check_update(d, replay, idx, n)
    assert want["steps"].max() <= n and (n == 1 or want["steps"].max() > 1)
    # a second n on the same learner, and back
    d.enable_n_step(2)
    _check_update(d, replay, idx, 2)
    d.enable_n_step(n)
    _check_update(d, replay, idx[::-1].copy(), n)
    d.close()


def test_state_size_59(pkg, gpu):
    rp = _replay(S=59)
    d = _make(pkg, rp, 3, S=59)
    _check_update(d, rp, det_indices(19, 1, B, N)[0], 3)
    d.close()


@pytest.mark.parametrize("n", [3, 16])
def test_windows_cross_the_rings_physical_end(pkg, gpu, n):
    """capacity 256, 400 transitions in two appends of 200: the second evicts 145, the window starts at physical slot 145 and logical
    110 is the last slot before the wrap"""
    cap = 256
    rp = _replay(n=400, seed=6)
    d = pkg.DQN(S, minibatch=B, hidden=HID, memory=cap, seed=3)
    d.add_transitions_arrays(*[x[:200] for x in rp])
    d.add_transitions_arrays(*[x[200:] for x in rp])
    size = d.memory_size()
    assert size == 255
    mem = d.read_memory(0, size)
    for got, all_ in zip(mem, rp):
        assert np.array_equal(got, all_[400 - size:])
    d.enable_n_step(n)
    wrap = cap - 145 - 1                         # the logical index in the ring's last physical slot
    idx = np.concatenate([np.arange(wrap - 19, wrap + 5), np.array([0, 1, size - 1, size - 2, size - n, size - n - 1, 128, 200])]).astype(np.int64)
    assert len(idx) == B
    want = _check_update(d, mem, idx, n)
    crossing = (idx <= wrap) & (idx + want["steps"] - 1 > wrap)
    assert crossing.sum() >= 2, "no window of this case crosses the physical end"
    assert d.validate_memory() == (0, -1)
    d.close()


@pytest.mark.parametrize("n", [3, 16, 64])
def test_a_non_terminal_tail_ends_the_window(pkg, gpu, n):
    rp = [x.copy() for x in _replay(seed=8)]
    rp[5][-1] = 0                                # the memory ends inside an episode
    rp[4][-1] = np.random.default_rng(1).uniform(-1, 1, S).astype(F)
    last_term = int(np.nonzero(rp[5])[0][-1])
    d = _make(pkg, rp, n)
    idx = det_indices(23, 1, B, N)[0]
    idx[:6] = (N - 1, N - 2, N - n, N - n - 1, last_term + 1, last_term)
    want = _check_update(d, rp, idx, n)
    assert want["steps"][0] == 1 and want["terminal"][0] == 0 and want["steps"][1] == min(2, n)
    d.close()


def test_the_bootstrap_state_is_the_windows_last(pkg, gpu, replay):
    """q' of an n = 3 learner equals that of an n = 1 learner exactly on the rows whose window is one step long: every other row's
    critic-target input is another transition's next state"""
    one, three = _make(pkg, replay, 1), _make(pkg, replay, 3)
    idx = det_indices(29, 1, B, N)[0]
    one.UpdateActorCritic(idx); three.UpdateActorCritic(idx)
    m = three.n_step_debug_read("steps")
    q1, q3 = one.debug_read("q_target").view(np.uint32), three.debug_read("q_target").view(np.uint32)
    assert (m == 1).sum() >= 2 and (m > 1).sum() >= 2, m
    assert np.array_equal(q1[m == 1], q3[m == 1])
    assert (q1[m > 1] != q3[m > 1]).all()
    # the online critic's input is li's state and action either way
    assert np.array_equal(one.debug_read("q_train").view(np.uint32), three.debug_read("q_train").view(np.uint32))
    one.close(); three.close()


def test_validate_memory(pkg, gpu, replay):
    d = _make(pkg, replay, None)                 # any learner may validate
    assert d.n_step() == 0
    assert d.validate_memory() == (0, -1) and d.validate_memory(100, 500) == (0, -1) and d.validate_memory(N, 0) == (0, -1)
    with pytest.raises(pkg.DQNFatal, match="outside the memory"):
        d.validate_memory(0, N + 1)
    d.close()
    # one stored next state that is not its successor's state: a second memory with a perturbed nx
    term = replay[5]
    free = np.nonzero(term[:-1] == 0)[0]
    k, k2 = int(free[len(free) // 2]), int(free[len(free) // 4])
    rp = [x.copy() for x in replay]
    rp[4][k, S - 1] = np.nextafter(rp[4][k, S - 1], F(2))          # one ulp, the last float of the row
    d = _make(pkg, rp, 3)
    assert d.validate_memory() == (1, k)
    assert d.validate_memory(k, 1) == (1, k) and d.validate_memory(0, k) == (0, -1) and d.validate_memory(k + 1) == (0, -1)
    d.close()
    rp[4][k2, 0] = -rp[4][k2, 0] if rp[4][k2, 0] != 0 else F(1)
    d = _make(pkg, rp, None)
    assert d.validate_memory() == (2, k2) and d.validate_memory(k2 + 1) == (1, k)
    d.close()
    # the memory's last transition is exempt, terminal or not
    rp = [x.copy() for x in replay]
    rp[5][-1] = 0
    rp[4][-1] = 7.0
    d = _make(pkg, rp, None)
    assert d.validate_memory() == (0, -1)
    d.close()
