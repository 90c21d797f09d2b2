"""tests/nstep_ref.py against answers worked out by hand, and the n-step entry points' argument checks — no GPU."""
import ctypes as C

import numpy as np

import nstep_ref as R

F, F64 = np.float32, np.float64
G = 0.5          # a discount whose powers and products are exact: the hand answers below are exact too

# three episodes: [0, 1, 2], [3, 4], [5, 6, 7, 8 ...] — the last one has no terminal transition (the memory ends inside it)
REW = np.array([1, 2, 4, 8, 16, 32, 64, 128, 256], F)
TERM = np.array([0, 0, 1, 0, 1, 0, 0, 0, 0], np.uint8)


def _g(idx, n, gamma=G):
    return R.gather(REW, TERM, np.asarray(idx), n, gamma)


def test_n_1_is_the_one_step_transition():
    g = _g(np.arange(9), 1)
    assert np.array_equal(g["steps"], np.ones(9, np.int64)) and np.array_equal(g["b"], np.arange(9))
    assert np.array_equal(g["reward"].view(np.uint32), REW.view(np.uint32))
    assert np.array_equal(g["disc"], np.full(9, G)) and np.array_equal(g["terminal"], TERM.astype(F))
    # any gamma: R is r exactly and disc is gamma exactly
    g = _g(np.arange(9), 1, 0.99)
    assert np.array_equal(g["reward"].view(np.uint32), REW.view(np.uint32)) and (g["disc"] == F64(0.99)).all()


def test_terminal_at_step_2_of_3():
    g = _g([1, 3], 3)
    # from 1: r1 + g r2 = 2 + 2, stops at the terminal transition 2; from 3: 8 + 8, stops at 4
    assert list(g["steps"]) == [2, 2] and list(g["b"]) == [2, 4]
    assert list(g["reward"]) == [4.0, 16.0] and list(g["disc"]) == [0.25, 0.25] and list(g["terminal"]) == [1.0, 1.0]
    # a window that starts on a terminal transition is that transition
    g = _g([2], 3)
    assert (g["steps"][0], g["reward"][0], g["disc"][0], g["terminal"][0]) == (1, 4.0, 0.5, 1.0)
    # a full window inside an episode: 1 + 1 + 1 = 3 with the bootstrap row the terminal one
    g = _g([0], 3)
    assert (g["steps"][0], g["b"][0], g["reward"][0], g["disc"][0], g["terminal"][0]) == (3, 2, 3.0, 0.125, 1.0)


def test_non_terminal_tail():
    """the memory's last transition ends a window: never a read beyond it, and the bootstrap row is non-terminal"""
    g = _g([8, 7, 6, 5], 3)
    assert list(g["steps"]) == [1, 2, 3, 3] and list(g["b"]) == [8, 8, 8, 7]
    assert list(g["reward"]) == [256.0, 128.0 + 128.0, 64.0 + 64.0 + 64.0, 32.0 + 32.0 + 32.0]
    assert list(g["disc"]) == [0.5, 0.25, 0.125, 0.125] and list(g["terminal"]) == [0.0, 0.0, 0.0, 0.0]


def test_n_larger_than_every_episode():
    g = _g(np.arange(9), 64)
    assert list(g["steps"]) == [3, 2, 1, 2, 1, 4, 3, 2, 1]
    assert list(g["b"]) == [2, 2, 2, 4, 4, 8, 8, 8, 8]
    assert list(g["reward"]) == [3.0, 4.0, 4.0, 16.0, 16.0, 128.0, 192.0, 256.0, 256.0]
    assert list(g["disc"]) == [0.125, 0.25, 0.5, 0.25, 0.5, 0.0625, 0.125, 0.25, 0.5]


def test_the_reward_sum_rounds_as_stated():
    """Horner from the back in float64, one product and one sum rounded per step, float32 once at the end"""
    r = np.array([0.1, -0.07, 0.03, 5.02], F)
    term = np.array([0, 0, 0, 1], np.uint8)
    gamma = 0.99
    acc = F64(r[3])
    acc = F64(F64(r[2]) + F64(gamma * acc)); acc = F64(F64(r[1]) + F64(gamma * acc)); acc = F64(F64(r[0]) + F64(gamma * acc))
    g = R.gather(r, term, [0], 4, gamma)
    assert g["reward"][0] == F(acc) and g["disc"][0] == ((F64(gamma) * gamma) * gamma) * gamma and g["steps"][0] == 4


def test_relabel_and_target():
    rng = np.random.default_rng(1)
    n = len(REW)
    s = rng.uniform(-1, 1, (n, 5)).astype(F); a = rng.uniform(-1, 1, (n, 10)).astype(F)
    nx = np.vstack([s[1:], rng.uniform(-1, 1, (1, 5)).astype(F)]); nx[TERM.astype(bool)] = 0
    mc = rng.uniform(-1, 1, n).astype(F)
    s2, a2, r2, mc2, nx2, t2 = R.relabel((s, a, REW, mc, nx, TERM), 3, G)
    g = _g(np.arange(n), 3)
    assert np.array_equal(s2, s) and np.array_equal(a2, a) and np.array_equal(mc2, mc)
    assert np.array_equal(r2, g["reward"]) and np.array_equal(t2, g["terminal"].astype(np.uint8)) and np.array_equal(nx2, nx[g["b"]])
    assert np.array_equal(nx2[0], nx[2]) and np.array_equal(nx2[5], nx[7]) and t2[0] == 1 and t2[5] == 0
    # the target on exact values: beta = 0.5, q' = 8
    y = R.target(g["reward"], g["disc"], np.full(n, 8, F), g["terminal"], np.full(n, 2, F), 0.5)
    assert y[0] == 0.5 * 2 + 0.5 * 3.0                        # terminal window: R alone
    assert y[5] == 0.5 * 2 + 0.5 * (96.0 + 0.125 * 8)         # 32 + 32 + 32, three steps, non-terminal
    assert y[8] == 0.5 * 2 + 0.5 * (256.0 + 0.5 * 8)


def test_argument_checks_on_a_null_handle(pkg):
    lib = pkg.capi.load()
    for name in ("dqnhip_nstep_enable", "dqnhip_nstep_get", "dqnhip_nstep_debug_read", "dqnhip_nstep_debug_read_f64", "dqnhip_nstep_validate"):
        assert hasattr(lib, name), name
    assert pkg.capi.NSTEP_MAX == R.NSTEP_MAX == 64 and "n_step" in pkg.capi.PLAN_FORMS and pkg.capi.PLAN_FORMS.index("n_step") == 14
    assert lib.dqnhip_nstep_enable(None, 3) != 0
    assert b"dqnhip_nstep_enable: null handle" in lib.dqnhip_last_error() and b"n-step returns" in lib.dqnhip_last_error()
    n = C.c_int32(7)
    assert lib.dqnhip_nstep_get(None, C.byref(n)) != 0 and b"dqnhip_nstep_get: null argument" in lib.dqnhip_last_error()
    v, fb = C.c_int64(), C.c_int32()
    assert lib.dqnhip_nstep_validate(None, 0, 1, C.byref(v), C.byref(fb)) != 0
    assert b"dqnhip_nstep_validate: null handle" in lib.dqnhip_last_error()
    buf = (C.c_float * 4)()
    assert lib.dqnhip_nstep_debug_read(None, b"reward", buf, 4) != 0 and b"null argument" in lib.dqnhip_last_error()
    for m in ("enable_n_step", "n_step", "n_step_debug_read", "validate_memory"):
        assert callable(getattr(pkg.DQN, m)), m
