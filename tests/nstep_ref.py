"""N-step returns restated in numpy from the semantics of include/dqnhip.h (dqnhip_nstep_enable), and nothing else.

For a sampled logical index li, ring size `size`, discount gamma (a float64) and n in 1 .. 64:
    m     the smallest k in 1 .. n with term[li + k - 1] != 0, or li + k - 1 == size - 1, or k == n
    R     acc = r[li + m - 1]; for k = m - 2 .. 0: acc = float64(r[li + k]) + gamma * acc; R = float32(acc)   (two roundings per step)
    disc  d = gamma, then m - 1 times d = d * gamma
    b     li + m - 1: next state and terminal flag are b's; state, action, mc and idx are li's
    off   term ? R : float32(float64(R) + disc * float64(q'))        then the beta mix of the 1-step update
Every array is in LOGICAL order (index 0 = the oldest transition of the memory)."""
from fractions import Fraction

import numpy as np

F = np.float32
F64 = np.float64
NSTEP_MAX = 64


def window(term, size, li, n):
    """m of the window that starts at li"""
    for k in range(1, n + 1):
        if term[li + k - 1] != 0 or li + k - 1 == size - 1 or k == n:
            return k
    raise AssertionError("unreachable: k == n ends every window")


def discount(gamma, m):
    d = F64(gamma)
    for _ in range(m - 1):
        d = F64(d * F64(gamma))
    return d


def reward_sum(r, li, m, gamma):
    acc = F64(r[li + m - 1])
    for k in range(m - 2, -1, -1):
        acc = F64(F64(r[li + k]) + F64(F64(gamma) * acc))
    return F(acc)


def gather(r, term, idx, n, gamma):
    """-> dict of [len(idx)] arrays: steps (int64), reward (float32), disc (float64), b (int64), terminal (float32: 0 / 1)"""
    assert 1 <= n <= NSTEP_MAX
    r, term, idx = np.asarray(r, F), np.asarray(term), np.asarray(idx, np.int64)
    size = len(r)
    m = np.array([window(term, size, int(li), n) for li in idx], np.int64)
    b = idx + m - 1
    return {"steps": m, "b": b,
            "reward": np.array([reward_sum(r, int(li), int(k), gamma) for li, k in zip(idx, m)], F),
            "disc": np.array([discount(gamma, int(k)) for k in m], F64),
            "terminal": (term[b] != 0).astype(F)}


def relabel(replay, n, gamma):
    """the 1-step replay (s_i, a_i, R_i, mc_i, next[b_i], term[b_i]) an n-step learner sees behind every index"""
    s, a, r, mc, nx, term = replay
    g = gather(r, term, np.arange(len(r)), n, gamma)
    return s.copy(), a.copy(), g["reward"], np.asarray(mc, F).copy(), np.asarray(nx, F)[g["b"]].copy(), np.asarray(term)[g["b"]].astype(np.uint8)


def _fma64(a, b, c):
    """float64(a * b + c) with one rounding: the update's head kernel forms the double products and sums fused (finite inputs)"""
    return F64(float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))))


def target(R, disc, q_target, terminal, mc, beta):
    """y of each row, float32: off = term ? R : float32(R + disc q'), y = float32(beta mc + (1 - beta) off) — the 1-step update's
    expressions (src/dqn.cpp:892-900 of the reference) with disc in gamma's place and R in r's, the double multiply-adds fused"""
    out = np.empty(len(R), F)
    for i in range(len(R)):
        off = F(R[i]) if terminal[i] != 0 else F(_fma64(disc[i], F64(q_target[i]), F64(R[i])))
        out[i] = F(_fma64(F64(beta), F64(mc[i]), F64(F64(1 - F64(beta)) * F64(off))))
    return out
