"""tests/sweep_ref.py without a GPU: its comparator accepts the report the reference itself forms — also with its double sums formed in
another order — and rejects each way a sweep can go wrong that the bounds are there to catch: a dropped tail row, a counted pad row,
a window shifted by one, a NaN counted as finite, a histogram bin off by one."""
import copy

import numpy as np
import pytest

import diag_ref as R
import sweep_ref as W

F = np.float32
N, B, FIRST, COUNT = 127, 32, 5, 70


def _memory(seed=3):
    rng = np.random.default_rng(seed)
    q, y, qp, mc = (rng.normal(0, 2, N).astype(F) for _ in range(4))
    reward = rng.uniform(-0.1, 0.1, N).astype(F)
    term = np.zeros(N, np.uint8)
    term[8::9] = 1
    term[-1] = 1
    mu, stored = rng.uniform(-1, 1, (N, 10)).astype(F), rng.uniform(-1, 1, (N, 10)).astype(F)
    return dict(q=q, y=y, q_policy=qp, mc=mc, reward=reward, terminal=term, mu=mu, stored=stored)


def _report(mem, first, n, **kw):
    return W.report(W.rows_of(**mem), first, n, B, **kw)


def _device_like(mem, first, n, pad_rows=0, drop_tail=0):
    """the report as a device would form it: float64 sums in chunk order (another association than fsum's), optionally with `pad_rows`
    copies of the last row counted or the last `drop_tail` rows left out"""
    rows = W.rows_of(**mem)
    take = list(range(first, first + n - drop_tail)) + [first + n - 1] * pad_rows
    out = {}
    for k in W.QUANTITIES:
        x = rows[k][take]
        v = x[np.isfinite(x)].astype(np.float64)
        s = ss = 0.0
        for c in range(0, len(v), B):
            s += float(np.sum(v[c:c + B]))
            ss += float(np.sum(v[c:c + B] ** 2))
        out[k] = {"min": float(v.min()) if v.size else 0.0, "max": float(v.max()) if v.size else 0.0, "sum": s, "sum_sq": ss,
                  "n_nonfinite": int(x.size - v.size)}
    out.update({"first": first, "n": n, "n_chunks": (n + B - 1) // B, "n_terminal": int(rows["terminal"][take].sum()),
                "n_action_match": int(rows["action_match"][take].sum()), "td_hist": R.histogram(rows["td"][take]),
                "actor_iter": 0, "critic_iter": 0})
    return out


@pytest.mark.parametrize("first,n", [(0, N), (FIRST, COUNT), (0, 0)])
def test_accepts_the_exact_report_and_another_order_of_sums(first, n):
    mem = _memory()
    ref = _report(mem, first, n)
    W.compare(copy.deepcopy(ref), ref)
    W.compare(_device_like(mem, first, n), ref)
    assert ref["n_chunks"] == {N: 4, COUNT: 3, 0: 0}[n]
    assert int(ref["td_hist"].sum()) + ref["td"]["n_nonfinite"] == n      # (no td of this memory is zero)


def test_terminal_and_match_counts():
    mem = _memory()
    ref = _report(mem, 0, N)
    assert ref["n_terminal"] == int(mem["terminal"].sum()) and mem["terminal"][-1]
    # GetAction: logit 2 never wins, the first maximum does
    ao = np.array([[0.1, 0.1, 9.0, 0.1], [0.0, 0.2, 9.0, 0.2], [-1, -2, 9.0, -0.5], [np.nan, 1, 1, 1]], F)
    assert W.get_action(ao).tolist() == [0, 1, 3, 0]
    assert 0 < ref["n_action_match"] < N


def test_rejects_a_dropped_tail_row():
    mem = _memory()
    with pytest.raises(R.Mismatch):
        W.compare(_device_like(mem, 0, N, drop_tail=1), _report(mem, 0, N))


def test_rejects_a_counted_pad_row():
    mem = _memory()
    with pytest.raises(R.Mismatch):
        W.compare(_device_like(mem, 0, N, pad_rows=1), _report(mem, 0, N))
    # ... even a pad row that moves no sum: the last row's td, q and q - mc zero, not terminal, no match — the other quantities still count it
    mem["q"][-1] = mem["y"][-1] = mem["mc"][-1] = 0
    with pytest.raises(R.Mismatch):
        W.compare(_device_like(mem, 0, N, pad_rows=1), _report(mem, 0, N))


def test_rejects_a_window_shifted_by_one():
    mem = _memory()
    ref = _report(mem, FIRST, COUNT)
    for shift in (-1, 1):
        dev = _device_like(mem, FIRST + shift, COUNT)
        dev["first"] = FIRST
        with pytest.raises(R.Mismatch):
            W.compare(dev, ref)


def test_rejects_a_nan_counted_as_finite():
    mem = _memory()
    mem["reward"][40] = np.nan
    mem["y"][41] = np.inf
    ref = _report(mem, 0, N)
    assert ref["reward"]["n_nonfinite"] == 1 and ref["y"]["n_nonfinite"] == 1 and ref["td"]["n_nonfinite"] == 1
    W.compare(_device_like(mem, 0, N), ref)
    for k in ("reward", "td"):
        dev = _device_like(mem, 0, N)
        dev[k]["n_nonfinite"] = 0
        with pytest.raises(R.Mismatch):
            W.compare(dev, ref)
    dev = _device_like(mem, 0, N)
    dev["y"]["max"] = float("inf")           # the infinity taken for the maximum
    with pytest.raises(R.Mismatch):
        W.compare(dev, ref)


def test_rejects_a_bin_off_by_one():
    mem = _memory()
    ref = _report(mem, 0, N)
    dev = _device_like(mem, 0, N)
    b = int(np.argmax(dev["td_hist"]))
    dev["td_hist"][b] -= 1
    dev["td_hist"][b + 1] += 1
    with pytest.raises(R.Mismatch):
        W.compare(dev, ref)


def test_refreshed_leaf_bound():
    td = np.array([0.0, 1e-3, -2.5, 17.0], F)
    want = W.refreshed_leaf(td, 1e-6, 0.6).astype(F)
    assert W.leaf_matches(want, td, 1e-6, 0.6).all()
    assert W.leaf_matches(np.nextafter(np.nextafter(want, F(np.inf)), F(np.inf)), td, 1e-6, 0.6).all()      # 2 steps: powf's allowance
    three = np.nextafter(np.nextafter(np.nextafter(want, F(np.inf)), F(np.inf)), F(np.inf))
    assert not W.leaf_matches(three, td, 1e-6, 0.6).any()
    assert (W.refreshed_leaf(td, 1e-6, 0.0) == 1.0).all()
