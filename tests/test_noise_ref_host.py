"""tests/noise_ref.py, the numpy restatement of the noise body, checked on its own: the moments of its normal draws, their range, the
extreme generator words, the OU step at theta = 1, and clip / clamp corner cases on hand-written rows."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import noise_ref as NR  # noqa: E402

F = np.float32


def test_moments_and_range_of_the_normal_draws():
    n = 128000
    rows = np.arange(n // 10)
    z = np.concatenate([NR.normal(11, c, NR.lanes(rows[c::4]).ravel()) for c in range(4)]).astype(np.float64)
    assert z.size == n
    assert abs(z.mean()) <= 5 / np.sqrt(n), z.mean()
    assert abs(z.var() - 1) <= 5 * np.sqrt(2 / n), z.var()
    assert np.abs(z).max() <= NR.Z_MAX
    # the cosine half and the radius half both take part: neither tail is missing
    assert (z > 3).sum() > 0 and (z < -3).sum() > 0


def test_keys_are_distinct_draws():
    a = NR.row_normals(5, 9, np.arange(64))
    assert a.shape == (64, 10) and len(np.unique(a.view(np.uint32))) > 630
    assert not np.array_equal(a, NR.row_normals(6, 9, np.arange(64)))          # seed
    assert not np.array_equal(a, NR.row_normals(5, 10, np.arange(64)))         # counter
    b = NR.row_normals(5, np.full(64, 9), np.arange(64))
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # column j of row r reads lanes r 32 + 2 j and + 1: neighbouring columns share no word
    assert np.array_equal(NR.lanes([0, 3])[:, [0, 9]], [[0, 18], [96, 114]])


def test_extreme_words_are_finite():
    for x1 in (0, 0xFF, 0xFFFFFF00, 0xFFFFFFFF):           # u1 = 2^-24 (twice), u1 = 1 (twice)
        for x2 in (0, 0x80000000, 0xFFFFFFFF):
            z = NR.normal_of([x1], [x2])[0]
            assert np.isfinite(z) and abs(z) <= NR.Z_MAX, (x1, x2, z)
    assert NR.normal_of([0xFFFFFFFF], [0])[0] == 0                  # u1 = 1: radius 0
    assert abs(NR.normal_of([0], [0])[0] - np.sqrt(48 * np.log(2))) < 1e-6   # u1 = 2^-24, angle 0: the largest draw, 5.768


def test_ou_with_theta_one_is_sigma_z():
    rng = np.random.default_rng(3)
    z = rng.standard_normal((50, 10)).astype(F)
    sig = NR.sigmas(0.05, 0.1)
    x = rng.standard_normal((50, 10)).astype(F) * F(7)
    got = NR.ou_step(x, 1.0, sig, z)
    assert np.array_equal(got.view(np.uint32), (sig * z).view(np.uint32))
    # theta < 1 keeps (1 - theta) of the state, formed as x - theta x
    got = NR.ou_step(x, 0.15, sig, z)
    assert np.array_equal(got, (x - F(0.15) * x) + sig * z) and got.dtype == F


def test_clip_and_clamp_corner_cases():
    sig = NR.sigmas(0.3, 0.3)
    z = np.array([[0, 1, -1, 0.5, 5.7, -5.7, 0.8333, 0.84, -0.84, 0]], F)
    t = NR.clipped(sig, z, 0.25)
    assert np.array_equal(t[0, [1, 2, 4, 5, 7, 8]], F([0.25, -0.25, 0.25, -0.25, 0.25, -0.25]))   # the clip binds
    assert t[0, 3] == F(0.3) * F(0.5) and t[0, 6] == F(0.3) * F(0.8333) < 0.25 and t[0, 0] == 0      # it does not
    assert np.array_equal(NR.clipped(sig, z, 0.0), sig * z)                                          # clip 0: no clip
    mu = np.array([[0.75, -0.75, 0.0, 1.0, 99.0, 170.0, -170.0, 0.0, 1.0, 180.0]], F)
    tt = np.array([[0.25, -0.25, 0.25, 0.0, 0.25, 0.25, -0.25, -0.25, -0.25, 0.0]], F)
    free = NR.apply(mu, tt, False)
    assert np.array_equal(free, F([[1.25, -1.25, 0.5, 1.0, 124.0, 260.0, -260.0, -90.0, -24.0, 180.0]]))
    held = NR.apply(mu, tt, True)
    assert np.array_equal(held, F([[1.0, -1.0, 0.5, 1.0, 100.0, 180.0, -180.0, -90.0, 0.0, 180.0]]))
    # a value already outside its bounds is pulled in by the clamp even under zero noise, and left alone without it
    out = np.array([[1.5, 0, 0, 0, -3.0, 200.0, 0, 0, 0, 0]], F)
    assert np.array_equal(NR.apply(out, np.zeros((1, 10), F), False), out)
    assert np.array_equal(NR.apply(out, np.zeros((1, 10), F), True)[0, [0, 4, 5]], F([1.0, 0.0, 180.0]))


def test_ulps32():
    a = F(1.0)
    assert NR.ulps32(a, np.nextafter(a, F(2))) == 1 and NR.ulps32(a, a) == 0
    assert NR.ulps32(F(0.0), F(-0.0)) == 0 and NR.ulps32(np.nextafter(F(0), F(1)), np.nextafter(F(0), F(-1))) == 2
