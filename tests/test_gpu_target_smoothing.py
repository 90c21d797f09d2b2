"""Target policy smoothing (dqnhip_target_noise_enable, k_target_smooth) through whole updates, against tests/noise_ref.py.

  * "target_noise_z" against the reference's draws on the keys (seed, "target_noise_counter", r 32 + 2 j): equal or one float32 ulp
    away (device double log / cos against numpy's), at least 99 % bit-equal — a cap, so that the allowance cannot hide a wrong key;
    the counter advances by one per update;
  * "actor_target_smoothed" bit for bit from "actor_target_out" (the clean mu'(s'), which stays readable) and the device's own z, with
    sigma 0.3 and clip 0.25 so that rows where the clip binds, where the clamp binds and where neither does all occur;
  * "q_target" against a float64 numpy forward of the target critic on (s', a~) within QTOL + QRTOL |q| of
    tests/test_gpu_update_parity.py, on weights large enough that in the reference the clean and the smoothed q' differ by at least
    100 QTOL on at least half the rows — asserted on the reference, so dropping the noise fails the test;
  * sigma = 0 with clamp off: every bit of a plain learner on the same schedule (DQNHIP_TUNE_SEPARATE_CRITIC_FIRST_LAYERS);
  * sixteen single updates against one update_async_n(16), eager and captured, bit for bit: sixteen consecutive counters;
  * with n-step returns and with prioritized replay: runs, plan bits, one launch more than the same learner on the forced schedule;
  * save, new learner, enable, load, continue: the bits of never stopping; every refusal names target smoothing.
Shapes: B = 32, S = 58, hidden 2 x 64, capacity 512."""
import numpy as np
import pytest

import noise_ref as NR
from oracle import torch_ref
from synth import det_indices, synth_replay
from test_gpu_update_parity import QRTOL, QTOL

pytestmark = pytest.mark.gpu

B, S, HID, CAP, N = 32, 58, (64, 64), 512, 400
F = np.float32
SEED = 0x5EED5EED77
SMOOTH = dict(sigma_logits=0.3, sigma_params=0.3, clip=0.25, clamp=True, seed=SEED)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _replay():
    return synth_replay(np.random.default_rng(5), N, S, mean_len=10)


def _make(pkg, smooth=None, n_step=None, per=None, wscale=1.0, **kw):
    d = pkg.DQN(S, minibatch=B, hidden=HID, memory=CAP, seed=3, **kw)
    if wscale != 1.0:
        rng = np.random.default_rng(9)
        for net, actor in ((0, True), (1, False)):
            d.set_params(net, torch_ref.init_params_np(rng, S, HID, actor) * wscale)
            d.CloneNet(net)
    d.add_transitions_arrays(*_replay())
    if per is not None:
        d.enable_prioritized_replay(**per)
    if n_step is not None:
        d.enable_n_step(n_step)
    if smooth is not None:
        d.enable_target_smoothing(**smooth)
    return d


def _bits(d):
    out = [d.get_params(net).view(np.uint32) for net in range(4)]
    out += [d.get_params(net, kind).view(np.uint32) for net in (0, 1) for kind in (1, 2)]
    return out


def _same(a, b, what):
    for k, (g, w) in enumerate(zip(_bits(a), _bits(b))):
        assert np.array_equal(g, w), (what, "arena", k)
    for name in ("q_target", "y", "q_train"):
        assert np.array_equal(bits(a.debug_read(name)), bits(b.debug_read(name))), (what, name)


def critic64(vec, s, a):
    """float64 forward of a critic from its dense parameter vector (Caffe order: W[n, k], b[n] per layer; leaky ReLU 0.01)"""
    x = np.concatenate([s, a], axis=1).astype(np.float64)
    off, shapes = 0, torch_ref.layout(S + 10, HID, (1,))
    for i, (n, k) in enumerate(shapes):
        W = vec[off:off + n * k].astype(np.float64).reshape(n, k); off += n * k
        b = vec[off:off + n].astype(np.float64); off += n
        x = x @ W.T + b
        if i < len(HID):
            x = np.where(x > 0, x, 0.01 * x)
    assert off == vec.size
    return x[:, 0]


def test_noise_smoothed_action_and_q_target(pkg, gpu):
    d = _make(pkg, smooth=SMOOTH, wscale=10.0)
    got = d.target_smoothing()
    assert got["clip"] == 0.25 and got["sigma_params"] == F(0.3) and got["clamp"] and got["seed"] == SEED
    X = _replay()
    idx = det_indices(11, 3, B, N)
    sig = NR.sigmas(0.3, 0.3)
    n_equal = n_draws = n_clip = n_clamp = n_free = 0
    c0 = None
    for u in range(3):
        w_ct = d.get_params(3)                                        # the target critic this update's q' is formed with
        d.UpdateActorCritic(idx[u])
        c = d.target_noise_counter()
        c0 = c if c0 is None else c0
        assert c == c0 + u
        z, mu, sm = d.debug_read("target_noise_z"), d.debug_read("actor_target_out"), d.debug_read("actor_target_smoothed")
        dist = NR.ulps32(z, NR.row_normals(SEED, c, np.arange(B)))
        assert dist.max() <= 1, (u, dist.max())
        n_equal += int((dist == 0).sum()); n_draws += dist.size
        t = NR.clipped(sig, z, 0.25)                                  # from the device's own z: bit for bit from here on
        want = NR.apply(mu, t, True)
        np.testing.assert_array_equal(bits(sm), bits(want), err_msg="update %d" % u)
        clipped = np.abs(sig * z) > F(0.25)
        clamped = bits(NR.apply(mu, t, False)) != bits(want)
        n_clip += int(clipped.sum()); n_clamp += int(clamped.sum()); n_free += int((~clipped & ~clamped).sum())
        nx = X[4][idx[u]]
        q_clean, q_smooth = critic64(w_ct, nx, mu), critic64(w_ct, nx, sm)
        # a condition on the inputs: the noise moves q' far beyond the tolerance on at least half the rows
        assert (np.abs(q_clean - q_smooth) >= 100 * QTOL).sum() >= B // 2, np.abs(q_clean - q_smooth)
        q = d.debug_read("q_target")
        assert np.all(np.abs(q - q_smooth) <= QTOL + QRTOL * np.abs(q_smooth)), (u, np.abs(q - q_smooth).max())
    assert n_clip > 0 and n_clamp > 0 and n_free > 0, (n_clip, n_clamp, n_free)
    assert n_equal >= 0.99 * n_draws, (n_equal, n_draws)
    d.close()


def test_zero_sigma_without_clamp_is_a_plain_learner_on_the_same_schedule(pkg, gpu):
    plain = _make(pkg, tuning=pkg.capi.TUNE_SEPARATE_CRITIC_FIRST_LAYERS)
    zero = _make(pkg, smooth=dict(sigma_logits=0.0, sigma_params=0.0, clip=0.25, clamp=False, seed=1))
    idx = det_indices(11, 3, B, N)
    for u in range(3):
        want, got = plain.UpdateActorCritic(idx[u]), zero.UpdateActorCritic(idx[u])
        assert np.array_equal(bits(got), bits(want)), (u, got, want)
        _same(zero, plain, u)
    assert np.array_equal(bits(zero.debug_read("actor_target_smoothed")), bits(zero.debug_read("actor_target_out")))
    plain.close(); zero.close()


@pytest.mark.parametrize("use_graph", [True, False])
def test_update_async_n_is_sixteen_single_updates(pkg, gpu, use_graph):
    a, b = _make(pkg, smooth=SMOOTH, use_graph=use_graph), _make(pkg, smooth=SMOOTH, use_graph=not use_graph)
    a.update_async_n(16)
    counters = []
    for u in range(16):
        b.UpdateActorCritic()
        counters.append(b.target_noise_counter())
    assert counters == list(range(counters[0], counters[0] + 16))
    _same(a, b, use_graph)                                            # sixteen different noises: the same sixteen counters
    assert np.array_equal(bits(np.asarray(a.read_stats(), F)), bits(np.asarray(b.read_stats(), F)))
    assert a.target_noise_counter() == counters[-1]
    assert np.array_equal(bits(a.debug_read("target_noise_z")), bits(b.debug_read("target_noise_z")))
    assert np.array_equal(bits(a.debug_read("actor_target_smoothed")), bits(b.debug_read("actor_target_smoothed")))
    # ... and sixteen different ones: a learner whose noise never moves ends elsewhere
    a.update_async_n(1)
    assert not np.array_equal(bits(a.debug_read("target_noise_z")), bits(b.debug_read("target_noise_z")))
    a.close(); b.close()


def test_composes_with_n_step_and_prioritized_replay(pkg, gpu):
    T = pkg.capi.TUNE_SEPARATE_CRITIC_FIRST_LAYERS
    for extra in (dict(), dict(n_step=3), dict(per=dict()), dict(n_step=3, per=dict())):
        forced, d = _make(pkg, tuning=T, use_graph=True, **extra), _make(pkg, smooth=SMOOTH, use_graph=True, **extra)
        pf, pd = forced.update_plan(), d.update_plan()
        assert set(pd["forms"]) == set(pf["forms"]) | {"target_smoothing"}, (extra, pd["forms"], pf["forms"])
        assert "first_layers_merged" not in pd["forms"] and "early_gather_l0" not in pd["forms"]
        if "n_step" in extra:
            assert "n_step" in pd["forms"]
        if "per" in extra:
            assert "prioritized" in pd["forms"]
        for k in ("launches_single", "launches_graph_first", "launches_in_graph"):
            assert pd[k] == pf[k] + 1, (extra, k, pd[k], pf[k])          # k_target_smooth, counted from a capture
        d.UpdateActorCritic()
        d.update_async_n(3)
        assert all(np.isfinite(d.read_stats()))
        c = d.target_noise_counter()
        assert NR.ulps32(d.debug_read("target_noise_z"), NR.row_normals(SEED, c, np.arange(B))).max() <= 1
        forced.close(); d.close()
    never = _make(pkg)
    assert "target_smoothing" not in never.update_plan()["forms"] and never.target_smoothing() is None
    never.close()


def test_resume_continues_bit_for_bit(pkg, gpu, tmp_path):
    path = str(tmp_path / "learner.state")
    a = _make(pkg, smooth=SMOOTH)
    for u in range(2):
        a.UpdateActorCritic()
    a.save_state(path)
    b = pkg.DQN(S, minibatch=B, hidden=HID, memory=CAP, seed=3)
    b.enable_target_smoothing(**SMOOTH)          # a hyper-parameter, not state: the file holds the counter, not the config
    b.load_state(path)
    for u in range(2):
        want, got = a.UpdateActorCritic(), b.UpdateActorCritic()
        assert np.array_equal(bits(got), bits(want))
        assert a.target_noise_counter() == b.target_noise_counter()
        assert np.array_equal(bits(a.debug_read("target_noise_z")), bits(b.debug_read("target_noise_z")))
        _same(a, b, ("resumed", u))
    a.close(); b.close()


def test_refusals_name_target_smoothing(pkg, gpu):
    d = _make(pkg, smooth=SMOOTH)
    idx = np.arange(B, dtype=np.int32)
    m = "target smoothing"
    with pytest.raises(pkg.DQNFatal, match=m):
        d.UpdateActorCriticChained(idx, idx)
    with pytest.raises(pkg.DQNFatal, match=m):
        d.UpdateActorCriticPipelined(idx)
    with pytest.raises(pkg.DQNFatal, match=m):
        d.update_indexed_n(np.stack([idx, idx]))
    with pytest.raises(pkg.DQNFatal, match=m):
        d.update_phase(0, idx)
    with pytest.raises(pkg.DQNFatal, match=m):
        d.dp_init(pkg.DQN.dp_unique_id())
    other = _make(pkg)
    with pytest.raises(pkg.DQNFatal, match=m):
        d.ShareParameters(other, 1, 1)
    with pytest.raises(pkg.DQNFatal, match=m):
        other.ShareReplayMemory(d)
    half = pkg.DQN(S, minibatch=128, hidden=(128, 128), memory=CAP, seed=3, precision="fp16")
    with pytest.raises(pkg.DQNFatal, match=m):
        half.enable_target_smoothing()
    rank = pkg.DQN(S, minibatch=B, hidden=HID, memory=CAP, seed=3, dp_world=2, dp_rank=0)
    with pytest.raises(pkg.DQNFatal, match=m):
        rank.enable_target_smoothing()
    import ctypes as C
    cfg = pkg.capi.NoiseConfig()
    assert d.lib.dqnhip_noise_default_config(C.byref(cfg), pkg.capi.NOISE_TARGET) == 0
    assert (cfg.sigma_logits, cfg.sigma_params, cfg.theta, cfg.clip, cfg.clamp) == (F(0.1), F(0.1), 1.0, 0.25, 1)
    cfg.theta = 0.5
    assert d.lib.dqnhip_target_noise_enable(other.h, C.byref(cfg)) != 0 and b"theta must be 1" in d.lib.dqnhip_last_error() and m.encode() in d.lib.dqnhip_last_error()
    with pytest.raises(pkg.DQNFatal, match="sigma_params >= 0"):
        other.enable_target_smoothing(sigma_params=-1.0)
    with pytest.raises(pkg.DQNFatal, match="not enabled"):
        other.debug_read("target_noise_z")
    # the replay sweep keeps evaluating the clean target, and the learner still works
    d.evaluate_memory()
    d.UpdateActorCritic(idx)
    assert all(np.isfinite(d.read_stats())) and other.target_smoothing() is None
    for x in (d, other, half, rank):
        x.close()
