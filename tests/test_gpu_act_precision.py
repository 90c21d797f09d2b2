"""fp16 acting of the fp16 learner (dqnhip_set_act_precision): select_actions*, critic_forward on the fp16 weight mirrors.

The spec is the function the update's own forward passes compute, i.e. what tower16 + heads32 of tests/test_gpu_fp16.py emulate:
inputs rounded to fp16, every tower layer an fp16 GEMM with fp32 accumulation / bias / leaky ReLU stored as fp16, fp32 heads on the
fp16 tower top.  Bounds are close16's (same rounding points, different fp32 summation order: 0.9-quantile <= 3e-4, max <= 5e-3 of the
reference's scale).  Everything that compares two runs of the SAME launch sequence is bit for bit."""
import ctypes as C

import numpy as np
import pytest

from helpers import make_pair
from test_gpu_fp16 import _actor32, close16, heads32, tower16, unpack

pytestmark = pytest.mark.gpu

ACTOR, CRITIC, ACTOR_TARGET, CRITIC_TARGET = 0, 1, 2, 3
B = 128
A_MIN = np.array([-1] * 4 + [0, -180, -180, -180, 0, -180], np.float32)
A_MAX = np.array([1] * 4 + [100, 180, 180, 180, 100, 180], np.float32)


def learner(pkg, S=59, hidden=(256, 128), wscale=5.0, **kw):
    kw.setdefault("precision", "fp16")
    return make_pair(pkg, B=B, S=S, hidden=hidden, n_replay=2048, wscale=wscale, **kw)


def emu_actor(dqn, net, x, S, hid):
    p = unpack(dqn.get_params(net), S, hid, (4, 6))
    return heads32(tower16(x, p, len(hid))[1], p, len(hid))


def emu_critic(dqn, net, x, a, S, hid):
    p = unpack(dqn.get_params(net), S + 10, hid, (1,))
    return heads32(tower16(np.concatenate([x, a], 1), p, len(hid))[1], p, len(hid))[:, 0]


def actions(rng, n):
    """actor outputs with the action parameters over their full ranges (+-180 degrees, 0 .. 100 power)"""
    return (A_MIN + (A_MAX - A_MIN) * rng.random((n, 10), dtype=np.float32)).astype(np.float32)


def test_switch(pkg, gpu):
    S, hid = 59, (256, 128)
    dqn, orc, data, rng = learner(pkg, S, hid)
    st = data[0][:50]
    assert dqn.act_precision == "fp32"                                         # the default
    first = dqn.SelectActionGreedily(st)
    np.testing.assert_allclose(first, _actor32(dqn, st, S, hid), rtol=1e-4, atol=1e-5)   # fp32 master weights, exact-fp32 kernels
    q_first = dqn.CriticForward(st, data[1][:50])
    dqn.set_act_precision("fp16")
    assert dqn.act_precision == "fp16"
    second = dqn.SelectActionGreedily(st)
    close16(second, emu_actor(dqn, ACTOR, st, S, hid), "fp16 acting")
    assert not np.array_equal(first, second)                                   # (another function: fp16-rounded inputs and weights)
    dqn.set_act_precision("fp32")
    assert dqn.act_precision == "fp32"
    np.testing.assert_array_equal(dqn.SelectActionGreedily(st), first)         # bit for bit what it was
    np.testing.assert_array_equal(dqn.CriticForward(st, data[1][:50]), q_first)
    with pytest.raises(pkg.DQNFatal):
        dqn.set_act_precision("bf16")
    dqn.close(); orc.close()
    d32, o32, _, _ = learner(pkg, S, hid, precision="fp32")
    with pytest.raises(pkg.DQNFatal, match="precision"):
        d32.set_act_precision("fp16")
    assert d32.act_precision == "fp32"
    d32.set_act_precision("fp32")                                              # (allowed: what it does anyway)
    with pytest.raises(pkg.DQNFatal, match="precision"):
        pkg.DQN(S, minibatch=32, hidden=hid, memory=1000, act_precision="fp16")
    d32.close(); o32.close()
    d16 = pkg.DQN(S, minibatch=B, hidden=hid, memory=1000, precision="fp16", act_precision="fp16")
    assert d16.act_precision == "fp16"
    d16.close()


# By hgemm_plan 4096 and 8192 rows of a 1024-wide layer take the 128x128 and the 256x128 tile, everything smaller the 64x64 split-K
# tile; 1, 50: one tile with pad rows; 64: exactly one; 65, 200: two and four tiles, the last with pad rows
@pytest.mark.parametrize("S,hid,wscale,ns", [
    (59, (256, 128), 5.0, (1, 50, 64, 65, 200)),
    (77, (128, 256), 5.0, (1, 50, 64, 65, 200)),
    (58, (1024, 1024), 2.0, (4096, 8192)),
])
def test_emulation(pkg, gpu, S, hid, wscale, ns):
    dqn, orc, data, rng = learner(pkg, S, hid, wscale, tau=0.25)
    for it in range(2):                                                        # tau = 0.25: the targets now differ from the online nets
        dqn.UpdateActorCritic(rng.integers(0, 2048, size=B))
    assert not np.array_equal(dqn.get_params(ACTOR), dqn.get_params(ACTOR_TARGET))
    assert not np.array_equal(dqn.get_params(CRITIC), dqn.get_params(CRITIC_TARGET))
    dqn.set_act_precision("fp16")
    x_all = np.concatenate([data[0], rng.uniform(-1, 1, size=(max(ns) - 2048, S)).astype(np.float32)]) if max(ns) > 2048 else data[0]
    a_all = actions(rng, max(ns))
    # one emulation per net on the largest n: a row's result does not depend on the other rows
    want = {net: emu_actor(dqn, net, x_all[:max(ns)], S, hid) for net in (ACTOR, ACTOR_TARGET)}
    want.update({net: emu_critic(dqn, net, x_all[:max(ns)], a_all, S, hid) for net in (CRITIC, CRITIC_TARGET)})
    for n in ns:
        for net in (ACTOR, ACTOR_TARGET):
            close16(dqn.SelectActionGreedily(x_all[:n], net), want[net][:n], "actor net %d n %d" % (net, n))
        for net in (CRITIC, CRITIC_TARGET):
            if n > 1:
                close16(dqn.CriticForward(x_all[:n], a_all[:n], net), want[net][:n], "critic net %d n %d" % (net, n))
            else:
                # close16 takes its scale from the values it is given and one q has none but its own: sixteen n = 1 calls, compared together
                got = np.array([dqn.CriticForward(x_all[j:j + 1], a_all[j:j + 1], net)[0] for j in range(16)])
                close16(got, want[net][:16], "critic net %d, n = 1 calls" % net)
    dqn.close(); orc.close()


def test_padding_and_row_independence(pkg, gpu):
    S, hid = 59, (256, 128)
    dqn, orc, data, rng = learner(pkg, S, hid)
    dqn.set_act_precision("fp16")
    x = data[0]
    a = actions(rng, 65)
    o64, q64 = dqn.SelectActionGreedily(x[:64]), dqn.CriticForward(x[:64], a[:64])
    for j in (0, 1, 31, 49, 63):                                               # row j of n = 64 == the n = 1 call on state j
        np.testing.assert_array_equal(dqn.SelectActionGreedily(x[j:j + 1])[0], o64[j])
        np.testing.assert_array_equal(dqn.CriticForward(x[j:j + 1], a[j:j + 1])[0], q64[j])
    np.testing.assert_array_equal(dqn.SelectActionGreedily(x[:50]), o64[:50])  # pad rows change nothing
    np.testing.assert_array_equal(dqn.CriticForward(x[:50], a[:50]), q64[:50])
    np.testing.assert_array_equal(dqn.SelectActionGreedily(x[:65])[:64], o64)  # 128 rows: the same 64x64 tile, twice
    np.testing.assert_array_equal(dqn.CriticForward(x[:65], a[:65])[:64], q64)
    dqn.close(); orc.close()


def test_stale_panels(pkg, gpu):
    """the acting panels are reused between actor and critic passes and between row counts: what an earlier call left in them —
    action columns at the ends of their ranges where the actor's pad columns are, rows beyond n — must not reach a later result"""
    S, hid = 59, (256, 128)
    dqn, orc, data, rng = learner(pkg, S, hid)
    dqn.set_act_precision("fp16")
    x = data[0]
    before = dqn.SelectActionGreedily(x[:50])
    extreme = np.where(rng.random((200, 10)) < 0.5, A_MIN, A_MAX).astype(np.float32)
    q = dqn.CriticForward(x[:200], extreme)
    assert np.all(np.isfinite(q))
    np.testing.assert_array_equal(dqn.SelectActionGreedily(x[:50]), before)
    one = dqn.SelectActionGreedily(x[7:8])
    dqn.SelectActionGreedily(x[:200])
    np.testing.assert_array_equal(dqn.SelectActionGreedily(x[7:8]), one)
    q1 = dqn.CriticForward(x[7:8], extreme[7:8])
    np.testing.assert_array_equal(q1[0], q[7])
    dqn.close(); orc.close()


def test_mirrors_follow_host_side_weight_changes(pkg, gpu):
    S, hid = 59, (256, 128)
    dqn, orc, data, rng = learner(pkg, S, hid)
    dqn.set_act_precision("fp16")
    x = data[0][:100]
    old = dqn.SelectActionGreedily(x)
    w = dqn.get_params(ACTOR)
    w2 = (w * np.float32(0.5) + rng.standard_normal(w.size).astype(np.float32) * np.float32(0.02)).astype(np.float32)
    dqn.set_params(ACTOR, w2)                                                  # no update in between: the mirror is dirty
    got = dqn.SelectActionGreedily(x)
    close16(got, emu_actor(dqn, ACTOR, x, S, hid), "after set_params")
    assert not np.array_equal(got, old)
    np.testing.assert_array_equal(dqn.SelectActionGreedily(x, ACTOR_TARGET), old)          # (the target still has the old weights)
    dqn.CloneNet(ACTOR)
    np.testing.assert_array_equal(dqn.get_params(ACTOR_TARGET), w2)
    got_t = dqn.SelectActionGreedily(x, ACTOR_TARGET)
    close16(got_t, emu_actor(dqn, ACTOR_TARGET, x, S, hid), "after clone_to_target")
    np.testing.assert_array_equal(got_t, got)                                  # same weights, same launches
    wc = dqn.get_params(CRITIC)
    dqn.set_params(CRITIC, (wc * np.float32(0.75)).astype(np.float32))
    a = actions(rng, 100)
    close16(dqn.CriticForward(x, a), emu_critic(dqn, CRITIC, x, a, S, hid), "critic after set_params")
    dqn.close(); orc.close()


def _hip():
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    return hip


@pytest.mark.parametrize("n", [1, 70])
def test_host_and_device_entry_agree(pkg, gpu, n):
    S, hid = 59, (256, 128)
    dqn, orc, data, rng = learner(pkg, S, hid)
    dqn.set_act_precision("fp16")
    x = np.ascontiguousarray(data[0][:n], np.float32)
    host = dqn.SelectActionGreedily(x)
    hip = _hip()
    ds, do = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(ds), x.nbytes) == 0 and hip.hipMalloc(C.byref(do), n * 40) == 0
    assert hip.hipMemcpy(ds, x.ctypes.data_as(C.c_void_p), x.nbytes, 1) == 0
    dqn._ck(dqn.lib.dqnhip_select_actions_device(dqn.h, ds, n, do))
    assert hip.hipDeviceSynchronize() == 0
    dev = np.empty((n, 10), np.float32)
    assert hip.hipMemcpy(dev.ctypes.data_as(C.c_void_p), do, dev.nbytes, 2) == 0
    hip.hipFree(ds); hip.hipFree(do)
    np.testing.assert_array_equal(dev, host)
    dqn.close(); orc.close()


def test_acting_is_the_policy_the_update_differentiates(pkg, gpu):
    S, hid = 59, (256, 128, 128, 128)
    dqn, orc, data, rng = learner(pkg, S, hid)
    dqn.set_act_precision("fp16")
    idx = rng.integers(0, 2048, size=B)
    acted = dqn.SelectActionGreedily(data[0][idx])
    dqn.update_phase(0, idx)
    close16(acted, dqn.debug_read("actor_out"), "acting vs the update's mu(s)")
    dqn.update_phase(1); dqn.update_phase(2)
    loss, q = dqn.read_stats()
    assert np.isfinite(loss) and np.isfinite(q)
    dqn.close(); orc.close()
