"""dqnhip_snapshot_async (DQN.Snapshot(..., wait=False)): the Caffe snapshot's files, under the same names, written behind training.
The synchronous dqnhip_snapshot is the yardstick of every test here: the four protobuf files are compared as bytes, the
`.replaymemory` as its decompressed bytes (Python's gzip verifies the member's CRC-32 — computed on the device — and ISIZE on the
way), and once more against a stream put together in the test with struct-style packing from dqnhip_read_memory.  The image is
frozen on the device: k_snap_pack_replay writes the stream in its final bytes (records of 4 S + 49 bytes, so every 4-byte phase and
an odd total length occur), (ring_head, ring_size) are read there.  No tolerances anywhere: files are bytes, learners are bits."""
import gzip
import os

import numpy as np
import pytest

from synth import synth_replay

pytestmark = pytest.mark.gpu

B, HID, CAP = 32, (64, 64), 1024
F = np.float32
_cache = {}


def _replay(S, seed, n):
    if (S, seed, n) not in _cache:
        _cache[(S, seed, n)] = synth_replay(np.random.default_rng(seed), n, S, mean_len=5)
    return _cache[(S, seed, n)]


def _fill(d, S, total, salt=0):
    """`total` transitions in batches that fit the capacity (AddTransitions keeps one slot free)"""
    cap = d.cfg.replay_capacity
    step = max(min(cap - 1, 400), 1)
    for k, first in enumerate(range(0, total, step)):
        d.add_transitions_arrays(*_replay(S, 5 + salt + k, min(step, total - first)))


def _make(pkg, tmp_path, name="live", S=58, cap=CAP, fill=300, seed=3, updates=3, B=B, hidden=HID, **kw):
    os.makedirs(str(tmp_path / name), exist_ok=True)
    d = pkg.DQN(S, minibatch=B, hidden=hidden, memory=cap, seed=seed, save_path=str(tmp_path / name / "dqn"), **kw)
    _fill(d, S, fill)
    if fill and updates:
        d.update_async_n(updates)
    return d


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _listing(directory, prefix):
    return sorted(f[len(prefix):] for f in os.listdir(directory) if f.startswith(prefix))


def _expected_stream(d):
    """the uncompressed .replaymemory of the learner's memory as it is now, from dqnhip_read_memory (src/dqn.cpp:1146-1178)"""
    n, S = d.memory_size(), d.state_size_
    out = np.int32(n).tobytes()
    if n == 0:
        return out
    s, a, r, mc, _, t = d.read_memory(0, n)
    rec = np.zeros((n, 4 * S + 49), np.uint8)
    rec[:, :4 * S] = s.view(np.uint8).reshape(n, 4 * S)
    rec[:, 4 * S:4 * S + 40] = a.view(np.uint8).reshape(n, 40)
    rec[:, 4 * S + 40:4 * S + 44] = r.view(np.uint8).reshape(n, 4)
    rec[:, 4 * S + 44:4 * S + 48] = mc.view(np.uint8).reshape(n, 4)
    rec[:, 4 * S + 48] = t != 0
    return out + rec.tobytes()


SUFFIXES = ["_actor_iter_%d.caffemodel", "_actor_iter_%d.solverstate", "_critic_iter_%d.caffemodel", "_critic_iter_%d.solverstate"]


def _both(d, tmp_path, tag, memory=True, threads=0):
    """the synchronous snapshot under one prefix, the asynchronous one under another, nothing in between -> the two prefixes"""
    ps, pa = str(tmp_path / (tag + "_sync")), str(tmp_path / (tag + "_async"))
    d.Snapshot(snapshot_prefix=ps, remove_old=False, snapshot_memory=memory)
    d.Snapshot(snapshot_prefix=pa, remove_old=False, snapshot_memory=memory, wait=False, compress_threads=threads)
    ia, ic = d.snapshot_wait()
    assert (ia, ic) == (d.actor_iter(), d.critic_iter())
    return ps, pa


def _same_files(ps, pa, it, memory=True):
    """every file of the asynchronous set against the synchronous one -> the decompressed stream"""
    for suf in SUFFIXES:
        a, b = _read(ps + suf % it), _read(pa + suf % it)
        assert a == b, suf
    if not memory:
        return None
    want = gzip.decompress(_read(ps + "_iter_%d.replaymemory" % it))
    got = gzip.decompress(_read(pa + "_iter_%d.replaymemory" % it))
    assert got == want
    return got


@pytest.mark.parametrize("S", [58, 59, 77])
def test_stream_identity(pkg, gpu, tmp_path, S):
    """plain windows of every size class on one learner, then windows that wrap: a learner of capacity n + 1 filled past it holds
    n transitions at ring_head != 0, straddling the ring's end"""
    d = _make(pkg, tmp_path, S=S, fill=0)
    for n in (0, 1, 2, 3, 4, 5, 255, 256, 257, CAP - 1):
        d.ClearReplayMemory()
        _fill(d, S, n, salt=n)
        assert d.memory_size() == n
        ps, pa = _both(d, tmp_path, "plain%d" % n)
        got = _same_files(ps, pa, 0)
        assert len(got) == 4 + n * (4 * S + 49) and got == _expected_stream(d), n
    d.close()
    for n in (1, 2, 3, 4, 5, 255, 256, 257, CAP - 1):
        w = _make(pkg, tmp_path, name="wrap%d" % n, S=S, cap=n + 1, fill=0)
        _fill(w, S, 2 * n + 3 if n < 6 else n + n // 2 + 1, salt=100 + n)
        assert w.memory_size() == n
        ps, pa = _both(w, tmp_path, "wrap%d" % n)
        got = _same_files(ps, pa, 0)
        assert got == _expected_stream(w), n
        term = np.frombuffer(got[4:], np.uint8).reshape(n, 4 * S + 49)[:, -1]
        assert set(term.tolist()) <= {0, 1}
        if n >= 255:
            assert 0 < int(term.sum()) < n                   # terminal flags mixed
        w.close()


PROTO_CASES = {
    "adam": dict(),
    "rmsprop": dict(solver="RMSProp", actor_lr=1e-5, critic_lr=1e-3, momentum=0.0, rms_decay=0.99),
    "adadelta": dict(solver="AdaDelta", actor_lr=1e-2, critic_lr=0.5, momentum=0.95, delta=1e-6),
    "fp16": dict(precision="fp16", B=128, hidden=(128, 128)),
}


@pytest.mark.parametrize("case", list(PROTO_CASES))
def test_protobuf_identity(pkg, gpu, tmp_path, case):
    d = _make(pkg, tmp_path, updates=4, **PROTO_CASES[case])
    assert d.actor_iter() == 4
    ps, pa = _both(d, tmp_path, case)
    _same_files(ps, pa, 4)
    two = case in ("adam", "adadelta", "fp16")
    m, v = d.get_params(0, 1), d.get_params(0, 2)
    assert m.any() and v.any() == two                        # (the histories the files hold are not trivially zero)
    d.close()


def test_names_with_remove_old_and_hiscore_prefix(pkg, gpu, tmp_path):
    """two successive snapshots with remove_old: the directory holds what the synchronous path leaves; a HiScore-style prefix with
    remove_old = 0 and snapshot_memory = 0 writes exactly the four files"""
    listings = {}
    for mode in ("syn", "asy"):                               # (directory names of one length: the solverstates hold the path)
        d = _make(pkg, tmp_path, name=mode, updates=2)
        wait = mode == "syn"
        d.Snapshot(wait=wait)                                 # Snapshot(): save_path_, remove_old, snapshot_memory
        d.update_async_n(3)
        d.Snapshot(wait=wait)
        assert d.snapshot_wait() == ((5, 5) if not wait else (0, 0))
        d.update_async_n(1)                                   # (at the same iteration the renames would carry the plain snapshot's files away)
        hs = str(tmp_path / mode / "dqn_HiScore-3")
        d.Snapshot(snapshot_prefix=hs, remove_old=False, snapshot_memory=False, wait=wait)
        d.snapshot_wait()
        listings[mode] = _listing(str(tmp_path / mode), "dqn")
        d.close()
    assert listings["asy"] == listings["syn"]
    assert listings["syn"] == sorted([s % 5 for s in SUFFIXES] + ["_iter_5.replaymemory"] + ["_HiScore-3" + s % 6 for s in SUFFIXES])
    for s in SUFFIXES:
        for pre, it in (("dqn", 5), ("dqn_HiScore-3", 6)):
            a, b = _read(str(tmp_path / "syn" / (pre + s % it))), _read(str(tmp_path / "asy" / (pre + s % it)))
            # (the solverstate names its caffemodel by the save path, which differs between the two directories)
            assert a.replace(b"/syn/", b"/asy/") == b, (pre, s)


def test_image_is_frozen_at_the_call(pkg, gpu, tmp_path):
    """what is enqueued behind the asynchronous call — 32 updates, appends that overwrite slots of the window — is not in the files: they
    equal what a twin (same seed, same calls) writes synchronously at the snapshot point"""
    a = _make(pkg, tmp_path, name="a", cap=CAP, fill=CAP + 200, use_graph=True)
    twin = _make(pkg, tmp_path, name="a", cap=CAP, fill=CAP + 200, use_graph=True)      # (the same save path: the solverstates name it)
    pa, pt = str(tmp_path / "img_async"), str(tmp_path / "img_twin")
    a.Snapshot(snapshot_prefix=pa, remove_old=False, wait=False)
    a.update_async_n(32)                                      # without waiting
    for k in range(3):
        a.add_transitions_arrays(*_replay(58, 41 + k, 400))
    assert a.snapshot_wait() == (3, 3)
    twin.Snapshot(snapshot_prefix=pt, remove_old=False)
    got = _same_files(pt, pa, 3)
    assert got == _expected_stream(twin) and got != _expected_stream(a)      # (the learner did move on)
    assert a.actor_iter() == 35
    a.close(); twin.close()


def _param_bits(d):
    return [d.get_params(net).view(np.uint32) for net in range(4)] + [d.get_params(net, k).view(np.uint32) for net in (0, 1) for k in (1, 2)]


def test_snapshotting_does_not_perturb_training(pkg, gpu, tmp_path):
    a, b = (_make(pkg, tmp_path, name=n, use_graph=True) for n in ("saver", "plain"))
    for k in range(3):
        a.Snapshot(wait=False)
        for d in (a, b):
            d.update_async_n(4)
            d.add_transitions_arrays(*_replay(58, 50 + k, 30))
    assert a.snapshot_wait() == (11, 11)
    for x, y in zip(_param_bits(a), _param_bits(b)):
        assert np.array_equal(x, y)
    assert a.actor_iter() == b.actor_iter() == 15
    a.close(); b.close()


def test_round_trip_through_the_loaders(pkg, gpu, tmp_path):
    a = _make(pkg, tmp_path, name="a", cap=CAP, fill=CAP + 77)
    p = str(tmp_path / "rt")
    a.Snapshot(snapshot_prefix=p, remove_old=False, wait=False)
    a.snapshot_wait()
    af, cf, mf = pkg.FindLatestSnapshot(p)
    assert af == p + "_actor_iter_3.solverstate" and cf == p + "_critic_iter_3.solverstate" and mf == p + "_iter_3.replaymemory"
    b = _make(pkg, tmp_path, name="b", cap=CAP, fill=10, seed=11, updates=0)
    b.LoadReplayMemory(mf)
    n = a.memory_size()
    assert b.memory_size() == n == CAP - 1
    ma, mb = a.read_memory(0, n), b.read_memory(0, n)
    for i in (0, 1, 2, 3, 5):                                 # states, actions, rewards, targets, terminal (next states are rebuilt by the loader)
        assert np.array_equal(ma[i].view(np.uint8), mb[i].view(np.uint8)), i
    b.RestoreActorSolver(af)
    b.RestoreCriticSolver(cf)
    assert (b.actor_iter(), b.critic_iter()) == (3, 3)
    for net in (0, 1):
        for kind in (0, 1, 2):
            assert np.array_equal(a.get_params(net, kind).view(np.uint32), b.get_params(net, kind).view(np.uint32)), (net, kind)
    a.close(); b.close()


def test_poll_wait_second_call_and_destroy(pkg, gpu, tmp_path):
    d = _make(pkg, tmp_path, cap=5000, fill=5200)
    assert d.snapshot_wait() == (0, 0) and d.snapshot_done() is True       # nothing in flight
    p0, p1, p2, p3 = (str(tmp_path / n) for n in ("p0", "p1", "p2", "p3"))
    d.Snapshot(snapshot_prefix=p0, remove_old=False)
    d.Snapshot(snapshot_prefix=p1, remove_old=False, wait=False)
    d.snapshot_done()                                        # (either answer is right here; test_poll_does_not_block has a job that cannot end)
    d.Snapshot(snapshot_prefix=p2, remove_old=False, wait=False, compress_threads=2)      # joins the first
    assert os.path.exists(p1 + "_iter_3.replaymemory")
    _same_files(p0, p1, 3)
    assert d.snapshot_wait() == (3, 3) and d.snapshot_done() is True
    _same_files(p0, p2, 3)
    # the synchronous calls join a snapshot in flight as well
    d.Snapshot(snapshot_prefix=p3, remove_old=False, wait=False, compress_threads=1)
    d.SnapshotReplayMemory(str(tmp_path / "plain.replaymemory"))
    assert d.snapshot_done() is True
    _same_files(p0, p3, 3)
    # dqnhip_destroy joins: the files are complete afterwards
    p4 = str(tmp_path / "p4")
    d.Snapshot(snapshot_prefix=p4, remove_old=False, wait=False)
    d.close()
    _same_files(p0, p4, 3)
    assert not [f for f in os.listdir(str(tmp_path)) if f.endswith(".tmp")]
    e = _make(pkg, tmp_path, updates=0, fill=0)
    with pytest.raises(pkg.DQNFatal, match="compress_threads -1 is outside"):
        e.Snapshot(snapshot_prefix=p4, remove_old=False, wait=False, compress_threads=-1)
    e.close()


def test_poll_does_not_block(pkg, gpu, tmp_path):
    """A job that cannot end while the test holds it: the first file the writer thread opens, <save path>_actor_iter_3.caffemodel.tmp,
    is a FIFO nobody reads yet, so the writer blocks in its open.  poll must answer False, at once.  When the test then reads the
    FIFO the job goes on and fails (a pipe cannot be fsynced): the wait reports that call's error, and the learner is usable."""
    import threading
    import time
    d = _make(pkg, tmp_path)
    fifo = str(tmp_path / "live" / "dqn_actor_iter_3.caffemodel.tmp")
    os.mkfifo(fifo)

    def drain():
        with open(fifo, "rb") as f:
            while f.read(1 << 16):
                pass

    valve = threading.Timer(20.0, drain)                     # so that a poll that did block fails this test instead of hanging it
    valve.start()
    d.Snapshot(remove_old=False, wait=False)
    t0 = time.perf_counter()
    done = [d.snapshot_done() for _ in range(3)]
    dt = time.perf_counter() - t0
    released_by_valve = not valve.is_alive()
    valve.cancel()
    assert done == [False, False, False] and dt < 1.0 and not released_by_valve, (done, dt)
    d.update_async_n(2)                                      # the learner goes on behind the stuck job
    assert d.actor_iter() == 5 and d.snapshot_done() is False
    drain()
    with pytest.raises(pkg.DQNFatal, match="dqnhip_snapshot_wait: the asynchronous snapshot to .* failed.*Invalid argument"):
        d.snapshot_wait()
    assert d.snapshot_done() is True
    assert not [f for f in os.listdir(str(tmp_path / "live")) if "iter_3" in f]
    d.Snapshot(wait=False)
    assert d.snapshot_wait() == (5, 5)
    d.close()


def test_unwritable_directory_fails_at_the_wait(pkg, gpu, tmp_path):
    d = _make(pkg, tmp_path)
    os.makedirs(str(tmp_path / "there"))
    bad = str(tmp_path / "no" / "such" / "dir" / "dqn")
    d.save_path_ = bad
    d.Snapshot(wait=False)                                   # the call itself has nothing to refuse
    with pytest.raises(pkg.DQNFatal, match="dqnhip_snapshot_wait: the asynchronous snapshot to .*no/such/dir/dqn failed"):
        d.snapshot_wait()
    assert not os.path.exists(str(tmp_path / "no"))
    d.snapshot_wait()                                        # reported once
    # the save path is writable, the prefix's directory is not: nothing appears under a final name there
    d.save_path_ = str(tmp_path / "there" / "dqn")
    d.Snapshot(snapshot_prefix=bad, remove_old=False, wait=False)
    with pytest.raises(pkg.DQNFatal, match="dqnhip_snapshot_async: the asynchronous snapshot to .*failed"):
        d.Snapshot(snapshot_prefix=str(tmp_path / "there" / "good"), remove_old=False, wait=False)      # the joining call reports it and does not run
    assert not [f for f in os.listdir(str(tmp_path / "there")) if f.startswith("good") or f.endswith(".tmp")]
    before = d.actor_iter()
    d.update_async_n(2)                                      # the learner is usable
    assert d.actor_iter() == before + 2
    d.Snapshot(wait=False)
    assert d.snapshot_wait() == (before + 2, before + 2)
    assert os.path.exists(str(tmp_path / "there" / ("dqn_iter_%d.replaymemory" % (before + 2))))
    d.close()


def test_v1_refusals(pkg, gpu, tmp_path):
    never = str(tmp_path / "never")

    def refused(d, match):
        with pytest.raises(pkg.DQNFatal, match="dqnhip_snapshot_async: the asynchronous snapshot: .*" + match):
            d.Snapshot(snapshot_prefix=never, remove_old=False, wait=False)
        assert d.snapshot_done() is True and not [f for f in os.listdir(str(tmp_path)) if f.startswith("never")]

    owner, sharer = _make(pkg, tmp_path, updates=0), _make(pkg, tmp_path, seed=4, updates=0)
    owner.ShareReplayMemory(sharer)
    for d in (owner, sharer):
        refused(d, "shares a replay memory")
    powner, psharer = _make(pkg, tmp_path, updates=0), _make(pkg, tmp_path, seed=4, updates=0)
    powner.ShareParameters(psharer, 1, 1)
    for d in (powner, psharer):
        refused(d, "shares parameters")
    dp = _make(pkg, tmp_path, updates=0, dp_world=2, dp_rank=0)
    refused(dp, "data-parallel")
    live = _make(pkg, tmp_path, updates=0, dp_world=1, dp_rank=0)      # a group of one: dp_world says nothing, the communicator is live
    live.dp_init(pkg.DQN.dp_unique_id())
    refused(live, "data-parallel")
    ph = _make(pkg, tmp_path)
    ph.update_phase(0)
    refused(ph, "a phased update is in progress")
    ph.update_abort()
    tm = _make(pkg, tmp_path)
    tm.set_kernel_timing(True)
    refused(tm, "kernel timing is on")
    tm.set_kernel_timing(False)
    tm.Snapshot(snapshot_prefix=never, remove_old=False, wait=False)
    assert tm.snapshot_wait() == (3, 3)
    # the synchronous snapshot of a refused learner works as before
    owner.Snapshot(snapshot_prefix=str(tmp_path / "owner"), remove_old=False)
    assert os.path.exists(str(tmp_path / "owner_iter_0.replaymemory"))
    for d in (sharer, owner, psharer, powner, dp, live, ph, tm):
        d.close()


def test_state_save_and_snapshot_in_flight_together(pkg, gpu, tmp_path):
    d = _make(pkg, tmp_path, cap=5000, fill=5200)
    s0, s1 = str(tmp_path / "s0.learnerstate"), str(tmp_path / "s1.learnerstate")
    p0, p1 = str(tmp_path / "p0"), str(tmp_path / "p1")
    d.save_state(s0)
    d.Snapshot(snapshot_prefix=p0, remove_old=False)
    d.save_state(s1, wait=False)
    d.Snapshot(snapshot_prefix=p1, remove_old=False, wait=False)
    d.update_async_n(4)                                      # neither job holds the caller's thread or the stream
    assert d.snapshot_wait() == (3, 3)
    d.save_state_wait()
    assert _read(s1) == _read(s0)
    _same_files(p0, p1, 3)
    # the other order, and a prioritized learner (the Caffe files carry no priorities either way)
    d.enable_prioritized_replay(alpha=0.6, beta0=0.4, beta_anneal_iters=20)
    d.update_async_n(2)
    p2, p3, s2, s3 = str(tmp_path / "p2"), str(tmp_path / "p3"), str(tmp_path / "s2.learnerstate"), str(tmp_path / "s3.learnerstate")
    d.Snapshot(snapshot_prefix=p2, remove_old=False)
    d.save_state(s2)
    d.Snapshot(snapshot_prefix=p3, remove_old=False, wait=False)
    d.save_state(s3, wait=False)
    d.save_state_wait()
    assert d.snapshot_wait() == (9, 9)
    assert _read(s3) == _read(s2)
    _same_files(p2, p3, 9)
    d.close()
