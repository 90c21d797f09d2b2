"""dqnhip_save_state_async (DQN.save_state(path, wait=False)): the file it writes is, byte for byte, the file the synchronous
dqnhip_save_state writes at the same point of the learner's stream — the synchronous save is the yardstick of every test here, the
asynchronous path is never compared against itself.  The image is frozen on the device by the pack kernels (parameters out of the
padded arenas, the ring's window in logical order with (head, size) read on the device, the priority leaves) and checksummed there
(k_state_crc); a writer thread streams it to the file.  No tolerances: files are compared as bytes, learners as bits."""
import os

import numpy as np
import pytest

import state_ref
from synth import synth_replay
from test_gpu_state_file import _bits, _same

pytestmark = pytest.mark.gpu

B, HID = 32, (64, 128)
F = np.float32
_cache = {}


def _replay(S, seed, n):
    if (S, seed, n) not in _cache:
        _cache[(S, seed, n)] = synth_replay(np.random.default_rng(seed), n, S, mean_len=10)
    return _cache[(S, seed, n)]


def _make(pkg, S=58, cap=96, fill=130, seed=3, B=B, hidden=HID, per=None, updates=3, **kw):
    d = pkg.DQN(S, minibatch=B, hidden=hidden, memory=cap, seed=seed, **kw)
    for k, first in enumerate(range(0, fill, max(cap // 2, 1))):       # (a batch has to fit the capacity)
        d.add_transitions_arrays(*_replay(S, 5 + k, min(cap // 2, fill - first)))
    if per is not None:
        d.enable_prioritized_replay(**per)
    if fill and updates:
        d.update_async_n(updates)
    return d


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _pair(pkg, d, tmp_path, **kw):
    """p0 synchronously, p1 asynchronously with nothing in between -> (bytes of p0, bytes of p1)"""
    p0, p1 = str(tmp_path / "p0.learnerstate"), str(tmp_path / "p1.learnerstate")
    d.save_state(p0, **kw)
    d.save_state(p1, wait=False, **kw)
    d.save_state_wait()
    assert not os.path.exists(p1 + ".tmp")
    a, b = _read(p0), _read(p1)
    assert len(a) == len(b) == pkg.state_info(p1)["file_bytes"]
    assert a == b
    return a, b


@pytest.mark.parametrize("S", [59, 58])
def test_wrapped_window_odd_size_pad_columns(pkg, gpu, tmp_path, S):
    d = _make(pkg, S=S, cap=96, fill=130)
    assert d.memory_size() == 95                     # odd RTRM; 130 appended into 96 slots: head != 0
    _pair(pkg, d, tmp_path)
    info = pkg.state_info(str(tmp_path / "p1.learnerstate"))
    assert info["memory_size"] == 95 and info["has_memory"] == 1 and info["actor_iter"] == 3
    d.close()


def test_capacity_5000_filled_spans_many_crc_chunks(pkg, gpu, tmp_path):
    d = _make(pkg, cap=5000, fill=5200)
    assert d.memory_size() == 4999
    _pair(pkg, d, tmp_path)
    d.close()


def test_empty_memory(pkg, gpu, tmp_path):
    d = _make(pkg, fill=0)
    assert d.memory_size() == 0
    _pair(pkg, d, tmp_path)
    assert pkg.state_info(str(tmp_path / "p1.learnerstate"))["memory_size"] == 0
    d.close()


def test_without_memory(pkg, gpu, tmp_path):
    d = _make(pkg)
    _pair(pkg, d, tmp_path, memory=False)
    assert pkg.state_info(str(tmp_path / "p1.learnerstate"))["has_memory"] == 0
    d.close()


def test_prioritized(pkg, gpu, tmp_path):
    d = _make(pkg, cap=200, fill=260, per=dict(alpha=0.6, beta0=0.4, beta_anneal_iters=20), updates=4)
    leaves = d.per_priorities(0, d.memory_size())
    assert len(np.unique(leaves)) > 2                # the updates wrote priorities back: the leaves differ
    _pair(pkg, d, tmp_path)
    assert pkg.state_info(str(tmp_path / "p1.learnerstate"))["has_per"] == 1
    d.close()


def test_fp16_dynamic_loss_scale(pkg, gpu, tmp_path):
    d = _make(pkg, B=128, hidden=(128, 128), cap=300, fill=350, precision="fp16", loss_scale_mode="dynamic", loss_scale_growth_interval=3,
              updates=5)
    _pair(pkg, d, tmp_path)
    assert pkg.state_info(str(tmp_path / "p1.learnerstate"))["has_loss_scale"] == 1
    d.close()


def test_every_optional_section_at_once(pkg, gpu, tmp_path):
    """SOLV, LRSC, LSCL, the memory, PERC / PERL and USER in one file: a non-Adam solver under an lr policy with a weight decay, fp16 with
    dynamic loss scaling, prioritized replay, a wrapped window of odd size, user bytes of odd length"""
    d = _make(pkg, S=59, B=128, hidden=(128, 128), cap=96, fill=130, precision="fp16", loss_scale_mode="dynamic", loss_scale_growth_interval=3,
              solver="RMSProp", actor_lr=1e-5, critic_lr=1e-3, momentum=0.0, rms_decay=0.99, lr_policy="step", lr_gamma=0.5, lr_stepsize=2,
              weight_decay=1e-3, regularization="L2", per=dict(alpha=0.6, beta0=0.4, beta_anneal_iters=20), updates=5)
    assert d.memory_size() == 95
    user = bytes(range(7))
    a, _ = _pair(pkg, d, tmp_path, user=user)
    info, sections = state_ref.read_bytes(a)
    assert list(sections) == ["WGT0", "WGT1", "WGT2", "WGT3", "ADM0", "ADV0", "ADM1", "ADV1", "SOLV", "LRSC", "DEVS", "LSCL", "HOST",
                              "RING", "RSTA", "RNXT", "RACT", "RREW", "RMCT", "RTRM", "PERC", "PERL", "USER"]
    out = state_ref.decode(info, sections)
    assert out["states"].shape == (95, 59) and len(out["terminal"]) == len(out["leaves"]) == 95 and out["ring"]["ring_head"] != 0
    assert out["user"] == user and out["dev"]["actor_iter"] == 5 and len(sections["SOLV"]) == 16 and len(sections["LRSC"]) == 104
    assert (info["has_memory"], info["has_per"], info["has_loss_scale"]) == (1, 1, 1)
    d.close()


@pytest.mark.parametrize("n_user", [0, 5, 4097])
def test_user_section(pkg, gpu, tmp_path, n_user):
    d = _make(pkg)
    user = bytes(np.random.default_rng(n_user).integers(0, 256, n_user, dtype=np.uint8))
    _pair(pkg, d, tmp_path, user=user)
    assert pkg.state_user(str(tmp_path / "p1.learnerstate")) == user
    d.close()


def test_image_is_frozen_at_the_call(pkg, gpu, tmp_path):
    """consistency: what is enqueued behind the asynchronous call — appends that overwrite every slot, updates — is not in the file"""
    d = _make(pkg, cap=96, fill=130, use_graph=True)
    p0, p1 = str(tmp_path / "p0.learnerstate"), str(tmp_path / "p1.learnerstate")
    d.save_state(p0)
    d.save_state(p1, wait=False)
    for k in range(3):                                       # without waiting: every slot of the window is overwritten ...
        d.add_transitions_arrays(*_replay(58, 41 + k, 48))
    d.update_async_n(16)                                     # ... and every arena moves
    d.save_state_wait()
    assert _read(p1) == _read(p0)
    p2 = str(tmp_path / "p2.learnerstate")
    d.save_state(p2)
    assert _read(p2) != _read(p0)                            # (the learner did move on)
    d.close()


@pytest.mark.parametrize("per", [None, dict(alpha=0.6, beta0=0.4, beta_anneal_iters=20)], ids=["uniform", "prioritized"])
def test_saving_does_not_perturb_training(pkg, gpu, tmp_path, per):
    a, b = (_make(pkg, cap=200, fill=260, per=per, use_graph=True) for _ in range(2))
    for k in range(3):
        a.save_state(str(tmp_path / ("s%d.learnerstate" % k)), wait=False)
        for d in (a, b):
            d.update_async_n(4)
            d.add_transitions_arrays(*_replay(58, 50 + k, 30))
    a.save_state_wait()
    _same(_bits(a), _bits(b), "saver against its twin that never saves")
    for k in range(3):
        assert pkg.state_info(str(tmp_path / ("s%d.learnerstate" % k)))["actor_iter"] == 3 + 4 * k
    a.close(); b.close()


def test_resume_from_the_asynchronous_file(pkg, gpu, tmp_path):
    p1 = str(tmp_path / "p1.learnerstate")
    a = _make(pkg, cap=200, fill=260, use_graph=True)
    b = _make(pkg, cap=200, fill=100, seed=11, use_graph=True)
    a.save_state(p1, wait=False)
    a.update_async_n(7)
    a.save_state_wait()
    b.load_state(p1)
    b.update_async_n(7)
    _same(_bits(b), _bits(a), "resumed from the asynchronous file")
    a.close(); b.close()


def test_wait_poll_and_a_second_save(pkg, gpu, tmp_path):
    d = _make(pkg)
    d.save_state_wait()                                      # nothing in flight: 0
    assert d.save_state_done() is True
    p0, p1, p2 = (str(tmp_path / n) for n in ("p0", "p1", "p2"))
    d.save_state(p0)
    d.save_state(p1, wait=False)
    assert d.save_state_done() in (True, False)              # never blocks, either answer is right here
    d.save_state(p2, wait=False)                             # joins the first
    assert os.path.exists(p1) and _read(p1) == _read(p0)
    d.save_state_wait()
    assert d.save_state_done() is True
    assert _read(p2) == _read(p0)
    for p in (p1, p2):
        assert pkg.state_info(p)["file_bytes"] == os.path.getsize(p)
    # the synchronous save and the load join a save in flight as well
    p3, p4 = str(tmp_path / "p3"), str(tmp_path / "p4")
    d.save_state(p3, wait=False)
    d.save_state(p4)
    assert d.save_state_done() is True and _read(p3) == _read(p4) == _read(p0)
    d.save_state(p3, wait=False)
    d.load_state(p0)
    assert d.save_state_done() is True and _read(p3) == _read(p0)
    d.close()


def test_close_with_a_save_in_flight_leaves_a_complete_file(pkg, gpu, tmp_path):
    d = _make(pkg, cap=5000, fill=5200)
    p0, p1 = str(tmp_path / "p0"), str(tmp_path / "p1")
    d.save_state(p0)
    d.save_state(p1, wait=False)
    d.close()
    assert pkg.state_info(p1)["memory_size"] == 4999 and not os.path.exists(p1 + ".tmp")
    assert _read(p1) == _read(p0)


def test_unwritable_path_fails_at_the_wait(pkg, gpu, tmp_path):
    d = _make(pkg)
    bad = str(tmp_path / "no" / "such" / "dir" / "x.learnerstate")
    d.save_state(bad, wait=False)                            # the call itself has nothing to refuse
    with pytest.raises(pkg.DQNFatal, match="dqnhip_save_state_wait: .*no/such/dir/x.learnerstate"):
        d.save_state_wait()
    assert not os.path.exists(bad + ".tmp") and not os.path.exists(bad)
    d.save_state_wait()                                      # reported once
    before = d.actor_iter()
    d.update_async_n(2)
    assert d.actor_iter() == before + 2
    # a failed save is also reported by the next call that joins it, and that call does not run
    good = str(tmp_path / "good")
    d.save_state(bad, wait=False)
    with pytest.raises(pkg.DQNFatal, match="dqnhip_save_state_async: .*no/such/dir"):
        d.save_state(good, wait=False)
    assert not os.path.exists(good)
    d.save_state(good, wait=False)
    d.save_state_wait()
    assert pkg.state_info(good)["actor_iter"] == before + 2
    d.close()


def test_refusals_of_the_synchronous_call_under_the_new_name(pkg, gpu, tmp_path):
    never = str(tmp_path / "never")

    def refused(d, match):
        with pytest.raises(pkg.DQNFatal, match="dqnhip_save_state_async: .*" + match):
            d.save_state(never, wait=False)
        assert d.save_state_done() is True and not os.path.exists(never) and not os.path.exists(never + ".tmp")

    owner, sharer = _make(pkg, updates=0), _make(pkg, seed=4, updates=0)
    owner.ShareReplayMemory(sharer)
    for d in (owner, sharer):
        refused(d, "shares a replay memory")
    powner, psharer = _make(pkg, updates=0), _make(pkg, seed=4, updates=0)
    powner.ShareParameters(psharer, 1, 1)
    for d in (powner, psharer):
        refused(d, "shares parameters")
    dp = _make(pkg, updates=0, dp_world=2, dp_rank=0)
    refused(dp, "data-parallel")
    ph = _make(pkg)
    ph.update_phase(0)
    refused(ph, "a phased update is in progress")
    ph.update_abort()
    tm = _make(pkg)
    tm.set_kernel_timing(True)
    refused(tm, "kernel timing is on")
    tm.set_kernel_timing(False)
    tm.save_state(never, wait=False)
    tm.save_state_wait()
    assert pkg.state_info(never)["actor_iter"] == 3
    with pytest.raises(pkg.DQNFatal, match="dqnhip_save_state_async: unknown flags"):
        tm._ck(tm.lib.dqnhip_save_state_async(tm.h, os.fsencode(never), 2, None, 0))
    for d in (sharer, owner, psharer, powner, dp, ph, tm):
        d.close()
