"""The native learner-state file (dqnhip_save_state / dqnhip_load_state): save, create ANOTHER learner, load, continue is bit-identical
to never having stopped.  Learner A and learner B always start from different seeds (other initial weights, another sampling key)
and B holds a ring of its own, so whatever the file fails to carry shows.  Every assertion on learner state is bit equality.
No reference counterpart: the reference resumes from its three snapshot files (src/dqn_main.cpp:213-220, 268-286) and loses what
they do not hold.  The ring is wrapped with head != 0 in every test: 2048 transitions, then batches that evict."""
import ctypes as C
import os

import numpy as np
import pytest

import state_ref
from synth import det_indices, synth_replay

pytestmark = pytest.mark.gpu

B, S, HID, CAP = 32, 58, (64, 64), 4096
F = np.float32
_cache = {}


def _replay(key, seed, n):
    if key not in _cache:
        _cache[key] = synth_replay(np.random.default_rng(seed), n, S, mean_len=10)
    return _cache[key]


def _fill(d, cap=CAP):
    """2048 transitions, then batches that evict: the window wraps and its head is not slot 0"""
    d.add_transitions_arrays(*_replay("first", 5, 2048))
    for k in range(4):
        d.add_transitions_arrays(*_replay("more%d" % k, 20 + k, 700))
    assert d.memory_size() == cap - 1


def _make(pkg, seed, per=None, fill=True, B=B, hidden=HID, cap=CAP, **kw):
    d = pkg.DQN(S, minibatch=B, hidden=hidden, memory=cap, seed=seed, **kw)
    if fill:
        _fill(d, cap)
    else:                       # a ring of its own: other transitions, another (head, size)
        d.add_transitions_arrays(*_replay("other", 6, 1000))
    if per is not None:
        d.enable_prioritized_replay(**per)
    return d


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint8 if np.asarray(a).dtype == np.uint8 else np.uint32)


def _tree(d):
    st = d.per_state()
    return [_u32(d.per_debug_read("level%d" % k)) for k in range(st["levels"] + 1)] + [_u32(np.array([st["p_max"]], F))]


def _bits(d):
    """everything the issue calls the learner's bits, as a list of (name, array)"""
    out = [("w%d" % net, _u32(d.get_params(net))) for net in range(4)]
    out += [("%s%d" % ("-mv"[kind], net), _u32(d.get_params(net, kind))) for net in (0, 1) for kind in (1, 2)]
    out.append(("iters", np.array([d.actor_iter(), d.critic_iter()])))
    out.append(("stats", _u32(np.asarray(d.read_stats(), F))))
    n = d.memory_size()
    out.append(("memory_size", np.array([n])))
    out += [("mem%d" % i, _u32(a)) for i, a in enumerate(d.read_memory(0, n))]
    out.append(("idx", _u32(d.debug_read("idx"))))
    out.append(("skipped", np.array([d.skipped_steps()])))
    ls = d.loss_scale_state()
    out.append(("loss_scale", _u32(np.array([ls[k] for k in sorted(ls) if k != "mode"], F))))
    st = d.per_state()
    if st["enabled"]:
        out.append(("per_state", np.array([st["size"], st["next_counter"], st["syncs"]], np.int64)))
        out.append(("per_total", _u32(np.array([st["total"], st["p_max"], st["beta_now"]], F))))
        out += [("level%d" % k, t) for k, t in enumerate(_tree(d))]
        out.append(("priorities", _u32(d.per_priorities(0, n))))
    return out


def _same(got, want, what=""):
    assert [n for n, _ in got] == [n for n, _ in want]
    for (name, g), (_, w) in zip(got, want):
        assert g.shape == w.shape and np.array_equal(g, w), (what, name)


def _differ(got, want, name):
    g, w = dict(got)[name], dict(want)[name]
    return g.shape != w.shape or not np.array_equal(g, w)


def _seed_of(d):
    c = type(d.cfg)()
    d._ck(d.lib.dqnhip_get_config(d.h, C.byref(c)))
    return c.seed


def test_device_sampling_fp32(pkg, gpu, tmp_path):
    path = str(tmp_path / "a.learnerstate")
    a, b = _make(pkg, 3, use_graph=True), _make(pkg, 11, fill=False, use_graph=True)
    b.update_async_n(2)                         # B has a history of its own
    assert _differ(_bits(a), _bits(b), "w0") and _differ(_bits(a), _bits(b), "mem0")
    for _ in range(3):
        a.SampleStatesFromMemory(4)
    a.update_async_n(5)
    a.save_state(path, user=b"caller's bytes")
    saved = _bits(a)
    b.load_state(path)
    at_load = _bits(b)
    _same([x for x in at_load if x[0] != "idx"], [x for x in saved if x[0] != "idx"], "at the load point")       # (idx: the last update's intermediates are not saved)
    # the targets are the saved ones, not clones of the online nets
    assert not np.array_equal(dict(at_load)["w0"], dict(at_load)["w2"]) and not np.array_equal(dict(at_load)["w1"], dict(at_load)["w3"])
    assert _seed_of(b) == 3 and b.cfg.seed == 3
    assert pkg.state_user(path) == b"caller's bytes"
    info = pkg.state_info(path)
    assert (info["actor_iter"], info["critic_iter"], info["update_counter"], info["memory_size"], info["has_memory"], info["has_per"]) == (5, 5, 5, CAP - 1, 1, 0)
    # the state-sampling stream continues where A's is
    assert np.array_equal(_u32(a.SampleStatesFromMemory(6)), _u32(b.SampleStatesFromMemory(6)))
    a.update_async_n(7); b.update_async_n(7)
    _same(_bits(b), _bits(a), "after the continuation")
    assert a.actor_iter() == 12
    a.close(); b.close()


def test_prioritized(pkg, gpu, tmp_path):
    path = str(tmp_path / "p.learnerstate")
    per = dict(alpha=0.6, beta0=0.4, beta_anneal_iters=20)
    a, b = _make(pkg, 3, per=per), _make(pkg, 11, per=per, fill=False)
    a.set_per_priorities(0, np.random.default_rng(9).lognormal(0.0, 1.5, CAP - 1).astype(F))
    b.update_async_n(2)
    a.update_async_n(5)
    a.save_state(path)
    tree, saved = _tree(a), _bits(a)
    b.load_state(path)
    for k, (g, w) in enumerate(zip(_tree(b), tree)):
        assert np.array_equal(g, w), ("straight after the load: level / p_max", k)
    _same([x for x in _bits(b) if x[0] != "idx"], [x for x in saved if x[0] != "idx"], "at the load point")
    a.update_async_n(7); b.update_async_n(7)
    _same(_bits(b), _bits(a), "after the continuation")
    # ... and the ring keeps evicting in step: the tree follows the same physical slots
    for d in (a, b):
        d.add_transitions_arrays(*_replay("late", 31, 300))
        d.update_async_n(2)
    _same(_bits(b), _bits(a), "after further evictions")
    a.close(); b.close()


def test_fp16_dynamic_loss_scale(pkg, gpu, tmp_path):
    path = str(tmp_path / "h.learnerstate")
    kw = dict(B=128, hidden=(128, 128), precision="fp16", loss_scale_mode="dynamic", loss_scale_growth_interval=3)
    a, b = _make(pkg, 3, **kw), _make(pkg, 11, fill=False, **kw)
    a.set_loss_scale(2.0 ** -3, 2.0 ** -2)
    a.update_async_n(5)
    a.save_state(path)
    at_save = a.loss_scale_state()
    assert at_save["growths_critic"] >= 1 and pkg.state_info(path)["has_loss_scale"] == 1      # the multipliers moved within the run
    b.load_state(path)
    assert b.loss_scale_state() == at_save
    a.update_async_n(7); b.update_async_n(7)
    assert a.loss_scale_state() == b.loss_scale_state() and a.loss_scale_state() != at_save
    _same(_bits(b), _bits(a), "after the continuation")
    # a static learner ignores the section; a dynamic one whose bounds exclude the multipliers refuses the file
    c = _make(pkg, 11, fill=False, B=128, hidden=(128, 128), precision="fp16")
    c.load_state(path)
    assert c.loss_scale_state()["mult_critic"] == 1.0
    e = _make(pkg, 11, fill=False, loss_scale_min_mult=0.5, **kw)
    before = _bits(e)
    with pytest.raises(pkg.DQNFatal, match="loss-scale multiplier .* is outside"):
        e.load_state(path)
    _same(_bits(e), before)
    for d in (a, b, c, e):
        d.close()


def test_explicit_indices_blocking(pkg, gpu, tmp_path):
    """the drop-in's default path: one blocking UpdateActorCritic(idx) per step"""
    path = str(tmp_path / "e.learnerstate")
    a, b = _make(pkg, 3), _make(pkg, 11, fill=False)
    idx = det_indices(17, 12, B, CAP - 1)
    for u in range(5):
        a.UpdateActorCritic(idx[u])
    a.save_state(path)
    b.load_state(path)
    for u in range(5, 12):
        ra, rb = a.UpdateActorCritic(idx[u]), b.UpdateActorCritic(idx[u])
        assert np.array_equal(_u32(np.asarray(ra, F)), _u32(np.asarray(rb, F))), u
    _same(_bits(b), _bits(a), "after the continuation")
    a.close(); b.close()


def test_without_memory(pkg, gpu, tmp_path):
    path = str(tmp_path / "n.learnerstate")
    a, b = _make(pkg, 3), _make(pkg, 11, fill=False)
    a.update_async_n(5)
    a.save_state(path, memory=False)
    info = pkg.state_info(path)
    assert info["has_memory"] == 0 and info["flags"] == pkg.capi.STATE_NO_MEMORY and info["file_bytes"] < 400000
    mem = lambda bits: [x for x in bits if x[0].startswith("mem")]
    rest = lambda bits: [x for x in bits if not x[0].startswith("mem") and x[0] != "idx"]
    before, want = _bits(b), _bits(a)
    b.load_state(path)
    after = _bits(b)
    _same(mem(after), mem(before), "B's own ring")
    assert b.memory_size() == 1000
    _same(rest(after), rest(want), "parameters and counters")
    a.close(); b.close()


def test_cross_check_through_the_python_reader(pkg, gpu, tmp_path):
    path = str(tmp_path / "x.learnerstate")
    a = _make(pkg, 3, per=dict(alpha=0.6, beta0=0.4, beta_anneal_iters=20))
    a.set_per_priorities(0, np.random.default_rng(9).lognormal(0.0, 1.5, CAP - 1).astype(F))
    a.update_async_n(5)
    a.save_state(path, user=b"u" * 33)
    info, sections = state_ref.read(path)
    f = state_ref.decode(info, sections)
    n = a.memory_size()
    for net in range(4):
        assert np.array_equal(_u32(f["w"][net]), _u32(a.get_params(net))), net
    for net in (0, 1):
        assert np.array_equal(_u32(f["m"][net]), _u32(a.get_params(net, 1))) and np.array_equal(_u32(f["v"][net]), _u32(a.get_params(net, 2))), net
    s, act, r, mc, nx, t = a.read_memory(0, n)
    for name, want in (("states", s), ("actor_out", act), ("rewards", r), ("mc", mc), ("next_states", nx), ("terminal", t)):
        assert f[name].shape == want.shape and np.array_equal(_u32(f[name]), _u32(want)), name
    assert np.array_equal(_u32(f["leaves"]), _u32(a.per_priorities(0, n)))
    st = a.per_state()
    assert f["ring"]["ring_size"] == n == info["memory_size"] and f["ring"]["ring_head"] != 0
    assert (f["per"]["p_max"], f["per"]["syncs"], f["per"]["beta_anneal_iters"]) == (st["p_max"], st["syncs"], 20)
    assert f["dev"]["actor_iter"] == 5 and f["dev"]["update_counter"] == st["next_counter"] == 5 and f["host"]["seed"] == 3
    assert f["user"] == b"u" * 33 and (info["has_memory"], info["has_per"], info["has_loss_scale"]) == (1, 1, 0)
    # and a file the Python writer re-assembles from the same sections is one the library loads
    again = str(tmp_path / "again.learnerstate")
    with open(path, "rb") as fh:
        data = fh.read()
    order = [name for name, _, _ in state_ref.layout(data)[2:]]
    with open(again, "wb") as fh:
        fh.write(state_ref.write_bytes(info, [(name.encode(), sections[name]) for name in order]))
    b = _make(pkg, 11, per=dict(alpha=0.6), fill=False)
    b.load_state(again)
    _same([x for x in _bits(b) if x[0] != "idx"], [x for x in _bits(a) if x[0] != "idx"])
    a.close(); b.close()


def _refused(pkg, d, path, match):
    before = _bits(d)
    with pytest.raises(pkg.DQNFatal, match=match) as e:
        d.load_state(path)
    assert os.path.basename(path) in str(e.value)
    _same(_bits(d), before, match)


def test_refusals_leave_the_learner_untouched(pkg, gpu, tmp_path):
    plain, prio = str(tmp_path / "plain.learnerstate"), str(tmp_path / "prio.learnerstate")
    a = _make(pkg, 3)
    a.update_async_n(3)
    a.save_state(plain, user=b"user section")
    ap = _make(pkg, 3, per=dict(alpha=0.6))
    ap.update_async_n(3)
    ap.save_state(prio)
    b = _make(pkg, 11, fill=False)
    b.update_async_n(2)
    bp = _make(pkg, 11, fill=False, per=dict(alpha=0.7))
    bp.update_async_n(2)
    other_hidden, other_cap = _make(pkg, 11, fill=False, hidden=(64, 128)), _make(pkg, 11, fill=False, cap=2048)
    _refused(pkg, other_hidden, plain, "hidden 64,64.*are not this learner's.*hidden 64,128")
    _refused(pkg, other_cap, plain, "replay capacity 4096 is not this learner's 2048")
    _refused(pkg, b, prio, "the file holds priorities")
    _refused(pkg, bp, plain, "the file holds no priorities")
    _refused(pkg, bp, prio, "alpha 0.6, this learner's alpha is 0.7")
    with open(plain, "rb") as fh:
        data = fh.read()
    bad = str(tmp_path / "bad.learnerstate")
    for name, first, end in state_ref.layout(data):
        if end == first:
            continue
        flipped = bytearray(data)
        flipped[max((first + end) // 2, 12)] ^= 0x01
        with open(bad, "wb") as fh:
            fh.write(bytes(flipped))
        _refused(pkg, b, bad, {"header": "header CRC mismatch", "table": "section table CRC mismatch"}.get(name, "section %s CRC mismatch" % name))
    for cut in (len(data) - 1, len(data) // 2, 100, 0):
        with open(bad, "wb") as fh:
            fh.write(data[:cut])
        _refused(pkg, b, bad, "truncated|bad magic")
    # v1's limits: sharing in either role, data parallelism — save and load alike
    owner, sharer = _make(pkg, 3, fill=False), _make(pkg, 4, fill=False)
    owner.ShareReplayMemory(sharer)
    for d in (owner, sharer):
        _refused(pkg, d, plain, "shares a replay memory")
        with pytest.raises(pkg.DQNFatal, match="dqnhip_save_state: .*shares a replay memory"):
            d.save_state(str(tmp_path / "never"))
    powner, psharer = _make(pkg, 3, fill=False), _make(pkg, 4, fill=False)
    powner.ShareParameters(psharer, 1, 1)
    for d in (powner, psharer):
        _refused(pkg, d, plain, "shares parameters")
    dp = _make(pkg, 3, fill=False, dp_world=2, dp_rank=0)
    _refused(pkg, dp, plain, "data-parallel")
    with pytest.raises(pkg.DQNFatal, match="dqnhip_save_state: .*data-parallel"):
        dp.save_state(str(tmp_path / "never"))
    assert not os.path.exists(str(tmp_path / "never"))
    # a failed save leaves the file that is there intact (<filename>.tmp cannot be created: a directory has its name)
    os.mkdir(plain + ".tmp")
    with pytest.raises(pkg.DQNFatal, match="cannot open .*plain.learnerstate.tmp"):
        a.save_state(plain)
    with open(plain, "rb") as fh:
        assert fh.read() == data
    # ... and the good file still loads
    b.load_state(plain)
    _same([x for x in _bits(b) if x[0] != "idx"], [x for x in _bits(a) if x[0] != "idx"])
    for d in (sharer, owner, psharer, powner, dp, a, ap, b, bp, other_hidden, other_cap):
        d.close()
