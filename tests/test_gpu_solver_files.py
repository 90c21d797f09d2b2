"""The files of a learner whose solver is not Adam: the Caffe .solverstate (one history blob per parameter for SGD, Nesterov, AdaGrad
and RMSProp; two — history 1 of every blob, then history 2 of every blob — for AdaDelta and Adam; "Incorrect length of history
blobs." across the two kinds) and the learner-state file (the 16-byte SOLV section behind ADV1, absent from an Adam learner's file;
exact resume; a load across solvers refused before the learner is touched; the asynchronous save equal to the synchronous one byte
for byte)."""
import os
import struct

import numpy as np
import pytest

import caffe_pb
import optimizer_forms_lib as L
import solver_forms_lib as SL
import solver_ref as R
import state_ref

pytestmark = pytest.mark.gpu

CASE = L._case("files", "eager", 32, 59, (64, 64), seed=41, n_updates=6)
INP = L.make_inputs(CASE)
ADAM = dict(actor_lr=1e-5, critic_lr=1e-3, momentum=0.95)
ALL = R.SOLVERS


def _kw(solver):
    return dict(ADAM if solver == "Adam" else SL.HYPER[solver], solver=solver)


def _make(pkg, solver, path=None, **kw):
    d = pkg.DQN(CASE.S, minibatch=CASE.B, hidden=CASE.hidden, memory=2 * L.REPLAY, seed=1, clip_grad=CASE.clip, tau=0.25,
                save_path=str(path) if path else "state/dqn", **dict(_kw(solver), **kw))
    for net in range(4):
        d.set_params(net, INP["w"][net])
    d.add_transitions_arrays(INP["s"], INP["a"], INP["r"], INP["mc"], INP["nx"], INP["term"])
    return d


def _bits(pkg, d):
    return [d.get_params(net).view(np.uint32) for net in range(4)] + [d.get_params(net, k).view(np.uint32) for net in (0, 1) for k in (pkg.KIND_M, pkg.KIND_V)]


def _snapshot(pkg, d, prefix):
    d.Snapshot(snapshot_prefix=str(prefix), remove_old=False, snapshot_memory=False)
    a, c, _ = pkg.FindLatestSnapshot(str(prefix))
    assert a and c
    return {0: a, 1: c}


@pytest.mark.parametrize("solver", ALL)
def test_solverstate_history_and_restore(pkg, gpu, solver, tmp_path):
    d = _make(pkg, solver, tmp_path / "live")
    try:
        for row in INP["idx"][:3]:
            d.UpdateActorCritic(row)
        files = _snapshot(pkg, d, tmp_path / "snap")
        two = solver in R.TWO_HISTORIES
        for net in (0, 1):
            st = caffe_pb.SolverState()
            with open(files[net], "rb") as f:
                st.ParseFromString(f.read())
            lay_blobs = 2 * (len(CASE.hidden) + (2 if net == 0 else 1))
            assert st.iter == 3 and len(st.history) == (2 if two else 1) * lay_blobs, (solver, net, len(st.history))
            flat = lambda hs: np.concatenate([np.asarray(h.data, np.float32) for h in hs])
            np.testing.assert_array_equal(flat(st.history[:lay_blobs]), d.get_params(net, pkg.KIND_M))
            if two:
                np.testing.assert_array_equal(flat(st.history[lay_blobs:]), d.get_params(net, pkg.KIND_V))
                assert d.get_params(net, pkg.KIND_V).any()
        fresh = _make(pkg, solver, tmp_path / "fresh")
        try:
            fresh.RestoreActorSolver(files[0]); fresh.RestoreCriticSolver(files[1])
            assert (fresh.actor_iter(), fresh.critic_iter()) == (3, 3)
            want, got = _bits(pkg, d), _bits(pkg, fresh)
            for i in (0, 1, 4, 5, 6, 7):                               # online weights, history 1 and 2 (the targets are re-cloned on restore)
                assert np.array_equal(want[i], got[i]), (solver, i)
        finally:
            fresh.close()
    finally:
        d.close()


@pytest.mark.parametrize("writer,reader", [("Adam", "SGD"), ("SGD", "Adam"), ("AdaDelta", "RMSProp"), ("Nesterov", "AdaDelta")])
def test_restore_across_history_counts_is_refused(pkg, gpu, writer, reader, tmp_path):
    d = _make(pkg, writer, tmp_path / "live")
    try:
        d.UpdateActorCritic(INP["idx"][0])
        files = _snapshot(pkg, d, tmp_path / "snap")
    finally:
        d.close()
    r = _make(pkg, reader, tmp_path / "reader")
    try:
        before = _bits(pkg, r)
        for net, restore in ((0, r.RestoreActorSolver), (1, r.RestoreCriticSolver)):
            with pytest.raises(pkg.DQNFatal, match="Incorrect length of history blobs."):
                restore(files[net])
        for x, y in zip(before, _bits(pkg, r)):
            assert np.array_equal(x, y)
        assert (r.actor_iter(), r.critic_iter()) == (0, 0)
    finally:
        r.close()


def _sections(path):
    with open(path, "rb") as f:
        data = f.read()
    info, sections = state_ref.read_bytes(data)
    return data, info, sections, [name for name, _, _ in state_ref.layout(data)][2:]


@pytest.mark.parametrize("solver", ["RMSProp", "AdaDelta"])
def test_exact_resume(pkg, gpu, solver, tmp_path):
    path = str(tmp_path / "learner.state")
    a = _make(pkg, solver)
    try:
        for row in INP["idx"][:3]:
            a.UpdateActorCritic(row)
        a.save_state(path)
        want_stats = [a.UpdateActorCritic(row) for row in INP["idx"][3:6]]
        want = _bits(pkg, a)
    finally:
        a.close()
    b = _make(pkg, solver)
    try:
        b.load_state(path)
        assert (b.actor_iter(), b.critic_iter()) == (3, 3)
        got_stats = [b.UpdateActorCritic(row) for row in INP["idx"][3:6]]
        assert np.array_equal(np.asarray(got_stats, np.float32).view(np.uint32), np.asarray(want_stats, np.float32).view(np.uint32))
        for x, y in zip(want, _bits(pkg, b)):
            assert np.array_equal(x, y)
    finally:
        b.close()


@pytest.mark.parametrize("solver", ALL)
def test_solv_section_and_async_save(pkg, gpu, solver, tmp_path):
    sync, asyn = str(tmp_path / "sync.state"), str(tmp_path / "async.state")
    d = _make(pkg, solver)
    try:
        for row in INP["idx"][:2]:
            d.UpdateActorCritic(row)
        d.save_state(sync, user=b"solver files")
        d.save_state(asyn, user=b"solver files", wait=False)
        d.save_state_wait()
        data, info, sections, order = _sections(sync)
        with open(asyn, "rb") as f:
            assert f.read() == data, (solver, "the asynchronous save's file differs from the synchronous one's")
        si = pkg.state_info(sync)
        if solver == "Adam":
            assert "SOLV" not in sections and (si["solver_type"], si["rms_decay"]) == (0, 0.0)
        else:
            assert order[order.index("ADV1") + 1] == "SOLV" and order[order.index("SOLV") + 1] == "DEVS", order
            assert len(sections["SOLV"]) == 16
            st, rho, r0, r1 = struct.unpack("<ifii", sections["SOLV"])
            assert (st, r0, r1) == (R.SOLVERS.index(solver), 0, 0) and rho == np.float32(SL.HYPER[solver].get("rms_decay", 0.99))
            assert si["solver_type"] == st and si["rms_decay"] == rho
        assert info["version"] == 1
        for net in (0, 1):
            np.testing.assert_array_equal(np.frombuffer(sections["ADM%d" % net], "<f4"), d.get_params(net, pkg.KIND_M))
            np.testing.assert_array_equal(np.frombuffer(sections["ADV%d" % net], "<f4"), d.get_params(net, pkg.KIND_V))
    finally:
        d.close()


@pytest.mark.parametrize("writer,reader", [("Adam", "SGD"), ("SGD", "Adam"), ("RMSProp", "AdaGrad")])
def test_load_across_solvers_is_refused(pkg, gpu, writer, reader, tmp_path):
    path = str(tmp_path / "learner.state")
    d = _make(pkg, writer)
    try:
        d.UpdateActorCritic(INP["idx"][0])
        d.save_state(path)
    finally:
        d.close()
    r = _make(pkg, reader)
    try:
        r.UpdateActorCritic(INP["idx"][1])
        before, n = _bits(pkg, r), r.memory_size()
        with pytest.raises(pkg.DQNFatal, match="%s solver.*%s" % (writer, reader)):
            r.load_state(path)
        for x, y in zip(before, _bits(pkg, r)):
            assert np.array_equal(x, y)
        assert (r.actor_iter(), r.critic_iter(), r.memory_size()) == (1, 1, n)
        r.UpdateActorCritic(INP["idx"][2])                             # and goes on training
    finally:
        r.close()
