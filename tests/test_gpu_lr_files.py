"""The files of a learner with an lr policy or a weight decay.  The Caffe .solverstate carries current_step for `step` and `multistep`
— what GetLearningRate last left: the count at iteration iter - 1, 0 at iteration 0 and under every other policy — and restore ignores
it (the schedule is stateless).  The learner-state file gets one 104-byte LRSC section (the schedule's words, the decay, its kind)
behind ADV1 / SOLV, written by the synchronous and the asynchronous save alike; a fixed learner without decay writes none and its file
is, byte for byte, what the independent writer of the format (tests/state_ref.py) makes of its sections; save, destroy, create, load,
continue is bit-identical; a load across a mismatch of schedule or decay is refused in both directions, before the learner is touched."""
import struct

import numpy as np
import pytest

import caffe_pb
import optimizer_forms_lib as L
import sched_forms_lib as SF
import sched_ref as SR
import state_ref

pytestmark = pytest.mark.gpu

CASE = L._case("lrfiles", "eager", 32, 59, (64, 64), seed=43, n_updates=6)
INP = L.make_inputs(CASE)
EXP = SR.schedule("exp", gamma=0.5)


def _make(pkg, solver="Adam", sched=SR.FIXED, decay=0.0, kind="L2", path=None, **kw):
    args = dict(SF.HYPER[solver], solver=solver, **SR.dqn_kwargs(sched, decay, kind))
    args.update(kw)
    d = pkg.DQN(CASE.S, minibatch=CASE.B, hidden=CASE.hidden, memory=2 * L.REPLAY, seed=1, clip_grad=CASE.clip, tau=0.25,
                save_path=str(path) if path else "state/dqn", **args)
    for net in range(4):
        d.set_params(net, INP["w"][net])
    d.add_transitions_arrays(INP["s"], INP["a"], INP["r"], INP["mc"], INP["nx"], INP["term"])
    return d


def _bits(pkg, d):
    return [d.get_params(net).view(np.uint32) for net in range(4)] + [d.get_params(net, k).view(np.uint32) for net in (0, 1) for k in (pkg.KIND_M, pkg.KIND_V)]


def _solverstates(pkg, d, prefix):
    d.Snapshot(snapshot_prefix=str(prefix), remove_old=False, snapshot_memory=False)
    # (named directly: FindLatestSnapshot does not report a snapshot taken at iteration 0)
    a, c = "%s_actor_iter_%d.solverstate" % (prefix, d.actor_iter()), "%s_critic_iter_%d.solverstate" % (prefix, d.critic_iter())
    out = {}
    for net, f in ((0, a), (1, c)):
        st = caffe_pb.SolverState()
        with open(f, "rb") as fh:
            st.ParseFromString(fh.read())
        out[net] = st
    return out, {0: a, 1: c}


@pytest.mark.parametrize("sched", [SR.schedule("step", gamma=0.5, stepsize=2), SR.schedule("multistep", gamma=0.5, stepvalues=(1, 2, 4)),
                                   EXP, SR.FIXED], ids=["step", "multistep", "exp", "fixed"])
def test_solverstate_current_step(pkg, gpu, sched, tmp_path):
    d = _make(pkg, sched=sched, path=tmp_path / "live")
    try:
        for n in range(0, 6):
            if n in (0, 1, 3, 5):
                states, files = _solverstates(pkg, d, tmp_path / ("snap%d" % n))
                want = SR.current_step(sched, n - 1) if n > 0 else 0
                for net in (0, 1):
                    assert states[net].iter == n and states[net].current_step == want, (sched.policy, n, net, states[net].current_step, want)
            d.UpdateActorCritic(INP["idx"][n])
        assert SR.current_step(SR.schedule("step", gamma=0.5, stepsize=2), 4) == 2 and SR.current_step(SR.schedule("multistep", gamma=0.5, stepvalues=(1, 2, 4)), 4) == 3
        # restore ignores the field: a second learner continues at the restored iteration's rate
        fresh = _make(pkg, sched=sched, path=tmp_path / "fresh")
        try:
            fresh.RestoreActorSolver(files[0]); fresh.RestoreCriticSolver(files[1])
            assert (fresh.actor_iter(), fresh.critic_iter()) == (5, 5)
            for net in (0, 1):
                base = SF.HYPER["Adam"]["actor_lr" if net == 0 else "critic_lr"]
                assert SR.ulps32(np.float32(fresh.learning_rate(net)), SR.rate(sched, base, 5)) <= SR.RATE_ULP
        finally:
            fresh.close()
    finally:
        d.close()


def _sections(path):
    with open(path, "rb") as f:
        data = f.read()
    info, sections = state_ref.read_bytes(data)
    return data, info, sections, [name for name, _, _ in state_ref.layout(data)][2:]


@pytest.mark.parametrize("solver,sched,decay,kind", [("Adam", EXP, 0.0, "L2"), ("Adam", SR.FIXED, 1e-2, "L1"), ("RMSProp", SR.schedule("multistep", gamma=0.1, stepvalues=(2, 4)), 1e-2, "L2")],
                         ids=["adam_exp", "adam_l1", "rmsprop_multistep_l2"])
def test_lrsc_section_exact_resume_sync_and_async(pkg, gpu, solver, sched, decay, kind, tmp_path):
    sync, asyn = str(tmp_path / "sync.state"), str(tmp_path / "async.state")
    a = _make(pkg, solver, sched, decay, kind)
    try:
        for row in INP["idx"][:3]:
            a.UpdateActorCritic(row)
        a.save_state(sync, user=b"lr files")
        a.save_state(asyn, user=b"lr files", wait=False)
        a.save_state_wait()
        data, info, sections, order = _sections(sync)
        with open(asyn, "rb") as f:
            assert f.read() == data, "the asynchronous save's file differs from the synchronous one's"
        prev = "SOLV" if solver != "Adam" else "ADV1"
        assert order[order.index(prev) + 1] == "LRSC" and order[order.index("LRSC") + 1] == "DEVS", order
        assert len(sections["LRSC"]) == 104
        w = struct.unpack("<iffffiii16ifi", sections["LRSC"])
        hp = SF.HYPER[solver]
        assert w[0] == SR.POLICIES.index(sched.policy) and w[1:3] == (np.float32(hp["actor_lr"]), np.float32(hp["critic_lr"]))
        assert w[3:5] == (sched.gamma, sched.power) and w[5:8] == (sched.stepsize, sched.max_iter, len(sched.stepvalues))
        assert w[8:24] == tuple(sched.stepvalues) + (0,) * (16 - len(sched.stepvalues))
        assert w[24] == np.float32(decay) and w[25] == SR.REGULARIZATIONS.index(kind)
        want_stats = [a.UpdateActorCritic(row) for row in INP["idx"][3:6]]
        want = _bits(pkg, a)
    finally:
        a.close()
    for path in (sync, asyn):
        b = _make(pkg, solver, sched, decay, kind)
        try:
            b.load_state(path)
            assert (b.actor_iter(), b.critic_iter()) == (3, 3)
            got_stats = [b.UpdateActorCritic(row) for row in INP["idx"][3:6]]
            assert np.array_equal(np.asarray(got_stats, np.float32).view(np.uint32), np.asarray(want_stats, np.float32).view(np.uint32))
            for x, y in zip(want, _bits(pkg, b)):
                assert np.array_equal(x, y)
        finally:
            b.close()


def test_fixed_learner_writes_the_file_it_always_wrote(pkg, gpu, tmp_path):
    path = str(tmp_path / "fixed.state")
    d = _make(pkg)
    try:
        for row in INP["idx"][:2]:
            d.UpdateActorCritic(row)
        d.save_state(path, user=b"fixed")
        data, info, sections, order = _sections(path)
        assert "LRSC" not in sections and "SOLV" not in sections
        assert order[:10] == ["WGT0", "WGT1", "WGT2", "WGT3", "ADM0", "ADV0", "ADM1", "ADV1", "DEVS", "HOST"], order
        # the format's independent writer, which knows no LRSC, from the sections in file order
        assert state_ref.write_bytes(info, [(name.encode(), sections[name]) for name in order]) == data
        apath = str(tmp_path / "fixed_async.state")
        d.save_state(apath, user=b"fixed", wait=False)
        d.save_state_wait()
        with open(apath, "rb") as f:
            assert f.read() == data
    finally:
        d.close()


MISMATCHES = [
    (dict(sched=EXP), dict(), "lr_policy exp.*lr_policy fixed"),
    (dict(), dict(sched=EXP), "lr_policy fixed.*lr_policy exp"),
    (dict(decay=1e-2), dict(), "weight_decay 0.01.*weight_decay 0"),
    (dict(), dict(decay=1e-2), "weight_decay 0.*weight_decay 0.01"),
    (dict(sched=EXP), dict(sched=SR.schedule("exp", gamma=0.25)), "another parameter of the schedule"),
    (dict(decay=1e-2, kind="L1"), dict(decay=1e-2, kind="L2"), "kind of decay"),
    (dict(sched=SR.schedule("multistep", gamma=0.5, stepvalues=(3, 5))), dict(sched=SR.schedule("multistep", gamma=0.5, stepvalues=(3, 6))), "lr_policy multistep"),
]


@pytest.mark.parametrize("writer,reader,message", MISMATCHES, ids=["exp_to_fixed", "fixed_to_exp", "decay_to_none", "none_to_decay", "gamma", "kind", "stepvalue"])
def test_load_across_a_schedule_mismatch_is_refused(pkg, gpu, writer, reader, message, tmp_path):
    path = str(tmp_path / "learner.state")
    d = _make(pkg, **writer)
    try:
        d.UpdateActorCritic(INP["idx"][0])
        d.save_state(path)
    finally:
        d.close()
    r = _make(pkg, **reader)
    try:
        r.UpdateActorCritic(INP["idx"][1])
        before, n = _bits(pkg, r), r.memory_size()
        with pytest.raises(pkg.DQNFatal, match=message):
            r.load_state(path)
        for x, y in zip(before, _bits(pkg, r)):
            assert np.array_equal(x, y)
        assert (r.actor_iter(), r.critic_iter(), r.memory_size()) == (1, 1, n)
        r.UpdateActorCritic(INP["idx"][2])                             # and goes on training
    finally:
        r.close()
