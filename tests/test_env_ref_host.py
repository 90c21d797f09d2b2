"""The host references of the external env handle (tests/env_ref.py), without a GPU.

Fed OracleEnv's own synthetic state stream — the states it reads back, the status and player-on-ball draws remade by the numpy Philox
twin — HostExternalEnv must reproduce OracleEnv exactly: that pins the twin, the draw-counter rule and the contract's claim that a
terminal step may be given the next episode's first state in the place of the successor state (src/hfo_game.cpp:164-168 zeroes the
deltas).  Beside it: known answers of evaluation_summary, and the Python surface of the feature."""
import math

import numpy as np
import pytest

import env_ref
from oracle import c_oracle, torch_ref


def oracle_pair(S=59, hidden=(128, 64, 64, 64), capacity=20000, seed=1, wscale=10.0):
    rng = np.random.default_rng(seed)
    w = [torch_ref.init_params_np(rng, S, hidden, actor) * wscale for actor in (True, False)]
    out = []
    for _ in range(2):
        orc = c_oracle.Oracle(B=32, S=S, hidden=hidden, capacity=capacity)
        for net in (0, 1):
            orc.set_params(net, w[net]); orc.clone_to_target(net)
        out.append(orc)
    return out


def test_philox_twin_matches_the_oracle():
    L = c_oracle.lib()
    for seed, ctr, lane in ((11, 0, 0), (0xDEADBEEFCAFE, 5, 256 * 63 + 13), (1, (1 << 40) + 3, 77)):
        size = (1 << 31) - 1
        want = L.orc_philox_index(seed, ctr, lane, size)
        got = (int(env_ref.philox_u32(seed, [ctr], [lane])[0]) * size) >> 32
        assert got == want


@pytest.mark.parametrize("eps", [0.0, 0.3])
def test_host_env_reproduces_oracle_env(eps):
    workers, T, unum, seed, p_end, p_goal = 16, 12, 7, 11, 0.08, 0.4
    oa, ob = oracle_pair()
    a = c_oracle.OracleEnv(oa, workers, max_steps=T, unum=unum, p_end=p_end, p_goal=p_goal, seed=seed)
    b = env_ref.HostExternalEnv(ob, workers, a.read()["state"], max_steps=T, unum=unum, seed=seed)
    for step in range(80):
        status, pob = env_ref.synthetic_status_pob(seed, b.g, p_end, p_goal, unum)
        a.step(eps)
        ra = a.read()
        act, args = b.act(eps)
        b.observe(ra["state"], status, pob)
        np.testing.assert_array_equal(act, ra["action"])
        np.testing.assert_array_equal(args[:, 0], ra["arg1"]); np.testing.assert_array_equal(args[:, 1], ra["arg2"])
        np.testing.assert_array_equal(b.reward, ra["reward"])                  # bit for bit
        np.testing.assert_array_equal(b.episode_len(), ra["episode_len"])
    sa, sb = a.stats(), b.stats()
    assert sa[0] == sb[0] == 80 * workers and sa[1] == sb[1] > 100 and sa[3] == sb[3] > 10
    assert abs(sa[2] - sb[2]) < 1e-9
    assert b.truncated > 10                                                    # forced OUT_OF_TIME: the handle's rule, not a draw
    assert [r.status for r in b.records].count(4) == b.truncated
    n = oa.memory_size()
    assert n == ob.memory_size() == sum(r.steps - 1 for r in b.records)         # HFOGameState::steps counts the initial update
    for x, y in zip(oa.read_memory(0, n), ob.read_memory(0, n)):
        np.testing.assert_array_equal(x, y)
    a.close(); oa.close(); ob.close()


def test_no_record_leaves_the_memory_alone():
    oa, ob = oracle_pair()
    first, stream = env_ref.walk_stream(3, 4, 59, 30)
    env = env_ref.HostExternalEnv(ob, 4, first, max_steps=12, record=False)
    for nx, st, pob in stream:
        env.act(0.0); env.observe(nx, st, pob)
    assert ob.memory_size() == 0 and env.n_episodes == len(env.records) > 0
    oa.close(); ob.close()


E = env_ref.Episode


def test_evaluation_summary_known_answers(pkg):
    eps = [E(1.5, 0.0, 10, 2, 0, 3), E(6.5, 5.0, 20, 1, 1, 5), E(2.5, 1.0, 30, 1, 0, 9), E(-0.5, 0.0, 40, 4, 1, 9)]
    s = pkg.evaluation_summary(eps)
    assert s["episodes"] == 4 and s["goals"] == 2 and s["goal_perc"] == 0.5
    assert s["avg_reward"] == 2.5 and s["avg_steps"] == 25.0 and s["success_steps"] == 25.0
    assert math.isclose(s["reward_std"], math.sqrt((1 + 16 + 0 + 9) / 3), rel_tol=1e-15)       # n - 1 divisor (src/dqn_main.cpp:164)
    assert math.isclose(s["steps_std"], math.sqrt(500 / 3), rel_tol=1e-15)
    assert math.isclose(s["success_std"], math.sqrt(50 / 1), rel_tol=1e-15)
    one = pkg.evaluation_summary(eps[:1])                                      # one trial, no goal: the reference divides 0 by 0
    assert one["goal_perc"] == 0.0 and one["avg_reward"] == 1.5 and math.isnan(one["reward_std"]) and math.isnan(one["success_steps"])
    third = pkg.evaluation_summary(eps[:3])
    assert third["goal_perc"] == float(np.float32(2) / np.float32(3))          # goals / float(repeat_games)
    with pytest.raises(ValueError):
        pkg.evaluation_summary([])


def test_external_env_is_exported(pkg):
    assert "ExternalEnv" in pkg.__all__ and "evaluation_summary" in pkg.__all__
    assert issubclass(pkg.ExternalEnv, pkg.EnvFrontEnd)
    for name in ("act", "observe", "act_device", "observe_device", "episodes", "stats", "debug_read", "close"):
        assert callable(getattr(pkg.ExternalEnv, name))
    import ctypes as C
    assert C.sizeof(pkg.capi.EnvEpisode) == 40 and pkg.capi.EnvEpisode.step_index.offset == 32
    assert C.sizeof(pkg.capi.EnvConfig) == 32                                  # dqnhip_env_config keeps its size
    assert pkg.capi.ENV_NO_RECORD == 1
