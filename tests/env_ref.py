"""Host references of the batched env front-end's external kind (include/dqnhip_env.h: dqnhip_env_act / dqnhip_env_observe).

* A numpy Philox-4x32-10 twin of env_u01 (dqn-hfo_amd/csrc/env.hip.h, oracle/dqn_oracle.c): the draws of the synthetic stream a test
  has to make itself when it feeds that stream to an external handle — status, player on ball — and the draw-counter rule (+1 per
  step, +2 on a step that ends an episode).
* HostExternalEnv: the learner side of PlayOneEpisode (src/dqn_main.cpp:97-153) for N workers on caller-supplied states, assembled
  from the oracle's pieces: actor_forward, get_action, GameState.update / reward, label_transitions, Oracle.add_transitions.
* walk_stream: an arbitrary (not the synthetic generator's) state stream: a bounded random walk with valid (sin, cos) pairs and
  kickable flips.
"""
from collections import namedtuple

import numpy as np

from oracle import c_oracle

M32 = np.uint64(0xFFFFFFFF)


def philox_u32(seed, ctr, lane):
    """c[0] of Philox-4x32-10 on counter (ctr lo, ctr hi, lane, 0x9E3779B9), key `seed` — elementwise over ctr / lane arrays"""
    ctr, lane = np.asarray(ctr, np.uint64), np.asarray(lane, np.uint64)
    c0, c1, c2 = ctr & M32, (ctr >> np.uint64(32)) & M32, lane & M32
    c0, c1, c2 = np.broadcast_arrays(c0, c1, c2)
    c3 = np.full(c0.shape, 0x9E3779B9, np.uint64)
    k0, k1 = np.uint64(int(seed) & 0xFFFFFFFF), np.uint64((int(seed) >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0.astype(np.uint32)


def env_u01(seed, g, w, k):
    """env_u01(seed, g, w, k): draw k of worker w at draw counter g, a float32 in [0, 1) on a 2^-24 grid"""
    lane = np.asarray(w, np.int64) * 256 + k
    return (philox_u32(seed, g, lane) >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def synthetic_status_pob(seed, g, p_end, p_goal, unum):
    """what k_env_step draws at per-worker counters g: (status before the max_steps rule, player on ball)"""
    w = np.arange(len(g))
    end = env_u01(seed, g, w, 11) < np.float32(p_end)
    goal = env_u01(seed, g, w, 12) < np.float32(p_goal)
    status = np.where(end, np.where(goal, 1, 2), 0).astype(np.int32)
    pob = np.where(env_u01(seed, g, w, 13) < np.float32(0.5), unum, -1).astype(np.int32)
    return status, pob


def random_actor_output(seed, g, w):
    """GetRandomActorOutput on the env's draws 1..10 (src/dqn.cpp:664-682; each one fmaf on a 24-bit u: exact in float64)"""
    u = env_u01(seed, np.full(10, g, np.uint64), np.full(10, w), 1 + np.arange(10)).astype(np.float64)
    ao = 360.0 * u - 180.0
    ao[:4] = 2.0 * u[:4] - 1.0
    ao[4] = 200.0 * u[4] - 100.0
    ao[8] = 100.0 * u[8]
    return ao.astype(np.float32)


Episode = namedtuple("Episode", "total_reward extrinsic_reward steps status worker step_index")


class HostExternalEnv:
    """The external handle's contract on the CPU oracle `orc` (record=False: nothing reaches its replay memory)."""

    def __init__(self, orc, workers, first_states, max_steps=500, unum=7, seed=1, record=True):
        self.orc, self.N, self.T, self.unum, self.seed, self.record = orc, workers, max_steps, unum, seed, record
        self.cur = np.array(first_states, np.float32).reshape(workers, orc.S)
        self.game = [self._new_game(self.cur[w]) for w in range(workers)]
        self.g = np.ones(workers, np.uint64)               # where the synthetic handle's counter stands after its reset
        self.ep = [[] for _ in range(workers)]             # open episode: (state, actor output, reward)
        self.pending = [None] * workers
        self.observes = 0
        self.records = []
        self.n_steps = self.n_episodes = self.n_goals = 0
        self.reward_sum = 0.0
        self.truncated = self.goals_own = self.goals_other = self.kickable_rewards = 0
        self.action = self.args = self.reward = None

    def _new_game(self, first_state):
        g = c_oracle.GameState(self.unum)
        g.update(first_state, 0, 0)                        # after the forced DASH(0,0), src/dqn_main.cpp:103-105
        return g

    def episode_len(self):
        return np.array([len(e) for e in self.ep], np.int32)

    def act(self, epsilon):
        assert all(p is None for p in self.pending), "act twice"
        ao = self.orc.actor_forward(self.cur)
        w = np.arange(self.N)
        rnd = env_u01(self.seed, self.g, w, 0) < np.float32(epsilon)
        for i in np.flatnonzero(rnd):
            ao[i] = random_actor_output(self.seed, self.g[i], i)
        act, a1, a2 = c_oracle.get_action(ao)
        self.pending = [(self.cur[i].copy(), ao[i].copy()) for i in range(self.N)]
        self.action, self.args, self.actor_out = act, np.stack([a1, a2], 1), ao
        return act, self.args

    def observe(self, next_states, status, pob):
        assert all(p is not None for p in self.pending), "observe without act"
        self.observes += 1
        nx = np.asarray(next_states, np.float32).reshape(self.N, self.orc.S)
        self.reward = np.zeros(self.N, np.float32)
        for w in range(self.N):
            st = int(status[w])
            assert 0 <= st <= 4
            if st == 0 and len(self.ep[w]) + 1 >= self.T:
                st = 4; self.truncated += 1
            game = self.game[w]
            had_kick = game.g.got_kickable_reward
            game.update(nx[w], st, int(pob[w]))
            r = np.float32(game.reward())
            self.kickable_rewards += int(game.g.got_kickable_reward and not had_kick)
            s, a = self.pending[w]
            self.ep[w].append((s, a, r))
            self.reward[w] = r
            self.n_steps += 1; self.reward_sum += float(r)
            if st == 1:
                self.n_goals += 1
                if int(pob[w]) == self.unum:
                    self.goals_own += 1
                else:
                    self.goals_other += 1
            if st != 0:
                self.records.append(Episode(game.g.total_reward, game.g.extrinsic_reward, game.g.steps, st, w, self.observes))
                self.n_episodes += 1
                if self.record:
                    self._add_episode(self.ep[w])
                self.ep[w] = []
                self.game[w] = self._new_game(nx[w])       # the row is the first state of the worker's next episode
                self.g[w] += np.uint64(2)
            else:
                self.g[w] += np.uint64(1)
        self.cur = nx.copy()
        self.pending = [None] * self.N

    def _add_episode(self, ep):
        s = np.stack([t[0] for t in ep]); a = np.stack([t[1] for t in ep]); r = np.array([t[2] for t in ep], np.float32)
        mc = c_oracle.label_transitions(self.orc.cfg.gamma, r)
        nx = np.zeros_like(s); nx[:-1] = s[1:]             # the terminal transition has no next state
        term = np.zeros(len(ep), np.uint8); term[-1] = 1
        self.orc.add_transitions(s, a, r, mc, nx, term)

    def stats(self):
        return self.n_steps, self.n_episodes, self.reward_sum, self.n_goals


def walk_first_states(rng, n, S):
    s = rng.uniform(-1, 1, size=(n, S)).astype(np.float32)
    s[:, 12] = -1.0                                        # not kickable at kick-off: a later flip to +1 earns the kickable reward
    s[:, 54] = rng.choice([-1.0, 1.0], size=n)
    for i, j in ((13, 14), (51, 52)):
        th = rng.uniform(-np.pi, np.pi, size=n)
        s[:, i] = np.sin(th); s[:, j] = np.cos(th)
    return s


def walk_step(rng, cur, status, p_flip=0.15):
    """The rows the workers show next: a clipped random-walk step of the current row (angles walk too, kickable flips with p_flip)
    where status is IN_GAME, a fresh first state where the episode ended."""
    n, S = cur.shape
    nx = np.clip(cur + rng.normal(0, 0.1, size=cur.shape), -1, 1).astype(np.float32)
    flip = rng.uniform(size=n) < p_flip
    nx[:, 12] = np.where(flip, -cur[:, 12], cur[:, 12])
    nx[:, 54] = cur[:, 54]
    for i, j in ((13, 14), (51, 52)):
        th = np.arctan2(cur[:, i], cur[:, j]) + rng.normal(0, 0.3, size=n)
        nx[:, i] = np.sin(th); nx[:, j] = np.cos(th)
    first = walk_first_states(rng, n, S)
    over = np.asarray(status) != 0
    nx[over] = first[over]
    return nx


def walk_stream(seed, workers, S, steps, unum=7, p_end=0.08, p_goal=0.5):
    """-> first states and, per step, (next_states, status, player_on_ball): the whole stream is decided up front, as a recorded
    simulator's would be (it does not depend on the actions)."""
    rng = np.random.default_rng(seed)
    cur = walk_first_states(rng, workers, S)
    first, out = cur.copy(), []
    for _ in range(steps):
        end = rng.uniform(size=workers) < p_end
        status = np.where(end, np.where(rng.uniform(size=workers) < p_goal, 1, rng.choice([2, 3], size=workers)), 0).astype(np.int32)
        pob = rng.choice([unum, -1, 3], size=workers).astype(np.int32)
        cur = walk_step(rng, cur, status)
        out.append((cur.copy(), status, pob))
    return first, out
