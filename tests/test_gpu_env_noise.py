"""Exploration noise of the env front-end (dqnhip_env_set_noise) against tests/noise_ref.py, for the synthetic and the external kind of
handle and for fp32 and fp16 acting.

Per step and worker the test knows the draw counter g (it starts at 1 and moves by 1, or by 2 on a step that ends the episode) and
whether epsilon chose the random row (env_ref.env_u01), so it can check
  * "noise_z" against the reference's draws on the keys (noise seed, g, w 32 + 2 j): every draw equal or one float32 ulp away (the
    device's and numpy's double log / cos may differ in the last bits), and at least 99 % of them bit-equal — a cap, so that the ulp
    allowance cannot hide a wrong key;
  * bit for bit, from the device's own z and the previous state: the next "noise_state" (zero after a step that ends the episode);
  * bit for bit, from "greedy_out" and that state: "actor_out" on greedy steps, GetAction's "action" / "arg1" / "arg2", and after
    the run the action rows of the replay memory; on epsilon-random steps the row is GetRandomActorOutput's, un-noised.
Shapes: S = 58, hidden 2 x 64 (2 x 128 for fp16 acting, whose learner needs multiples of 128), 5 and 64 workers, max_steps 7, 40
steps with an episode end every fifth step on average, so that resets and max_steps truncations happen; replay capacity 512."""
import numpy as np
import pytest

import env_ref
import noise_ref as NR
from oracle import c_oracle, torch_ref

pytestmark = pytest.mark.gpu

S, T, UNUM, STEPS, CAP = 58, 7, 7, 40, 512
ENV_SEED, NOISE_SEED = 11, 0xABCDEF0123
P_END, P_GOAL = 0.2, 0.4
F = np.float32
NOISE = dict(sigma_logits=0.05, sigma_params=0.1, theta=0.15, clamp=True, seed=NOISE_SEED)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def make_dqn(pkg, f16=False, use_graph=False):
    hidden, B = ((128, 128), 128) if f16 else ((64, 64), 32)
    kw = dict(precision="fp16") if f16 else {}
    dqn = pkg.DQN(S, minibatch=B, hidden=hidden, memory=CAP, seed=1, use_graph=use_graph, **kw)
    rng = np.random.default_rng(5)
    for net, actor in ((0, True), (1, False)):
        dqn.set_params(net, torch_ref.init_params_np(rng, S, hidden, actor) * 10)
        dqn.CloneNet(net)
    if f16:
        dqn.set_act_precision("fp16")
    return dqn


class Driver:
    """steps a handle of either kind one step at a time and knows what the device drew"""

    def __init__(self, pkg, dqn, kind, workers):
        self.kind, self.N = kind, workers
        if kind == "synthetic":
            self.env = pkg.EnvFrontEnd(dqn, workers, max_steps=T, unum=UNUM, p_end=P_END, p_goal=P_GOAL, seed=ENV_SEED)
        else:
            first, self.stream = env_ref.walk_stream(3, workers, S, STEPS, unum=UNUM, p_end=P_END)
            self.env = pkg.ExternalEnv(dqn, workers, first, max_steps=T, unum=UNUM, seed=ENV_SEED)
        self.g = np.ones(workers, np.uint64)
        self.len = np.zeros(workers, np.int64)
        self.t = 0

    def step(self, eps):
        """-> (g at the step's start, random-branch mask, ended mask, actor_out the caller was handed or None)"""
        g = self.g.copy()
        rnd = env_ref.env_u01(ENV_SEED, g, np.arange(self.N), 0) < F(eps)
        ao = None
        if self.kind == "synthetic":
            status, _ = env_ref.synthetic_status_pob(ENV_SEED, g, P_END, P_GOAL, UNUM)
            self.env.step(eps)
        else:
            nx, status, pob = self.stream[self.t]
            _, _, ao = self.env.act(eps, actor_out=True)
        ended = (status != 0) | (self.len + 1 >= T)
        self.pending = None if self.kind == "synthetic" else (nx, status, pob)
        self.g += np.where(ended, 2, 1).astype(np.uint64)
        self.len = np.where(ended, 0, self.len + 1)
        self.t += 1
        return g, rnd, ended, ao

    def finish_step(self):
        if self.pending is not None:
            self.env.observe(*self.pending)


def random_rows(g, rnd, N):
    out = np.zeros((N, 10), F)
    for w in np.flatnonzero(rnd):
        out[w] = env_ref.random_actor_output(ENV_SEED, g[w], w)
    return out


@pytest.mark.parametrize("f16", [False, True], ids=["act_fp32", "act_fp16"])
@pytest.mark.parametrize("kind", ["synthetic", "external"])
@pytest.mark.parametrize("workers", [5, 64])
def test_noise_against_the_reference(pkg, gpu, kind, workers, f16):
    dqn = make_dqn(pkg, f16)
    drv = Driver(pkg, dqn, kind, workers)
    env = drv.env
    env.set_noise(**NOISE)
    np.testing.assert_array_equal(bits(env.debug_read("actor_out")), bits(env.debug_read("greedy_out")))      # before the first step
    sig = NR.sigmas(NOISE["sigma_logits"], NOISE["sigma_params"])
    x = np.zeros((workers, 10), F)
    np.testing.assert_array_equal(env.debug_read("noise_state"), x)
    episodes = [[] for _ in range(workers)]
    expected, n_equal, n_draws, n_rnd, n_ended, n_clamped, n_free = [], 0, 0, 0, 0, 0, 0
    for step in range(STEPS):
        eps = 0.5 if step % 2 else 0.0
        g, rnd, ended, ao = drv.step(eps)
        # (the external kind: between act and observe the state is the advanced one; observe zeroes it where the episode ends)
        z = env.debug_read("noise_z")
        d = NR.ulps32(z, NR.row_normals(NOISE_SEED, g, np.arange(workers)))
        assert d.max() <= 1, (step, d.max())
        n_equal += int((d == 0).sum()); n_draws += d.size
        x_new = NR.ou_step(x, NOISE["theta"], sig, z)                      # from the device's own z: bit for bit from here on
        greedy = env.debug_read("greedy_out")
        noisy = NR.apply(greedy, x_new, True)
        chosen = np.where(rnd[:, None], random_rows(g, rnd, workers), noisy)
        if kind == "external":
            np.testing.assert_array_equal(bits(env.debug_read("noise_state")), bits(x_new), err_msg="step %d" % step)
            np.testing.assert_array_equal(bits(ao), bits(chosen), err_msg="step %d" % step)
        drv.finish_step()
        x = np.where(ended[:, None], F(0), x_new)
        np.testing.assert_array_equal(bits(env.debug_read("noise_state")), bits(x), err_msg="step %d" % step)
        np.testing.assert_array_equal(bits(env.debug_read("actor_out")), bits(chosen), err_msg="step %d" % step)
        np.testing.assert_array_equal(bits(env.debug_read("greedy_out")), bits(greedy))
        act, a1, a2 = c_oracle.get_action(chosen)
        np.testing.assert_array_equal(env.debug_read("action").astype(np.int32), act)
        np.testing.assert_array_equal(bits(env.debug_read("arg1")), bits(a1))
        np.testing.assert_array_equal(bits(env.debug_read("arg2")), bits(a2))
        free = NR.apply(greedy, x_new, False)
        n_clamped += int((bits(free) != bits(noisy))[~rnd].sum()); n_free += int((bits(free) == bits(noisy))[~rnd].sum())
        n_rnd += int(rnd.sum()); n_ended += int(ended.sum())
        for w in range(workers):
            episodes[w].append(chosen[w])
            if ended[w]:
                expected += episodes[w]; episodes[w] = []                 # AddTransitions in worker order
    # the run held every case: random and greedy steps, episode ends, noisy values inside their bounds and clamped ones
    assert n_rnd > 0 and n_ended > workers and n_clamped > 0 and n_free > 0
    assert n_equal >= 0.99 * n_draws, (n_equal, n_draws)
    env.stats()
    size = dqn.memory_size()
    assert size == min(len(expected), CAP - 1) > 0
    rows = dqn.read_memory(0, size)[1]
    np.testing.assert_array_equal(bits(rows), bits(np.stack(expected[-size:])))
    env.close(); dqn.close()


def final_state(dqn, env):
    env.stats()
    n = dqn.memory_size()
    mem = dqn.read_memory(0, n)
    return [bits(m) if m.dtype == F else m for m in mem] + [bits(env.debug_read(k)) for k in ("state", "arg1", "arg2", "reward", "action", "episode_len")]


def assert_same(a, b):
    assert len(a) == len(b)
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)


@pytest.mark.parametrize("kind", ["synthetic", "external"])
def test_zero_sigma_without_clamp_is_a_handle_without_noise(pkg, gpu, kind):
    out = []
    for noise in (False, True):
        dqn = make_dqn(pkg)
        drv = Driver(pkg, dqn, kind, 64)
        if noise:
            drv.env.set_noise(sigma_logits=0.0, sigma_params=0.0, theta=0.3, clamp=False, seed=5)
        for step in range(STEPS):
            drv.step(0.5 if step % 2 else 0.0); drv.finish_step()
        out.append(final_state(dqn, drv.env) + [bits(drv.env.debug_read("greedy_out"))])
        drv.env.close(); dqn.close()
    assert_same(out[0], out[1])


@pytest.mark.parametrize("f16", [False, True], ids=["act_fp32", "act_fp16"])
def test_captured_eager_and_twin_handles_agree(pkg, gpu, f16):
    """40 steps as 2 x 16 captured + 8 captured single steps, as 40 eager steps, and once more captured on a second learner: the
    same workers, noise states and replay memory, bit for bit.  Launch counts of the captured steps: those of a handle without noise."""
    out, nodes = [], []
    for use_graph, noise in ((True, True), (False, True), (True, True), (True, False)):
        dqn = make_dqn(pkg, f16, use_graph=use_graph)
        env = pkg.EnvFrontEnd(dqn, 64, max_steps=T, unum=UNUM, p_end=P_END, p_goal=P_GOAL, seed=ENV_SEED)
        if noise:
            env.set_noise(**NOISE)
        if use_graph:
            env.step(0.3, STEPS)
        else:
            for _ in range(STEPS):
                env.step(0.3)
        nodes.append(env.debug_read("graph_nodes"))
        if noise:
            out.append(final_state(dqn, env) + [bits(env.debug_read(k)) for k in ("noise_state", "noise_z", "actor_out", "greedy_out")])
        env.close(); dqn.close()
    assert_same(out[0], out[1]); assert_same(out[0], out[2])
    # a handle that enables nothing launches what it launched: L + 2 launches for a single step at L = 2 (fp16 acting: the same,
    # L tower layers + k_env_step + k_env_flush), 16 (L + 1) + 1 for sixteen with the flush riding in the next first layer (fp16 acting:
    # 16 (L + 2)) — and a handle with noise launches as many
    assert nodes[3] == ((4, 64) if f16 else (4, 49)), nodes
    assert nodes[0] == nodes[2] == nodes[3] and nodes[1] == (0, 0), nodes


def test_switching_noise_drops_the_captured_steps_and_zeroes_the_state(pkg, gpu):
    dqn = make_dqn(pkg, use_graph=True)
    env = pkg.EnvFrontEnd(dqn, 5, max_steps=T, unum=UNUM, p_end=0.0, p_goal=P_GOAL, seed=ENV_SEED)
    env.step(0.0, 1)
    assert env.debug_read("graph_nodes")[0] > 0
    with pytest.raises(pkg.DQNFatal, match="exploration noise is not enabled"):
        env.debug_read("noise_z")
    env.set_noise(**NOISE)
    assert env.debug_read("graph_nodes") == (0, 0)
    env.step(0.0, 2)
    assert np.abs(env.debug_read("noise_state")).min() > 0 and env.debug_read("graph_nodes")[0] > 0
    env.set_noise(**dict(NOISE, theta=1.0))                      # white noise: the state is sigma z
    np.testing.assert_array_equal(env.debug_read("noise_state"), np.zeros((5, 10), F))
    env.step(0.0, 1)
    z = env.debug_read("noise_z")
    np.testing.assert_array_equal(bits(env.debug_read("noise_state")), bits(NR.sigmas(0.05, 0.1) * z))
    env.set_noise(False)
    assert env.debug_read("graph_nodes") == (0, 0)
    with pytest.raises(pkg.DQNFatal, match="exploration noise is not enabled"):
        env.debug_read("noise_state")
    env.close(); dqn.close()


@pytest.mark.parametrize("kw,message", [
    (dict(sigma_params=-0.1), "sigma_params >= 0"), (dict(sigma_logits=float("inf")), "sigma_logits >= 0"),
    (dict(sigma_params=float("nan")), "sigma_params >= 0"), (dict(theta=0.0), "0 < theta <= 1"), (dict(theta=1.01), "0 < theta <= 1")])
def test_refusals(pkg, gpu, kw, message):
    import ctypes as C
    dqn = make_dqn(pkg)
    env = pkg.EnvFrontEnd(dqn, 5, max_steps=T, seed=ENV_SEED)
    with pytest.raises(pkg.DQNFatal, match=message):
        env.set_noise(**kw)
    cfg = pkg.capi.NoiseConfig()
    assert dqn.lib.dqnhip_noise_default_config(C.byref(cfg), pkg.capi.NOISE_EXPLORE) == 0
    assert (cfg.theta, cfg.sigma_params, cfg.sigma_logits, cfg.clamp) == (F(0.15), F(0.1), 0.0, 1)
    cfg.struct_size -= 8
    assert dqn.lib.dqnhip_env_set_noise(env.h, C.byref(cfg)) != 0 and b"struct_size" in dqn.lib.dqnhip_last_error()
    assert dqn.lib.dqnhip_noise_default_config(C.byref(cfg), 7) != 0 and b"unknown purpose" in dqn.lib.dqnhip_last_error()
    env.close(); dqn.close()
