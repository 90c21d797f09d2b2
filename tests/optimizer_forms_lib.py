"""The cases of tests/test_gpu_optimizer_forms.py and their inputs (numpy only: tests/test_adam_ref_host.py runs the same inputs
through the C oracle on the CPU to show that every blob of every case's gradient is large enough for the clip-scale check to see it).

A case is a learner shape + the way its update is run (`mode`):

    eager      UpdateActorCritic(idx)                        graph      the same as one captured graph (use_graph, update_async)
    indexed    update_indexed_n(idx[:k]) for k = 1 .. 4      chained    two UpdateActorCriticChained calls       (both on use_graph learners)
    dp         dp_update on a one-rank group (dp: plain / half / shard)
    shared     a ShareParameters pair, the sharer updates

Weights are He-scaled gaussians with small non-zero biases, so that activations and back-propagated gradients keep their magnitude from
layer to layer and no blob's share of sum g^2 falls below adam_ref.COVER * delta_s; states and actions are uniform in [-1, 1], a quarter
of the transitions terminal; rewards lie in [1, 3] and Monte-Carlo returns in [3, 5], so that q - y has one sign in most rows and the
critic's one head bias — the sum of the loss diffs — does not cancel to a share below that threshold.  Every learner runs WARMUP updates
first: the tested update then has a non-zero m, v history of real gradients and t = WARMUP + 1.
"""
import collections

import numpy as np

import head_ref

F32 = np.float32
NO = 10
WARMUP = 2
REPLAY = 256
SEP_FIRST_LAYER, LATE_GATHER = 32, 128       # capi.TUNE_SEPARATE_FIRST_LAYER, TUNE_LATE_GATHER (this module imports nothing of the package)

Case = collections.namedtuple("Case", "name mode precision B S hidden tuning want forbid clip freq tau dp loss_scale loss_mode n_updates seed")


def _case(name, mode, B, S, hidden, tuning=0, want=(), forbid=(), precision="fp32", clip=0.02, freq=1, tau=0.001, dp=None, loss_scale=0.0,
          loss_mode="static", n_updates=1, seed=0):
    return Case(name, mode, precision, B, S, tuple(hidden), tuning, tuple(want), tuple(forbid), clip, freq, tau, dp, loss_scale, loss_mode,
                n_updates, seed)


def _cases():
    out = []
    # first-layer riders of the critic's optimiser launch: k_adam_soft_fwd1<1> (K = 64), <2> (K = 128); 4 and 12 rider workgroups
    for tag, S, hid in (("k64_4riders", 54, (64, 128)), ("k128_4riders", 59, (64, 128)), ("k128_12riders", 77, (192, 64))):
        out.append(_case("fwd1_%s" % tag, "eager", 32, S, hid, want=("critic_l0_rides",), seed=len(out)))
        out.append(_case("fwd1_%s_graph" % tag, "graph", 32, S, hid, want=("critic_l0_rides",), seed=len(out)))
        out.append(_case("fwd1_%s_separate" % tag, "eager", 32, S, hid, tuning=SEP_FIRST_LAYER, forbid=("critic_l0_rides",), seed=len(out)))
    # multi-update graphs: adam_corr[pos & 1], soft_now[pos & 1]; k_adam_soft_fwd1_gather<1|2> + k_adam_soft_l0, or k_adam_soft_gather
    for tag, S in (("k64", 54), ("k128", 59)):
        out.append(_case("indexed_%s_early" % tag, "indexed", 32, S, (64, 128), want=("critic_l0_rides", "early_gather_l0"), freq=3, tau=0.25,
                         n_updates=4, seed=len(out)))
        out.append(_case("indexed_%s_late" % tag, "indexed", 32, S, (64, 128), tuning=LATE_GATHER, forbid=("early_gather_l0",), freq=3, tau=0.25,
                         n_updates=4, seed=len(out)))
    out.append(_case("chained_k128", "chained", 32, 59, (64, 128), want=("critic_l0_rides", "early_gather_l0"), freq=3, tau=0.25, n_updates=2, seed=len(out)))
    # the 1536-block cap: a second, short and ragged strided round
    out.append(_case("second_round", "eager", 32, 59, (1024, 1024, 512), want=("critic_l0_rides",), seed=len(out)))
    # every plan of head_ref.CASES: head riders, gemm_wgrad_tail, the narrow rider, k_head_bwd_big + k_head_wred, the ticket forms,
    # hgemm_group_db — each must deliver a complete clip norm
    for c in head_ref.CASES:
        out.append(_case("plan_" + c.name, "graph" if c.graph else "eager", c.B, c.S, c.hidden, tuning=c.tuning, want=c.want, forbid=c.forbid,
                         precision=c.precision, loss_scale=c.loss_scale, seed=len(out)))
    # the clip does not rescale: disabled, and a norm below it
    out.append(_case("exact_clip_disabled", "eager", 32, 59, (64, 128), clip=-1.0, seed=len(out)))
    out.append(_case("exact_norm_below_clip", "eager", 32, 59, (64, 128), clip=1e6, seed=len(out)))
    # data parallel, one rank: k_sumsq, k_sumsq_bf16, k_shard_scal
    for dp in ("plain", "half", "shard"):
        out.append(_case("dp_" + dp, "dp", 32, 59, (128, 128), dp=dp, want=("data_parallel",) if dp != "plain" else (), seed=len(out)))
    # a ShareParameters pair: one shared layer of each net
    out.append(_case("shared_prefix", "shared", 32, 59, (64, 128), seed=len(out)))
    # fp16 learner: static and dynamic loss scale, the switch on and off
    out.append(_case("fp16_static", "eager", 128, 59, (256, 128, 128), precision="fp16", want=("fp16",), loss_scale=0.0625, freq=2, tau=0.25,
                     n_updates=2, seed=len(out)))
    out.append(_case("fp16_dynamic", "eager", 128, 59, (256, 128, 128), precision="fp16", want=("fp16",), loss_scale=0.0625, loss_mode="dynamic",
                     freq=2, tau=0.25, n_updates=2, seed=len(out)))
    return out


CASES = _cases()
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)


def net_params(rng, in_dim, hidden, heads):
    """dense Caffe order: He-scaled gaussian weights, biases uniform in [-0.1, 0.1]"""
    parts = []
    for n, k in head_ref.shapes_of(in_dim, hidden, heads):
        parts.append((rng.standard_normal((n, k)) * np.sqrt(2.0 / k)).astype(F32).ravel())
        parts.append(rng.uniform(-0.1, 0.1, n).astype(F32))
    return np.concatenate(parts)


def make_inputs(case):
    """{"w": [actor, critic, actor_target, critic_target], "s", "a", "r", "mc", "nx", "term", "warm": [WARMUP][B], "idx": [n_updates][B]}"""
    rng = np.random.default_rng(9100 + case.seed)
    S, hid, B = case.S, case.hidden, case.B
    w = [net_params(rng, S, hid, (4, 6)), net_params(rng, S + NO, hid, (1,))]
    w += [(x + rng.normal(0, 1e-2, x.size)).astype(F32) for x in w]          # targets a little off their online nets
    uni = lambda *shape: rng.uniform(-1.0, 1.0, size=shape).astype(F32)
    d = {"w": w, "s": uni(REPLAY, S), "nx": uni(REPLAY, S), "a": uni(REPLAY, NO), "r": uni(REPLAY) + F32(2), "mc": uni(REPLAY) + F32(4)}
    d["term"] = (rng.random(REPLAY) < 0.25).astype(np.uint8)
    d["nx"][d["term"] != 0] = 0
    d["warm"] = rng.integers(0, REPLAY, size=(WARMUP, B)).astype(np.int32)
    d["idx"] = rng.integers(0, REPLAY, size=(case.n_updates, B)).astype(np.int32)
    return d
