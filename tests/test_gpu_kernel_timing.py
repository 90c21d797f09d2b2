"""Timing mode (dqnhip_set_kernel_timing / dqnhip_get_kernel_timing): every timed launcher of the update brackets its own kernel with
the dispatch packet's start / stop events, files the pair under a family name, and launches exactly the kernel an untimed update
launches.  Three small learners, eager (use_graph=False: timed launches are never captured), explicit indices, eight updates each:

  shifted   fp32, 64 rows into three 1024-wide layers: k_dgrad_qtrain, gemm_bwd_seq, gemm_wgrad_tail, k_dqda_head_bwd, the critic's
            first-layer rider (k_adam_soft_fwd1), first_layers_launch, gemm_fwd_lds.  (Three hidden layers, not two: the shifted
            schedule has a gemm_bwd_seq launch for layers L-2 .. 1 only — bwd_is_shifted / tower_backward — so two layers never reach it.)
  pair      fp32, 32 rows into two 128-wide layers: gemm_bwd_pair_direct, gemm_wgrad_narrow_rider, gemm_dgrad_narrow_qrider,
            gemm_fwd_direct, the plain k_adam_soft.  (With DQNHIP_TUNE_SEPARATE_ACTOR_HEAD_BWD: at these shapes plan_of otherwise takes
            k_dqda_head_bwd here too — dqda_head_shape_ok — and no narrow dgrad launch would be reached.)
  fp16      128 rows into two 128-wide layers: hgemm_launch_batch, hgemm_group_db_launch

Reference work covered by these launches: DQN::UpdateActorCritic, src/dqn.cpp:828-972."""
import numpy as np
import pytest

from synth import det_indices, synth_replay

pytestmark = pytest.mark.gpu

FAMILIES = ("gemm_fwd_lds_4x2", "gemm_fwd_lds_2x2", "gemm_fwd_direct", "gemm_dgrad", "gemm_wgrad", "gemm_bwd_pair", "adam",
            "hgemm_fwd", "hgemm_dgrad", "hgemm_wgrad")
UPDATES = 8
N_REPLAY = 2048

# (name, constructor arguments, forms the plan must / must not name, timed launches per update by family)
# The launch counts are a RECORDING of what the library does at these shapes (this test's own printout), not a derivation: a change
# of the launch layer must reproduce them.
CASES = [
    ("shifted_fp32", dict(state_size=58, minibatch=64, hidden=(1024, 1024, 1024)),
     {"bwd_shifted_critic", "bwd_shifted_actor", "q_train_in_dgrad", "dqda_head_bwd", "critic_l0_rides", "first_layers_merged"}, set(),
     {"gemm_fwd_lds_4x2": 4, "gemm_fwd_lds_2x2": 2, "gemm_fwd_direct": 1, "gemm_dgrad": 5, "gemm_wgrad": 2, "gemm_bwd_pair": 2, "adam": 2,
      "hgemm_fwd": 0, "hgemm_dgrad": 0, "hgemm_wgrad": 0}),
    ("pair_fp32", dict(state_size=59, minibatch=32, hidden=(128, 128), tuning_flag="TUNE_SEPARATE_ACTOR_HEAD_BWD"),
     {"critic_l0_rides", "first_layers_merged"}, {"bwd_shifted_critic", "bwd_shifted_actor", "q_train_in_dgrad", "dqda_head_bwd", "fp16"},
     {"gemm_fwd_lds_4x2": 0, "gemm_fwd_lds_2x2": 0, "gemm_fwd_direct": 4, "gemm_dgrad": 2, "gemm_wgrad": 2, "gemm_bwd_pair": 2, "adam": 2,
      "hgemm_fwd": 0, "hgemm_dgrad": 0, "hgemm_wgrad": 0}),
    ("fp16", dict(state_size=58, minibatch=128, hidden=(128, 128), precision="fp16"),
     {"fp16", "head_wgrad_rides_critic", "head_wgrad_rides_actor"}, set(),      # (the riders' carrier: hgemm_group_db_launch)
     {"gemm_fwd_lds_4x2": 0, "gemm_fwd_lds_2x2": 0, "gemm_fwd_direct": 0, "gemm_dgrad": 0, "gemm_wgrad": 0, "gemm_bwd_pair": 0, "adam": 2,
      "hgemm_fwd": 6, "hgemm_dgrad": 3, "hgemm_wgrad": 2}),
]


def _make(pkg, kw):
    kw = dict(kw)
    if "tuning_flag" in kw:
        kw["tuning"] = getattr(pkg.capi, kw.pop("tuning_flag"))
    d = pkg.DQN(memory=4096, seed=3, use_graph=False, **kw)
    d.add_transitions_arrays(*synth_replay(np.random.default_rng(5), N_REPLAY, kw["state_size"]))
    return d


def _bits(d):
    return [d.get_params(net).view(np.uint32) for net in range(4)] + [np.asarray(d.read_stats(), np.float32).view(np.uint32)]


@pytest.mark.parametrize("name,kw,forms_in,forms_out,k_fam", CASES, ids=[c[0] for c in CASES])
def test_timed_updates(pkg, gpu, name, kw, forms_in, forms_out, k_fam):
    idx = det_indices(11, UPDATES + 1, kw["minibatch"], N_REPLAY)
    plain, timed = _make(pkg, kw), _make(pkg, kw)
    plan = timed.update_plan()                       # (before timing goes on: the plan refuses while it is on)
    print(name, plan)
    assert forms_in <= set(plan["forms"]) and not (forms_out & set(plan["forms"])), (name, plan)
    timed.set_kernel_timing(True)
    with pytest.raises(pkg.DQNFatal, match="kernel timing is on"):
        timed.update_plan()
    for u in range(UPDATES):
        plain.UpdateActorCritic(idx[u])
        timed.UpdateActorCritic(idx[u])
    # bit identity: a timed launch runs the same kernel on the same arguments
    for got, want in zip(_bits(timed), _bits(plain)):
        assert np.array_equal(got, want), name
    # counts and durations
    seen = {fam: timed.kernel_timing(fam) for fam in FAMILIES}
    print(name, "launches per update:", {fam: n / UPDATES for fam, (ms, n) in seen.items()})
    print(name, "avg us:", {fam: round(ms * 1e3, 2) for fam, (ms, n) in seen.items() if n})
    for fam, (ms, n) in seen.items():
        assert n == UPDATES * k_fam[fam], (name, fam, n, k_fam[fam])
        if n > 0:
            assert np.isfinite(ms) and ms > 0, (name, fam, ms)
        else:
            assert ms == 0, (name, fam, ms)
    assert 0 < sum(k_fam.values()) <= plan["launches_single"], (name, k_fam, plan)     # the timed launches are a subset of the update's
    # reset, unknown family, recovery
    assert timed.kernel_timing("adam", reset=True)[1] == UPDATES * k_fam["adam"]
    for fam in FAMILIES:
        assert timed.kernel_timing(fam) == (0.0, 0), (name, fam)
    with pytest.raises(pkg.DQNFatal, match="unknown kernel family"):
        timed.kernel_timing("gemm_nonesuch")
    timed.set_kernel_timing(False)
    plain.UpdateActorCritic(idx[UPDATES])
    timed.UpdateActorCritic(idx[UPDATES])
    assert all(np.isfinite(timed.read_stats()))
    for got, want in zip(_bits(timed), _bits(plain)):
        assert np.array_equal(got, want), name
    assert timed.kernel_timing("adam") == (0.0, 0)                 # nothing is recorded while timing is off
    assert timed.update_plan() == plan
    plain.close(); timed.close()
