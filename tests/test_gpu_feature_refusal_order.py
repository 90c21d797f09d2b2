"""The order in which a call refuses a learner that carries several opt-in features (feature_refuse, csrc/learner_features.hip): lr
policy / weight decay, then prioritized replay, then n-step returns, then target smoothing — the first one enabled is the one named.
A learner with prioritized replay, n-step returns and target smoothing all enabled: dqnhip_update_indexed_n, _phase, _chained and
_pipelined name prioritized replay, and so does dqnhip_dp_init; created with an lr policy, dqnhip_dp_init names the policy.  With
prioritized replay left off the same calls name n-step returns.  Every refused call is entered once and returns before it enqueues
anything.  The expected texts are written out here as the library had them before the refusals got one home.
Shapes (tests/test_gpu_target_smoothing.py's): B = 32, S = 58, hidden 2 x 64, capacity 512."""
import re

import numpy as np
import pytest

from synth import synth_replay

pytestmark = pytest.mark.gpu

B, S, HID, CAP, N = 32, 58, (64, 64), 512, 400
PER = "%s: not available on a learner with prioritized replay (dqnhip_per_enable) in this version"
NSTEP = "%s: not available on a learner with n-step returns (dqnhip_nstep_enable) in this version"
SCHED = ("%s: not available on a learner with lr_policy exp / weight_decay 0 in this version "
         "(single learner, inside an update only, no diagnostics: DESIGN.md 9)")


def _make(pkg, per, **kw):
    d = pkg.DQN(S, minibatch=B, hidden=HID, memory=CAP, seed=3, **kw)
    d.add_transitions_arrays(*synth_replay(np.random.default_rng(5), N, S, mean_len=10))
    if per:
        d.enable_prioritized_replay()
    d.enable_n_step(3)
    d.enable_target_smoothing(sigma_logits=0.3, sigma_params=0.3, clip=0.25, clamp=True, seed=0x5EED5EED77)
    return d


def _refused(pkg, call, text):
    with pytest.raises(pkg.DQNFatal, match=re.escape(text)):
        call()


def _update_entry_points(pkg, d, fmt):
    idx = np.arange(B, dtype=np.int32)
    _refused(pkg, lambda: d.update_indexed_n(np.stack([idx, idx])), fmt % "dqnhip_update_indexed_n")
    _refused(pkg, lambda: d.update_phase(0, idx), fmt % "dqnhip_update_phase")
    _refused(pkg, lambda: d.UpdateActorCriticChained(idx, idx), fmt % "dqnhip_update_chained")
    _refused(pkg, lambda: d.UpdateActorCriticPipelined(idx), fmt % "dqnhip_update_pipelined")


def test_refusals_name_the_first_enabled_feature_in_order(pkg, gpu):
    uid = pkg.DQN.dp_unique_id()
    # prioritized replay, n-step returns and target smoothing: prioritized replay is named
    d = _make(pkg, per=True)
    _update_entry_points(pkg, d, PER)
    _refused(pkg, lambda: d.dp_init(uid), PER % "dqnhip_dp_init")
    d.close()
    # ... created with an lr policy: dqnhip_dp_init names the policy (the update forms do not refuse one: they name the next in the order)
    d = _make(pkg, per=True, lr_policy="exp", lr_gamma=0.5)
    _refused(pkg, lambda: d.dp_init(uid), SCHED % "dqnhip_dp_init")
    _update_entry_points(pkg, d, PER)
    d.close()
    # prioritized replay left off: n-step returns are named
    d = _make(pkg, per=False)
    _update_entry_points(pkg, d, NSTEP)
    _refused(pkg, lambda: d.dp_init(uid), NSTEP % "dqnhip_dp_init")
    d.close()
