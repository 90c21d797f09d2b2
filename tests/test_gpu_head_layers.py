"""Every head-layer launch of the update, element by element against float64 (rules and references: tests/head_ref.py).

Each case is a learner at the smallest shape that takes one launch form — asserted on `update_plan()["forms"]`, so that a later change
to plan_of turns the case red instead of silently testing another kernel — with weights from `set_params` and transitions from
`add_transitions_arrays`.  It runs update_phase(0, idx), reads back, runs update_phase(1), reads back, runs phase 2.  Every kernel
runs exactly as the learner launches it; the references are float64 numpy on the operand bits the device itself holds (`act<p>_<L>`,
`actor_out`, `actor_target_out`, `dq`, `dq_da`, `dxc`, `q_*`) and on `get_params` taken at the time the kernel ran (actor: pre-step in
phase 1; critic: post-step for q_policy and the seed).

Data edges, in every case (head_ref.make_inputs): top-layer units with zero weights and bias (x == 0 exactly: mask 0.01), one action
column the critic's first layer ignores (dxc == 0 exactly: dq_da 0, the head row does not move), mu(s) pushed out of its range in
columns 1 and 4 (inversion factor negative / above 1), terminal and bootstrapping rows, beta = 0.375, transition rows scaled by
2**-6 .. 2**6.  act2_1 (first_layers_merged) is compared on ALL rows: the gather copies the stored next state into the panel
whether or not the transition is terminal (gather_block), and what the replay memory stores for a terminal transition is a zero
next state (the add-transitions kernel of io_kernels.hip.h) — the reference reads the stored rows back with `read_memory`.  A learner whose plan has dqda_head_bwd keeps dxc in LDS: its dq_da must
equal, bit for bit, that of a twin built with TUNE_SEPARATE_ACTOR_HEAD_BWD, and the twin's is checked against float64.

The fp16 learner's pair is bit-identical because its separate form runs the fused kernel's own tile in a launch of its own
(DqdaHeadArgs::dxc: k_dqda_head_bwd<true> forms the 16-column dQ/da tile, stores it, and ends; k_head_bwd<10> inverts it).  This
file found the pair apart — the separate form used to be the fp16-MFMA layer-0 dgrad launch, the same exact products added in
another order: 957 of the 1280 elements of dq_da differed, by at most 830 ulp of float32 — and the separate form was changed.

Measured on the MI355X: max r = |got - ref| / (u s) of the kernel / of the float32 numpy yardstick (tight rule: kernel <= 4 x yardstick)

    case                   actor_out  actor_t_out  q_train    q_target   q_policy   dz_a       critic dW|db  actor dW|db  act2_1
    b32_h128               0.73/0.73  0.75/0.67    0.72/0.72  0.51/0.76  0.62/0.45  2.06/2.98  3.42/3.40     5.81/5.81    1.36/2.11
    b32_h64                0.78/0.81  0.68/1.21    0.61/0.74  0.72/0.43  0.39/0.46  2.21/3.27  5.70/5.70     6.30/7.17    1.37/1.89
    b32_h192               0.86/0.86  0.51/0.66    0.43/0.43  0.35/0.29  0.34/0.66  2.28/3.10  2.50/2.50     6.64/6.64    1.63/2.58
    b32_h320               0.62/0.62  0.73/0.73    0.76/0.76  0.39/0.53  0.18/0.46  2.52/3.96  8.10/9.88     9.21/9.21    1.81/2.44
    b32_h128_separate      0.68/0.75  0.70/0.68    0.45/0.65  0.37/0.42  0.43/0.61  1.89/2.54  7.69/7.69     5.95/6.02    -
    b32_h1024_qtrain       0.68/0.63  0.60/0.60    0.14/0.51  0.15/0.47  0.85/1.69  3.52/4.14  6.31/6.31     8.25/7.12    1.88/3.42
    b256_h512_qtrain       0.65/1.41  0.74/1.73    0.55/0.73  0.36/0.73  1.34/2.31  3.30/4.16  5.26/5.26     5.28/19.08   2.82/5.79
    b64_h1280              0.62/0.62  0.53/0.63    0.24/0.44  0.37/0.65  0.28/0.46  2.93/3.41  7.29/4.26     8.23/14.26   1.24/1.55
    b1024_h256_big         0.85/4.90  0.86/3.12    0.54/0.82  0.50/0.84  0.41/0.98  3.12/4.14  2.08/7.34     2.10/15.61   -
    b1024_h256_big_seed    0.93/3.61  0.88/4.29    0.69/0.85  0.55/0.69  0.50/1.00  3.27/3.87  2.35/7.95     2.36/15.00   -
    b2048_h1280_big_seed   0.83/1.94  0.58/1.89    0.52/0.64  0.33/0.75  0.37/0.75  3.75/5.18  1.92/8.81     2.48/21.79   -
    b1408_h128_ticket      1.03/3.59  0.95/3.71    0.71/0.79  0.97/0.98  0.89/0.72  2.98/3.74  2.27/5.38     2.91/23.01   -
    h16_b128_ride          0.89/2.98  0.82/3.03    0.64/0.83  0.66/0.79  0.80/0.87  (fp16)     2.06/2.03     2.46/9.33    -
    h16_b1024_h128_ticket  1.10/4.62  1.22/3.82    0.99/1.14  0.58/0.70  0.65/0.82  (fp16)     2.96/7.55     2.79/13.89   -
    h16_b1024_big          0.77/2.80  0.64/2.32    0.58/0.78  0.38/0.70  0.46/0.85  (fp16)     1.76/11.16    2.29/13.94   -
    b32_h128_graph         0.73/0.73  0.75/0.67    0.72/0.72  0.51/0.76  0.62/0.45  2.06/2.98  -             5.81/5.81    -

(dW|db: the head's db joins its dW as column H, so that the tight rule's maximum is taken over more than the critic's ONE db element;
the yardstick's db is the row-after-row float32 sum.  The whole file: 1.6 s of test calls, no case above 0.3 s.)

The tests bite.  Each of these in-bounds arithmetic edits, made on a scratch copy of the library and never committed, turns cases red
(first element named):

    edit                                                            red cases                                       first finding
    lrelu_mask: y <= 0 -> y < 0                                     all 16                                          b32_h128 dz_c(step1)[0][3] = -0.0, reference -6.68e-06
    k_dqda_head_bwd: inversion factors swapped for column 9         the 8 fused fp32 cases incl. the graph,         b32_h128 dq_da[0][9] against the twin, 32 of 320 elements
                                                                    h16_b128_ride
    k_head_wred: last row chunk left out                            the 3 fp32 *_big cases, h16_b1024_big           b1024_h256_big critic_head_dW|db[0][0] = -1.214, reference -1.481
    k_head_fwd_rows: 4 (t & 1) -> 4 (1 - (t & 1)), weight side      h16_b1024_h128_ticket, h16_b1024_big            h16_b1024_h128_ticket actor_target_out[0][0] = 0.114, reference 0.066
    k_head_q_train: gamma * qt added in float                       the 4 fp32 cases from 1024 rows, the 2 fp16     b1024_h256_big y[97][0] off by 10 ulp, 11 such rows
                                                                    cases from 1024 rows
    head_wgrad_rider: last row group skipped                        the 9 fp32 cases whose head gradients ride,     b32_h128 critic_head_dW|db[0][0]: |diff| 1.0e-06 > 40 u s = 6.9e-07
                                                                    the graph case

(The float gamma * qt edit stays within 1 ulp of y on the minibatches of 32 .. 256 rows and shows from 1024 rows on, where some row's
rounding differs; k_dgrad_qtrain has the same expression in a copy of its own, which the edit did not touch.)
"""
import time

import numpy as np
import pytest

import head_ref as R

pytestmark = pytest.mark.gpu

_twin_ops = {}


def run_case(pkg, case, inp, as_graph=False):
    """the ops dict of head_ref.check_all from one update of a learner of `case`, and its critic first-layer panel width if the merged
    first layers ran"""
    S, B, L = case.S, case.B, len(case.hidden)
    idx = inp["idx"]
    d = pkg.DQN(S, minibatch=B, hidden=case.hidden, memory=max(2 * B, 64), gamma=R.GAMMA, beta=R.BETA, seed=1, precision=case.precision,
                loss_scale=case.loss_scale, tuning=case.tuning, use_graph=as_graph)
    try:
        for net in range(4):
            d.set_params(net, inp["w"][net])
        d.add_transitions_arrays(inp["s"], inp["a"], inp["r"], inp["mc"], inp["nx"], inp["term"])
        forms = d.update_plan()["forms"]
        for f in case.want:
            assert f in forms, (case.name, "the plan no longer takes", f, forms)
        for f in case.forbid:
            assert f not in forms, (case.name, "the plan now takes", f, forms)
        merged, fused = "first_layers_merged" in forms, "dqda_head_bwd" in forms
        o = {"w%d" % n: d.get_params(n) for n in range(4)}
        for n in range(4):
            np.testing.assert_array_equal(o["w%d" % n], inp["w"][n])
        o["reward"], o["mc"] = inp["r"][idx], inp["mc"][idx]
        first = ("actor_out", "actor_target_out", "q_train", "q_target", "y", "dq")
        if as_graph:
            d.update_async(idx)
            o["loss"] = d.read_stats()[0]
            for p in range(5):
                o["act%d" % p] = d.debug_read("act%d_%d" % (p, L))
            for k in first:
                o[k] = d.debug_read(k)
        else:
            d.update_phase(0, idx)
            for p in range(4):
                o["act%d" % p] = d.debug_read("act%d_%d" % (p, L))
            for k in first:
                o[k] = d.debug_read(k)
            o["dz_c0"] = d.debug_read("dz_c")
            o["g1"] = d.get_params(1, pkg.KIND_G)
            if merged:
                o["act2_1"], o["next_states"] = d.debug_read("act2_1"), d.read_memory(0, B)[4][idx]
            d.update_phase(1)
            o["act4"] = d.debug_read("act4_%d" % L)
            np.testing.assert_array_equal(d.debug_read("actor_out"), o["actor_out"])
        o["term"] = d.debug_read("terminal")
        np.testing.assert_array_equal(o["term"], inp["term"][idx].astype(np.float32))
        np.testing.assert_array_equal(d.debug_read("idx").astype(np.int32), idx)
        o["w1_post"] = d.get_params(1)
        assert not np.array_equal(o["w1_post"], o["w1"])
        if not as_graph:
            np.testing.assert_array_equal(d.get_params(0), o["w0"])          # the actor steps in phase 2
        for k, name in (("q_policy", "q_policy"), ("dz_c1", "dz_c"), ("dz_a", "dz_a"), ("dq_da", "dq_da")):
            o[k] = d.debug_read(name)
        o["g0"] = d.get_params(0, pkg.KIND_G)
        if fused:
            with pytest.raises(Exception, match="'dxc'.*never writes it"):
                d.debug_read("dxc")
        else:
            o["dxc"] = d.debug_read("dxc")
        if not as_graph:
            d.update_phase(2)
            o["loss"] = d.read_stats()[0]
        kp0 = (S + R.NO + 63) // 64 * 64 if merged and not as_graph else None
        return o, kp0, fused
    finally:
        d.close()


def twin_ops(pkg, case, inp):
    """the ops of the case's twin with the separate actor head backward (one learner per shape and flag set, shared)"""
    key = (case.precision, case.B, case.hidden, case.tuning)
    if key not in _twin_ops:
        _twin_ops[key] = run_case(pkg, R.twin_of(case), inp)[0]
    return _twin_ops[key]


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_head_layers(pkg, gpu, name):
    case = R.CASE_BY_NAME[name]
    t0 = time.time()
    inp = R.make_inputs(case)
    o, kp0, fused = run_case(pkg, case, inp, as_graph=case.graph)
    twin = twin_ops(pkg, case, inp) if fused else None
    t1 = time.time()
    stats = R.check_all(case, o, kp0=kp0, twin=twin)
    if twin is not None:
        tw = R.twin_of(case)
        R.check_all(tw, twin)
    print("\n%s: device %.2f s, references %.2f s" % (name, t1 - t0, time.time() - t1))
    for k, v in sorted(stats.items()):
        print("   %-22s %s" % (k, "kernel r %.2f  yardstick r %.2f" % v if isinstance(v, tuple) else "%.2e" % v))
    if case.graph:
        # the same learner phase by phase leaves the same bits
        p = run_case(pkg, case._replace(graph=False), inp)[0]
        for k in ("q_target", "q_train", "q_policy", "y", "dq", "actor_out", "dq_da", "dz_a", "dz_c1", "g0", "w1_post"):
            np.testing.assert_array_equal(o[k].view(np.uint32), p[k].view(np.uint32), err_msg=k)
        assert o["loss"] == p["loss"]
