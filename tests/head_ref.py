"""Float64 references and a per-element comparator for the head layers of the update (numpy only).

The head kernels (dqn-hfo_amd/csrc/head_kernels.hip.h, head_fwd_kernels.hip.h and the riders q_head_rider / head_wgrad_rider of
gemm_bodies.hip.h) hold the update's non-GEMM arithmetic.  tests/test_gpu_head_layers.py runs them as the learner launches them,
through dqnhip_update_phase, reads every operand back (`debug_read`, `get_params`) and hands the lot to `check_all` as one dict
("ops").  tests/test_head_ref_host.py hands it `simulate`'s dict instead — a plain float32 numpy evaluation of the same update on the
same case list — and shows that every rule accepts it and rejects the faults the GPU test relies on it to catch.

Rules (u = 2**-24; each holds for EVERY element; s = the sum of the absolute values of the reference's terms, in float64):

    actor_out, actor_target_out, q_train, q_target, q_policy   x.w + b                        (H + 8) u s
    y            the kernel's own sequence on the device's q_target bits                       1 ulp of float32
    dq           float32(q - y) * float32(1 / B) on the device's bits                          1 ulp
    loss         sum (q - y)**2 / 2B                                                           relative (B + 8) u
    dz_c (Step 1)  (dq_r w_k) mask(x_rk)                                                      3 u |ref|, zeros exact
    dz_c (seed)    (-w_k) mask(x_rk) in float32                                               bit-exact
    dq_da        float64 inverting gradients of dxc with actor_out                             4 u |ref|, d == 0 gives exactly 0
    dz_a         (sum_j dA_rj W_jk) mask(x_rk) on the device's dq_da bits                      18 u s
    head dW, db  sum_m dy_mj x_mk, sum_m dy_mj                                                 (B + 8) u s
    act2_1       lrelu(W1 [s', mu'] + b) (first_layers_merged)                                 (kp0 + 8) u s, branch rule of gemm_ref

mask(x) = 1 for x > 0, else float32(0.01).  Every dot-product quantity also gets gemm_ref's tight rule: its max r = |got - ref| / (u s)
may be at most TIGHT_FACTOR times that of the float32 numpy evaluation of the same inputs (measured in the test, against the
reference).  The fp16 learner's dz_* are scaled fp16 panels: hgemm_ref's interval rule, got16 in [rne16(sc (ref - b)), rne16(sc (ref + b))].
"""
import collections

import numpy as np

import gemm_ref as G
import hgemm_ref as HG

U = G.U
SLOPE32 = G.SLOPE32
NA, NP_, NO = 4, 6, 10
F32, F64 = np.float32, np.float64
# src/dqn.cpp:924-957: actions in [-1, 1]; parameters 0 and 4 (columns 4, 8) in [0, 100], the others in [-180, 180]
MN = np.array([-1, -1, -1, -1, 0, -180, -180, -180, 0, -180], F64)
MX = np.array([1, 1, 1, 1, 100, 180, 180, 180, 100, 180], F64)
ZERO_UNITS = (3, 17, -1)          # top-layer units with zero weights and bias: x == 0 exactly, mask 0.01
ZERO_ACTION = 5                   # the critic's first layer ignores this action column: dxc == 0 exactly there
GAMMA, BETA = 0.99, 0.375

# capi.TUNE_* bits (kept as numbers: this module imports nothing of the package)
SEP_SEED, SEP_ACTOR_HEAD, SEP_CRITIC_L0 = 2, 8, 64

Case = collections.namedtuple("Case", "name precision B S hidden tuning want forbid graph loss_scale")


def _case(name, B, hidden, tuning=0, want=(), forbid=(), precision="fp32", graph=False):
    # fp16: the user factor of the static loss scales (ls_c = 16 B f, ls_q = 4096 f, ls_a = 16384 f): 2**-4 keeps the rows scaled by
    # 2**6 inside the fp16 range
    return Case(name, precision, B, 59, tuple(hidden), tuning, tuple(want), tuple(forbid), graph, 0.0625 if precision == "fp16" else 0.0)


_RIDE = ("head_wgrad_rides_critic", "head_wgrad_rides_actor")
_SMALL = _RIDE + ("dqda_head_bwd", "head_seed_fused", "first_layers_merged")
CASES = [
    # k_head_fwd<10> pair launch + L1 epilogue, k_head_q_train writing dZ, k_dqda_head_bwd<false>, head_wgrad_rider
    _case("b32_h128", 32, (64, 128), want=_SMALL, forbid=("q_train_in_dgrad",)),
    _case("b32_h64", 32, (64, 64), want=_SMALL, forbid=("q_train_in_dgrad",)),
    _case("b32_h192", 32, (64, 192), want=_SMALL, forbid=("q_train_in_dgrad",)),
    _case("b32_h320", 32, (64, 320), want=_SMALL, forbid=("q_train_in_dgrad",)),
    # k_head_bwd<10> without dW, k_head_bwd<1> as the seed with q-rider blocks, k_head_fwd without the L1 epilogue; gives dxc
    _case("b32_h128_separate", 32, (64, 128), tuning=SEP_ACTOR_HEAD | SEP_SEED | SEP_CRITIC_L0, want=_RIDE,
          forbid=("dqda_head_bwd", "head_seed_fused", "first_layers_merged", "q_train_in_dgrad")),
    # k_dgrad_qtrain: 64 / 32 pieces per row, one / several dZ_L slices per workgroup
    _case("b32_h1024_qtrain", 32, (1024, 1024), want=_RIDE + ("q_train_in_dgrad", "dqda_head_bwd")),
    _case("b256_h512_qtrain", 256, (1024, 512), want=_RIDE + ("q_train_in_dgrad", "dqda_head_bwd")),
    # H > 1024: un-hoisted weights in k_head_fwd, five strips per lane in k_head_q_train and the riders, five column chunks
    _case("b64_h1280", 64, (64, 1280), want=_SMALL, forbid=("q_train_in_dgrad",)),
    # k_head_fwd_rows<10>, k_head_bwd_big<1> / <10> + k_head_wred
    _case("b1024_h256_big", 1024, (64, 256), want=("head_seed_fused",), forbid=_RIDE + ("dqda_head_bwd", "first_layers_merged")),
    _case("b1024_h256_big_seed", 1024, (64, 256), tuning=SEP_SEED, forbid=_RIDE + ("dqda_head_bwd", "head_seed_fused")),
    _case("b2048_h1280_big_seed", 2048, (64, 1280), tuning=SEP_SEED, forbid=_RIDE + ("dqda_head_bwd", "head_seed_fused")),
    # the actor head no longer rides: k_head_bwd<10> with dW through 16 row chunks and the ticket
    _case("b1408_h128_ticket", 1408, (64, 128), want=("head_wgrad_rides_critic",), forbid=("head_wgrad_rides_actor", "dqda_head_bwd")),
    # fp16 learner
    _case("h16_b128_ride", 128, (256, 128, 128), want=("fp16",) + _RIDE + ("q_train_in_dgrad", "dqda_head_bwd"), precision="fp16"),
    # no carrier: k_head_bwd<1> / <10> on X416 with dZ16, dW through 16 row chunks and the ticket.  (Below 1024 rows every fp16 backward
    # ends in a hgemm_group_db launch that carries the head's dW / db — bwd16_has_carrier — so the form is reached from 1024 rows on a
    # tower top that the bandwidth-tiled pair does not take: H % 256 != 0.)
    _case("h16_b1024_h128_ticket", 1024, (128, 128), want=("fp16",), forbid=_RIDE + ("dqda_head_bwd",), precision="fp16"),
    _case("h16_b1024_big", 1024, (128, 768), want=("fp16",), forbid=_RIDE + ("dqda_head_bwd",), precision="fp16"),
    # the first shape as one captured graph (update_async): what survives a whole update
    _case("b32_h128_graph", 32, (64, 128), want=_SMALL, forbid=("q_train_in_dgrad",), graph=True),
]
CASE_BY_NAME = {c.name: c for c in CASES}


def seed_of(case):
    return 7000 + [c.name for c in CASES].index(case.name if not case.graph else "b32_h128")


def twin_of(case):
    """the same learner with the narrow dgrad + k_head_bwd<10> in place of k_dqda_head_bwd: it materialises dxc"""
    return case._replace(name=case.name + "_twin", tuning=case.tuning | SEP_ACTOR_HEAD, want=(), forbid=("dqda_head_bwd",), graph=False)


def static_scales(case):
    """(critic step, dQ/da pass, actor step) of learner_create.hip"""
    f = case.loss_scale if case.loss_scale > 0 else 1.0
    return 16.0 * case.B * f, 4096.0 * f, 16384.0 * f


# ---- parameters: dense Caffe order, (W [n][k], b [n]) per tower layer, then per head ---------------------------------------------------
def shapes_of(in_dim, hidden, heads):
    out, k = [], in_dim
    for h in hidden:
        out.append((h, k)); k = h
    return out + [(n, k) for n in heads]


def unpack(vec, in_dim, hidden, heads):
    out, off = [], 0
    for n, k in shapes_of(in_dim, hidden, heads):
        W = vec[off:off + n * k].reshape(n, k); off += n * k
        out.append((W, vec[off:off + n])); off += n
    assert off == vec.size, (off, vec.size)
    return out


def pack(layers):
    return np.concatenate([np.concatenate([W.ravel(), b]) for W, b in layers]).astype(F32)


def head_of(vec, in_dim, hidden, actor):
    """(W [n][H], b [n]) of a net's head layers: the actor's two as one [10][H] matrix, as the kernels hold them"""
    p = unpack(vec, in_dim, hidden, (NA, NP_) if actor else (1,))
    L = len(hidden)
    if actor:
        return np.concatenate([p[L][0], p[L + 1][0]]), np.concatenate([p[L][1], p[L + 1][1]])
    return p[L][0], p[L][1]


def make_inputs(case):
    """{"w": [actor, critic, actor_target, critic_target] dense float32, "s", "a", "r", "mc", "nx", "term", "idx"} with the data edges:
    zero top units, a dead action column, mu(s) out of range in columns 1 and 4, terminal rows, transition rows scaled by 2**-6 .. 2**6"""
    rng = np.random.default_rng(seed_of(case))
    S, hid, B = case.S, case.hidden, case.B
    L = len(hid)
    uni = lambda *shape: rng.uniform(-1.0, 1.0, size=shape).astype(F32)

    def net(in_dim, heads, bias):
        layers = []
        for n, k in shapes_of(in_dim, hid, heads):
            layers.append([uni(n, k) * F32(1.5 / np.sqrt(k)), uni(n) * F32(0.25 if bias or len(layers) >= L else 0.0)])
        for z in ZERO_UNITS:
            layers[L - 1][0][z, :] = 0; layers[L - 1][1][z] = 0
        return layers
    # tower biases zero (the tower tops then scale with the rows' powers of two), except in critic_target, whose first layer the target
    # actor's head kernel finishes (act2_1: the bias is part of that rule)
    actor, critic = net(S, (NA, NP_), False), net(S + NO, (1,), False)
    actor_t, critic_t = net(S, (NA, NP_), False), net(S + NO, (1,), True)
    critic[0][0][:, S + ZERO_ACTION] = 0
    actor[L][1][1] = 3.0            # action 1 above its range [-1, 1]
    actor[L + 1][1][0] = -50.0      # parameter 0 (column 4) below its range [0, 100]
    n = B
    sc = G.row_scales(n)[:, None]
    d = {"w": [pack(actor), pack(critic), pack(actor_t), pack(critic_t)]}
    d["s"], d["nx"], d["a"] = uni(n, S) * sc, uni(n, S) * sc, uni(n, NO) * sc
    d["a"][:, ZERO_ACTION] = 0      # ... and never sees a gradient there: the column stays dead through the critic's step
    d["r"], d["mc"] = uni(n), uni(n) * F32(2)
    d["term"] = (rng.random(n) < 0.25).astype(np.uint8)
    d["nx"][d["term"] != 0] = 0     # what the replay memory keeps for a terminal transition's next state
    d["idx"] = rng.integers(0, n, size=B).astype(np.int32)
    assert 0 < d["term"][d["idx"]].sum() < B
    return d


# ---- the float32 numpy evaluation (the yardstick's arithmetic; the host test's stand-in for the kernels) --------------------------------
def mask32(x):
    return np.where(x > 0, F32(1), SLOPE32)


def _tower32(layers, x, L, fp16):
    acts = [x]
    for W, b in layers[:L]:
        x = G.lrelu32((x @ W.T + b[None, :]).astype(F32))
        if fp16:
            x = x.astype(np.float16).astype(F32)
        acts.append(x)
    return acts


def td_target(q_t, r, mc, term, gamma=GAMMA, beta=BETA):
    """k_head_q_train's sequence (src/dqn.cpp:892-900): doubles where the reference has them, rounded to float twice"""
    off = np.where(term != 0, r, (r.astype(F64) + gamma * q_t.astype(F64)).astype(F32)).astype(F32)
    return (beta * mc.astype(F64) + (1 - beta) * off.astype(F64)).astype(F32)


def loss_diff32(q, y, B):
    return ((q - y).astype(F32) * F32(F32(1.0) / F32(B))).astype(F32)


def invert64(dxc, out):
    d, o = dxc.astype(F64), out.astype(F64)
    return np.where(d < 0, d * (MX - o) / (MX - MN), np.where(d > 0, d * (o - MN) / (MX - MN), 0.0))


def invert32(dxc, out, swap_col=None):
    mn, mx = MN.astype(F32), MX.astype(F32)
    up, dn = ((mx - out) / (mx - mn)).astype(F32), ((out - mn) / (mx - mn)).astype(F32)
    if swap_col is not None:
        up, dn = up.copy(), dn.copy()
        up[:, swap_col], dn[:, swap_col] = dn[:, swap_col].copy(), up[:, swap_col].copy()
    return np.where(dxc < 0, dxc * up, np.where(dxc > 0, dxc * dn, F32(0))).astype(F32)


def seq_sum32(a):
    """column sums of a float32 matrix taken row after row in float32"""
    return np.cumsum(a.astype(F32), axis=0, dtype=F32)[-1]


def simulate(case, inp):
    """One update of `case` on `inp` in float32 numpy, as the ops dict check_all reads.  The critic's optimiser step between the two
    phases is replaced by a 2**-10 relative change of its weights (what it does is not the heads' business; zeros stay zero)."""
    S, hid, B = case.S, case.hidden, case.B
    L, fp16 = len(hid), case.precision == "fp16"
    idx = inp["idx"]
    s, nx, a = inp["s"][idx], inp["nx"][idx], inp["a"][idx]
    if fp16:
        s, nx, a = (v.astype(np.float16).astype(F32) for v in (s, nx, a))
    o = {"w0": inp["w"][0], "w1": inp["w"][1], "w2": inp["w"][2], "w3": inp["w"][3], "next_states": nx,
         "reward": inp["r"][idx], "mc": inp["mc"][idx], "term": inp["term"][idx].astype(F32)}
    P = [unpack(inp["w"][0], S, hid, (NA, NP_)), unpack(inp["w"][1], S + NO, hid, (1,)),
         unpack(inp["w"][2], S, hid, (NA, NP_)), unpack(inp["w"][3], S + NO, hid, (1,))]
    head = lambda net: head_of(inp["w"][net], S if net % 2 == 0 else S + NO, hid, net % 2 == 0)
    hdot = lambda x, Wb: (x @ Wb[0].T + Wb[1][None, :]).astype(F32)
    o["act0"] = _tower32(P[2], nx, L, fp16)[L]
    o["act1"] = _tower32(P[0], s, L, fp16)[L]
    o["actor_target_out"], o["actor_out"] = hdot(o["act0"], head(2)), hdot(o["act1"], head(0))
    mu_t, mu = o["actor_target_out"], o["actor_out"]
    if fp16:
        mu_t, mu = mu_t.astype(np.float16).astype(F32), mu.astype(np.float16).astype(F32)
    a2 = _tower32(P[3], np.concatenate([nx, mu_t], 1), L, fp16)
    o["act2"], o["act2_1"] = a2[L], a2[1]
    o["act3"] = _tower32(P[1], np.concatenate([s, a], 1), L, fp16)[L]
    o["q_target"], o["q_train"] = hdot(o["act2"], head(3))[:, 0], hdot(o["act3"], head(1))[:, 0]
    o["y"] = td_target(o["q_target"], o["reward"], o["mc"], o["term"])
    o["dq"] = loss_diff32(o["q_train"], o["y"], B)
    wq = head(1)[0][0]
    dz = ((o["dq"][:, None] * wq[None, :]).astype(F32) * mask32(o["act3"])).astype(F32)
    sc_c, sc_q, sc_a = static_scales(case)
    o["dz_c0"] = (dz * F32(sc_c)).astype(np.float16).astype(F32) if fp16 else dz
    g1 = np.zeros_like(inp["w"][1])
    g1[-(hid[-1] + 1):-1] = (o["dq"][None, :] @ o["act3"]).astype(F32)[0]
    g1[-1] = seq_sum32(o["dq"][:, None])[0]
    o["g1"] = g1
    d = (o["q_train"] - o["y"]).astype(F32)
    o["loss"] = float(F32(seq_sum32((d * d)[:, None])[0] / F32(2 * B)))
    # phase 1
    o["w1_post"] = (inp["w"][1] * F32(1 + 2.0 ** -10)).astype(F32)
    P1 = unpack(o["w1_post"], S + NO, hid, (1,))
    a4 = _tower32(P1, np.concatenate([s, mu], 1), L, fp16)
    o["act4"] = a4[L]
    wq1, bq1 = head_of(o["w1_post"], S + NO, hid, False)
    o["q_policy"] = hdot(a4[L], (wq1, bq1))[:, 0]
    seed = ((-wq1[0])[None, :] * mask32(a4[L])).astype(F32)
    o["dz_c1"] = (seed * F32(sc_q)).astype(np.float16).astype(F32) if fp16 else seed
    g = seed
    for i in range(L - 1, -1, -1):
        g = (g @ P1[i][0]).astype(F32)
        if i > 0:
            g = (g * mask32(a4[i])).astype(F32)
    o["dxc"] = g[:, S:S + NO].copy()
    o["dq_da"] = invert32(o["dxc"], o["actor_out"])
    Wa = head(0)[0]
    dza = ((o["dq_da"] @ Wa).astype(F32) * mask32(o["act1"])).astype(F32)
    o["dz_a"] = (dza * F32(sc_a)).astype(np.float16).astype(F32) if fp16 else dza
    H = hid[-1]
    dW, db = (o["dq_da"].T @ o["act1"]).astype(F32), seq_sum32(o["dq_da"])
    g0 = np.zeros_like(inp["w"][0])
    g0[-(NO * H + NO):] = np.concatenate([dW[:NA].ravel(), db[:NA], dW[NA:].ravel(), db[NA:]])
    o["g0"] = g0
    return o


# ---- the comparator ------------------------------------------------------------------------------------------------------------------------
def _first(bad):
    return tuple(int(x) for x in np.argwhere(np.atleast_2d(bad))[0])


def _elem(tag, name, got, ref, bound, what):
    """|got - ref| <= bound for every element; names the first offender"""
    col = lambda v: np.asarray(v, F64).reshape(-1, 1) if np.ndim(v) == 1 else np.atleast_2d(np.asarray(v, F64))      # a per-row vector is [B][1]
    got2, ref2, b2 = col(got), col(ref), col(bound)
    err = np.abs(got2 - ref2)
    bad = ~(err <= b2)
    if bad.any():
        r, c = _first(bad)
        raise AssertionError(f"{tag} {name}[{r}][{c}] = {got2[r, c]!r}, reference {ref2[r, c]!r}: |diff| {err[r, c]:.3e} > {what} = {b2[r, c]:.3e}; "
                             f"{int(bad.sum())} such elements")
    return err


def _r(err, s):
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(np.atleast_2d(s) > 0, err / (U * np.atleast_2d(s)), 0.0).max())


def _dot_rule(tag, name, got, yard, ref, s, roundings, stats):
    """the derived bound on the kernel's value and on the float32 yardstick, then the tight rule"""
    what = f"({roundings}) u s"
    kr = _r(_elem(tag, name, got, ref, roundings * U * s, what), s)
    yr = _r(_elem(tag + " (float32 numpy yardstick)", name, yard, ref, roundings * U * s, what), s)
    assert kr <= G.TIGHT_FACTOR * yr, (f"tight bound: {tag} {name}: kernel max r = {kr:.3f} > {G.TIGHT_FACTOR} x yardstick max r = {yr:.3f} "
                                       f"(r = |y - ref| / (u s))")
    stats[name] = (kr, yr)


def _ulp_rule(tag, name, got, want32):
    want32 = np.asarray(want32, F32)
    _elem(tag, name, got, want32.astype(F64), np.spacing(np.abs(want32)).astype(F64), "1 ulp")


def _bits_rule(tag, name, got, want32):
    a, b = np.atleast_2d(np.asarray(got, F32)).view(np.uint32), np.atleast_2d(np.asarray(want32, F32)).view(np.uint32)
    bad = a != b
    if bad.any():
        r, c = _first(bad)
        far = int(np.abs(a.astype(np.int64) - b.astype(np.int64))[np.sign(np.atleast_2d(got)) == np.sign(np.atleast_2d(want32))].max())
        raise AssertionError(f"{tag} {name}[{r}][{c}] = {np.atleast_2d(got)[r, c]!r} (bits {int(a[r, c]):#010x}), expected bit for bit "
                             f"{np.atleast_2d(want32)[r, c]!r} ({int(b[r, c]):#010x}); {int(bad.sum())} of {bad.size} elements differ, by at most {far} ulp")


def _dz_rule(tag, name, got, ref, bound, fp16, sc, what):
    """a tower-top gradient: float32 within the bound, or the scaled fp16 panel inside the interval the bound rounds to"""
    if not fp16:
        return _elem(tag, name, got, ref, bound, what)
    bad = ~np.isfinite(got)
    assert not bad.any(), f"{tag} {name}[{_first(bad)[0]}][{_first(bad)[1]}] is not finite in fp16 (scale {sc})"
    HG._interval16(tag, name, np.asarray(got, F32).astype(np.float16), sc * ref, sc * bound, what + ", scaled, rounded to fp16")
    return None


def _fwd_dot(tag, name, got, x, Wb, stats, vec=False):
    W, b = Wb
    x64, W64, b64 = x.astype(F64), W.astype(F64), b.astype(F64)
    ref, s = x64 @ W64.T + b64[None, :], np.abs(x64) @ np.abs(W64).T + np.abs(b64)[None, :]
    yard = (x @ W.T + b[None, :]).astype(F32)
    got = np.asarray(got, F32).reshape(ref.shape) if vec else got
    _dot_rule(tag, name, got, yard, ref, s, x.shape[1] + 8, stats)


def _wgrad(tag, name, g, dy, x, B, in_dim, hidden, actor, stats):
    W, b = head_of(g, in_dim, hidden, actor)
    dy64, x64 = dy.astype(F64), x.astype(F64)
    # db joins dW as one more column: the per-element bound is the same sum over the rows, and the tight rule's maximum is then taken
    # over n (H + 1) elements (the critic's db alone is ONE element: the yardstick's r there is as likely 0 as 2)
    got = np.concatenate([W, b[:, None]], 1)
    yard = np.concatenate([(dy.T @ x).astype(F32), seq_sum32(dy)[:, None]], 1)
    ref = np.concatenate([dy64.T @ x64, dy64.sum(0)[:, None]], 1)
    s = np.concatenate([np.abs(dy64).T @ np.abs(x64), np.abs(dy64).sum(0)[:, None]], 1)
    _dot_rule(tag, name + "_dW|db", got, yard, ref, s, B + 8, stats)


def check_all(case, o, kp0=None, twin=None):
    """Every rule of the module's table on the quantities `o` holds (a quantity that is absent — overwritten before a whole update
    ends — is skipped together with the rules that need it).  twin: the ops of twin_of(case), for a learner whose plan keeps dxc in
    LDS.  Returns {quantity: (kernel max r, yardstick max r)} of the dot-product quantities."""
    tag, S, hid, B = case.name, case.S, case.hidden, case.B
    H, fp16 = hid[-1], case.precision == "fp16"
    sc_c, sc_q, sc_a = static_scales(case) if fp16 else (1.0, 1.0, 1.0)
    stats = {}
    head = lambda key, net: head_of(o[key], S if net % 2 == 0 else S + NO, hid, net % 2 == 0)
    # forward heads
    for name, xk, wk, net in (("actor_target_out", "act0", "w2", 2), ("actor_out", "act1", "w0", 0), ("q_target", "act2", "w3", 3),
                              ("q_train", "act3", "w1", 1), ("q_policy", "act4", "w1_post", 1)):
        if name in o and xk in o:
            _fwd_dot(tag, name, o[name], o[xk], head(wk, net), stats, vec=net % 2 == 1)
    # TD target, loss diff, loss
    _ulp_rule(tag, "y", o["y"], td_target(o["q_target"], o["reward"], o["mc"], o["term"]))
    _ulp_rule(tag, "dq", o["dq"], loss_diff32(o["q_train"], o["y"], B))
    if "loss" in o:
        d = o["q_train"].astype(F64) - o["y"].astype(F64)
        want = (d * d).sum() / (2 * B)
        assert abs(o["loss"] - want) <= (B + 8) * U * want, f"{tag} loss = {o['loss']!r}, reference {want!r}: relative error {abs(o['loss'] - want) / want:.3e} > (B + 8) u"
    # Step(1)'s tower-top gradient and the critic head's own gradients
    if "dz_c0" in o:
        wq = head("w1", 1)[0][0].astype(F64)
        ref = o["dq"].astype(F64)[:, None] * wq[None, :] * mask32(o["act3"]).astype(F64)
        _dz_rule(tag, "dz_c(step1)", o["dz_c0"], ref, 3 * U * np.abs(ref), fp16, sc_c, "3 u |ref|")
    if "g1" in o:
        _wgrad(tag, "critic_head", o["g1"], o["dq"][:, None], o["act3"], B, S + NO, hid, False, stats)
    # the dq = -1 seed
    if "dz_c1" in o:
        wq1 = head("w1_post", 1)[0][0]
        seed = ((-wq1)[None, :] * mask32(o["act4"])).astype(F32)
        if fp16:
            _bits_rule(tag, "dz_c(seed)", o["dz_c1"], (seed * F32(sc_q)).astype(np.float16).astype(F32))
        else:
            _bits_rule(tag, "dz_c(seed)", o["dz_c1"], seed)
    # inverting gradients
    src, deferred = o, None
    if "dxc" not in o:
        assert twin is not None and "dxc" in twin, f"{tag}: dxc is not materialised and no twin was given"
        _bits_rule(tag, "actor_out (against the twin)", o["actor_out"], twin["actor_out"])
        try:
            _bits_rule(tag, "dq_da (against the twin with the separate actor head backward)", o["dq_da"], twin["dq_da"])
        except AssertionError as e:
            deferred = e                  # raised at the end: the rules below read the learner's own dq_da bits and still apply
        src = twin
    ref = invert64(src["dxc"], src["actor_out"])
    _elem(tag, "dq_da", src["dq_da"], ref, 4 * U * np.abs(ref), "4 u |ref|")
    assert (src["dxc"][:, ZERO_ACTION] == 0).all() and (o["dq_da"][:, ZERO_ACTION] == 0).all(), f"{tag}: the dead action column {ZERO_ACTION} carries a gradient"
    # the actor's tower-top gradient and the actor heads' own gradients, from the device's dq_da bits
    dA, dA64 = o["dq_da"], o["dq_da"].astype(F64)
    if "dz_a" in o:
        Wa = head("w0", 0)[0]
        m = mask32(o["act1"])
        ref, s = (dA64 @ Wa.astype(F64)) * m, (np.abs(dA64) @ np.abs(Wa.astype(F64))) * m
        if fp16:
            _dz_rule(tag, "dz_a", o["dz_a"], ref, 18 * U * s, True, sc_a, "18 u s")
        else:
            _dot_rule(tag, "dz_a", o["dz_a"], ((dA @ Wa).astype(F32) * m).astype(F32), ref, s, 18, stats)
    if "g0" in o:
        _wgrad(tag, "actor_head", o["g0"], dA, o["act1"], B, S, hid, True, stats)
        Wg, bg = head("g0", 0)
        assert (Wg[ZERO_ACTION] == 0).all() and bg[ZERO_ACTION] == 0, f"{tag}: head row {ZERO_ACTION} moves although its dQ/da is 0"
    # critic_target's first layer, finished by the target actor's head kernel
    if kp0 is not None and "act2_1" in o:
        W1, b1 = unpack(o["w3"], S + NO, hid, (1,))[0]
        x = np.concatenate([o["next_states"], o["actor_target_out"]], 1)
        x64, W64, b64 = x.astype(F64), W1.astype(F64), b1.astype(F64)
        pre, s = x64 @ W64.T + b64[None, :], np.abs(x64) @ np.abs(W64).T + np.abs(b64)[None, :]
        bound = (kp0 + 8) * U * s
        near = np.abs(pre) <= bound
        stats["act2_1_branch_share"] = float(near.mean())
        assert near.mean() <= G.MAX_BRANCH_SHARE, (tag, "act2_1: elements within the bound of the ReLU kink", float(near.mean()))
        ref = np.where(pre > 0, pre, G.SLOPE * pre)
        other = np.where(pre > 0, G.SLOPE * pre, pre)          # the other branch, for the elements at the kink
        got = o["act2_1"].astype(F64)
        ok = (np.abs(got - ref) <= bound) | (near & (np.abs(got - other) <= bound))
        if not ok.all():
            r, c = _first(~ok)
            raise AssertionError(f"{tag} act2_1[{r}][{c}] = {got[r, c]!r}, reference {ref[r, c]!r}: |diff| {abs(got[r, c] - ref[r, c]):.3e} > "
                                 f"({kp0 + 8}) u s = {bound[r, c]:.3e}; {int((~ok).sum())} such elements")
        yard = G.lrelu32((x @ W1.T + b1[None, :]).astype(F32)).astype(F64)
        far = ~near
        kr, yr = _r(np.abs(got - ref) * far, s), _r(np.abs(yard - ref) * far, s)
        assert kr <= G.TIGHT_FACTOR * yr, f"tight bound: {tag} act2_1: kernel max r = {kr:.3f} > {G.TIGHT_FACTOR} x yardstick max r = {yr:.3f}"
        stats["act2_1"] = (kr, yr)
    if deferred is not None:
        raise deferred
    return stats
