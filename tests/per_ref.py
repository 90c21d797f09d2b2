"""Prioritized replay restated in numpy, operation for operation where the device computes in float32 (the definitions:
dqn-hfo_amd/csrc/per_kernels.hip.h): Philox-4x32-10, the stratified draw u_j, the radix-64 sum tree with its one summation order,
the Hillis-Steele descent, the window sync; and in float64 what the tests compare within a tolerance: the importance weights and the
write-back.  The check_* functions are what the GPU tests assert with: each raises AssertionError on the fault it names
(tests/test_per_ref_host.py shows that they do)."""
import numpy as np

F = np.float32
M32 = np.uint64(0xFFFFFFFF)


# ---- Philox-4x32-10, the library's philox_u32(seed, ctr, lane) (update_bodies.hip.h) -------------------------------------------
def philox_u32(seed, ctr, lanes):
    lanes = np.asarray(lanes, np.uint64)
    c = [np.full(lanes.shape, ctr & 0xFFFFFFFF, np.uint64), np.full(lanes.shape, (ctr >> 32) & 0xFFFFFFFF, np.uint64),
         lanes & M32, np.full(lanes.shape, 0x9E3779B9, np.uint64)]
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & M32]
        k0 = (k0 + 0x9E3779B9) & 0xFFFFFFFF
        k1 = (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c[0].astype(np.uint32)


def draw_u(seed, ctr, B, total):
    """u_j = (((float)j + r_j) * inv_B) * total with r_j = (philox >> 8) * 2^-24: three float32 operations in this order"""
    r = (philox_u32(seed, ctr, np.arange(B)) >> np.uint32(8)).astype(F) * F(1.0 / 16777216.0)
    inv_b = F(1.0) / F(B)
    u = np.arange(B, dtype=F) + r
    u = u * inv_b
    return u * F(total)


# ---- the tree -------------------------------------------------------------------------------------------------------------------
def node_sum(children):
    """[..., 64] float32 -> [...]: v32[i] = c[i] + c[i + 32], v16[i] = v32[i] + v32[i + 16], ... (the halving tree)"""
    v = np.asarray(children, F)
    w = 32
    while w >= 1:
        v = v[..., :w] + v[..., w:2 * w]
        w //= 2
    return v[..., 0]


def level_sizes(cap):
    n = [cap]
    while len(n) == 1 or n[-1] > 1:
        n.append((n[-1] + 63) // 64)
    return n


def pad64(a):
    a = np.asarray(a, F)
    out = np.zeros((len(a) + 63) // 64 * 64, F)
    out[:len(a)] = a
    return out


def build_levels(leaves):
    """every level recomputed from the cap leaves: [leaves, level 1, ..., [total]]"""
    levels = [np.asarray(leaves, F).copy()]
    for n in level_sizes(len(leaves))[1:]:
        levels.append(node_sum(pad64(levels[-1]).reshape(-1, 64))[:n])
    return levels


def hs_scan(c):
    """inclusive Hillis-Steele scan over 64 lanes, offsets 1, 2, 4, 8, 16, 32, float32"""
    p = np.asarray(c, F).copy()
    off = 1
    while off < 64:
        t = p.copy()
        t[off:] = p[off:] + p[:-off]
        p = t
        off *= 2
    return p


def descend(levels, u):
    """one row's walk from the root: (slot, leaf).  child = first lane with prefix > u and a non-zero value, else the last non-zero lane"""
    u = F(u)
    node = 0
    c = None
    for k in range(len(levels) - 2, -1, -1):
        lv = pad64(levels[k])
        ch = lv[node * 64:node * 64 + 64]
        p = hs_scan(ch)
        hit = np.nonzero((p > u) & (ch > 0))[0]
        nz = np.nonzero(ch > 0)[0]
        child = int(hit[0]) if len(hit) else (int(nz[-1]) if len(nz) else 0)
        if child > 0:
            u = F(u - p[child - 1])
        c = ch[child]
        node = node * 64 + child
    return node, c


def sample(levels, seed, ctr, B, head, cap):
    """-> (logical idx, slot, prob, u) of the minibatch on counter ctr"""
    total = levels[-1][0]
    u = draw_u(seed, ctr, B, total)
    slot = np.zeros(B, np.int64)
    prob = np.zeros(B, F)
    for j in range(B):
        s, leaf = descend(levels, u[j])
        slot[j], prob[j] = s, F(leaf) / F(total)
    return (slot - head + cap) % cap, slot, prob, u


# ---- the window sync --------------------------------------------------------------------------------------------------------------
def sync_leaves(leaves, seen, now, p_max):
    """k_per_sync on the leaves: seen / now = (head, size); the evicted slots get 0, the appended ones p_max"""
    cap = len(leaves)
    (hs, ss), (h, s) = seen, now
    e = (h - hs) % cap
    n = s - ss + e
    out = np.asarray(leaves, F).copy()
    li = (np.arange(cap) - h) % cap
    out[li >= s] = 0
    out[(li < s) & (li >= s - n)] = F(p_max)
    return out


# ---- weights and write-back (float64) ------------------------------------------------------------------------------------------------
def beta_now(beta0, anneal, critic_iter):
    return beta0 if anneal <= 0 else min(1.0, beta0 + (1.0 - beta0) * critic_iter / anneal)


def weights(prob, beta):
    p = np.asarray(prob, np.float64)
    return (p.min() / p) ** beta


def write_back(td_abs, eps, alpha):
    return (np.asarray(td_abs, np.float64) + float(eps)) ** alpha


def ulp_distance(got32, want64):
    """|got - float32(want)| in units of the last place of float32(want)"""
    want = np.asarray(want64, np.float64).astype(F)
    return np.abs(np.asarray(got32, F).view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))


# ---- the invariants the GPU tests assert --------------------------------------------------------------------------------------------
def check_tree(levels):
    """every level read back equals the recomputation from the leaves read back, bit for bit"""
    want = build_levels(levels[0])
    assert len(want) == len(levels), (len(want), len(levels))
    for k, (g, w) in enumerate(zip(levels, want)):
        bad = np.nonzero(np.asarray(g, F).view(np.uint32) != w.view(np.uint32))[0]
        assert len(bad) == 0, "level %d: node %d is %r, its children sum to %r (%d stale nodes)" % (k, bad[0], g[bad[0]], w[bad[0]], len(bad))


def check_window(leaves, head, size, total):
    cap = len(leaves)
    li = (np.arange(cap) - head) % cap
    out = np.nonzero((li >= size) & (np.asarray(leaves) != 0))[0]
    assert len(out) == 0, "slot %d lies outside the window [%d, %d + %d) and holds %r" % (out[0], head, head, size, leaves[out[0]])
    assert (total > 0) == (size > 0), (total, size)


def check_fresh(leaves, head, first, n, p_max):
    """the logical range [first, first + n) was appended and never sampled: every leaf is p_max"""
    cap = len(leaves)
    got = np.asarray(leaves, F)[(head + first + np.arange(n)) % cap]
    bad = np.nonzero(got.view(np.uint32) != np.full(n, p_max, F).view(np.uint32))[0]
    assert len(bad) == 0, "logical %d was refilled but holds %r, not p_max = %r" % (first + bad[0], got[bad[0]], p_max)


def check_weights(w, prob, beta, max_ulp):
    d = ulp_distance(w, weights(prob, beta))
    assert d.max() <= max_ulp, "weight %d: %r against (pmin / prob)^beta = %r (%d ulp)" % (d.argmax(), w[d.argmax()], weights(prob, beta)[d.argmax()], d.max())
    return int(d.max())


def check_write_back(leaf, td_abs, eps, alpha, max_ulp):
    d = ulp_distance(leaf, write_back(td_abs, eps, alpha))
    assert d.max() <= max_ulp, "leaf %d: %r against (|td| + eps)^alpha = %r (%d ulp)" % (d.argmax(), leaf[d.argmax()], write_back(td_abs, eps, alpha)[d.argmax()], d.max())
    return int(d.max())


def check_sample(levels, slot, prob):
    leaves = np.asarray(levels[0], F)
    got = leaves[np.asarray(slot, np.int64)]
    assert (got > 0).all(), "row %d drew slot %d, whose priority is zero" % (np.argmin(got > 0), slot[np.argmin(got > 0)])
    want = got / F(levels[-1][0])
    assert np.array_equal(np.asarray(prob, F).view(np.uint32), want.view(np.uint32)), "prob != leaf / total"
