"""numpy restatement of dqn-hfo_amd/csrc/noise_bodies.hip.h: Gaussian noise on an ActorOutput row.

Standard normal draw of the key (seed, ctr, lane0): x1 = philox_u32(seed, ctr, lane0), x2 = philox_u32(seed, ctr, lane0 + 1),
u1 = ((x1 >> 8) + 1) 2^-24 in (0, 1], u2 = (x2 >> 8) 2^-24 in [0, 1), z = float32(sqrt(-2 log u1) cos(6.283185307179586 u2)),
evaluated in float64 and rounded once.  Column j's range is mx - mn of inverting_bounds (2 for the four logits, 100 for the two
powers, 360 for the four angles); its sigma is sigma_logits below column 4 and sigma_params from there; sigmas and clip are in units
of the range.  Everything after the draw is one separately rounded float32 operation per step:
    exploration      x <- (x - theta x) + sigma_j z;  v' = v + range_j x;  clamp: min(max(v', mn), mx)
    target smoothing t = sigma_j z;  clip > 0: t = min(max(t, -clip), clip);  a~ = mu + range_j t;  clamp as above
Exploration keys: (noise seed, the worker's draw counter at the step's start, w 32 + 2 j); the state is zero at creation and after
every episode end, and advances on every step whether or not epsilon chose the random row.
Target smoothing keys: (noise seed, the update's sampling counter, r 32 + 2 j)."""
import numpy as np

from per_ref import philox_u32

F = np.float32
NO, NA = 10, 4
BOUNDS = np.array([(-1.0, 1.0)] * 4 + [(0.0, 100.0), (-180.0, 180.0), (-180.0, 180.0), (-180.0, 180.0), (0.0, 100.0), (-180.0, 180.0)], F)
MN, MX = BOUNDS[:, 0].copy(), BOUNDS[:, 1].copy()
RANGE = MX - MN
Z_MAX = 5.78
TWO_PI = 6.283185307179586


def normal_of(x1, x2):
    """z of two generator words (arrays of uint32) -> float32"""
    u1 = ((np.asarray(x1, np.uint32) >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (np.asarray(x2, np.uint32) >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    return (np.sqrt(-2.0 * np.log(u1)) * np.cos(TWO_PI * u2)).astype(F)


def normal(seed, ctr, lane0):
    lane0 = np.asarray(lane0, np.uint64)
    return normal_of(philox_u32(seed, ctr, lane0), philox_u32(seed, ctr, lane0 + np.uint64(1)))


def lanes(rows):
    """[len(rows), 10] lane0 of every column of the given rows (workers, minibatch rows)"""
    return np.asarray(rows, np.uint64)[:, None] * np.uint64(32) + np.uint64(2) * np.arange(NO, dtype=np.uint64)[None, :]


def row_normals(seed, ctrs, rows):
    """z [len(rows), 10] with row i keyed by (seed, ctrs[i], rows[i] 32 + 2 j); ctrs a scalar or one per row"""
    rows = np.asarray(rows)
    ctrs = np.broadcast_to(np.asarray(ctrs, np.uint64), rows.shape)
    ln = lanes(rows)
    out = np.empty((len(rows), NO), F)
    for c in np.unique(ctrs):
        m = ctrs == c
        out[m] = normal(seed, int(c), ln[m])
    return out


def sigmas(sigma_logits, sigma_params):
    return np.array([sigma_logits] * NA + [sigma_params] * (NO - NA), F)


def ou_step(x, theta, sigma, z):
    """x, sigma, z float32 arrays (sigma per column) -> the next state"""
    x, z, sigma, theta = np.asarray(x, F), np.asarray(z, F), np.asarray(sigma, F), F(theta)
    return (x - theta * x) + sigma * z


def clipped(sigma, z, clip):
    t = np.asarray(sigma, F) * np.asarray(z, F)
    if clip > 0:
        t = np.minimum(np.maximum(t, F(-clip)), F(clip))
    return t


def apply(v, t, clamp):
    """rows v [.., 10] with the noise t (units of the range) on them"""
    out = np.asarray(v, F) + RANGE * np.asarray(t, F)
    if clamp:
        out = np.minimum(np.maximum(out, MN), MX)
    return out


def ulps32(a, b):
    """distance in float32 ulps between two float32 arrays of equal sign pattern (or across zero)"""
    def key(x):
        i = np.asarray(x, F).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))
