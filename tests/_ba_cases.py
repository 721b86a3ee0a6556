"""Shared scenes of the bundle-adjustment tests (test_bundle_adjust.py, test_gpu_bundle_adjust.py): a
numpy restatement of the model of DESIGN §7m (residual, Cayley retraction, loss), a scene builder, the
named cases both files run, and the call wrapper. Nothing here calls the GPU by itself."""
import ctypes as C
from dataclasses import dataclass, field, replace

import numpy as np

from minicv_amd import camera as CM
from minicv_amd import native as N

SENTINEL = -77.25


# ---- the model, restated with numpy ----

def rot(c14):
    """R = rows (right, up, forward) of an mcvCamera row."""
    return np.stack([c14[9:12], c14[6:9], c14[3:6]])


def residuals(cams, pts, idx, obs, off):
    """(r[n, 2], pc[n, 3]) of every observation."""
    cams, pts, obs = np.asarray(cams, float).reshape(-1, 14), np.asarray(pts, float).reshape(-1, 3), np.asarray(obs, float).reshape(-1, 2)
    idx, off = np.asarray(idx), np.asarray(off)
    trk = np.repeat(np.arange(len(off) - 1), np.diff(off))
    r, pcs = np.empty((len(idx), 2)), np.empty((len(idx), 3))
    for k in range(len(idx)):
        c = cams[idx[k]]
        pc = rot(c) @ (pts[trk[k]] - c[0:3])
        pcs[k] = pc
        with np.errstate(all="ignore"):
            r[k] = c[12:14] * pc[:2] / pc[2] - obs[k]
    return r, pcs


def used_set(cams, pts, idx, obs, off):
    r, pc = residuals(cams, pts, idx, obs, off)
    off = np.asarray(off)
    trk = np.repeat(np.arange(len(off) - 1), np.diff(off))
    pts = np.asarray(pts, float).reshape(-1, 3)
    u = np.isfinite(pts[trk]).all(axis=1) & (pc[:, 2] > 0) & np.isfinite(r).all(axis=1)
    for t in range(len(off) - 1):
        if u[off[t]:off[t + 1]].sum() < 2:
            u[off[t]:off[t + 1]] = False
    return u


def rho(r, delta):
    e = np.sqrt((r * r).sum(axis=1))
    if delta <= 0:
        return e * e
    return np.where(e <= delta, e * e, 2 * delta * e - delta * delta)


def cost(cams, pts, idx, obs, off, used, delta=0.0):
    r, _ = residuals(cams, pts, idx, obs, off)
    return float(rho(r[used], delta).sum())


def residuals_v(cams, pts, idx, obs, off):
    """residuals() without the loop over the observations. The three products of a row of R with
    (X - c) are summed left to right here and by numpy's matrix product there, so pc may differ from the
    loop form's in the last place (a product may be fused into the sum there): test_bundle_adjust.py
    bounds the difference on a small case."""
    cams, pts, obs = np.asarray(cams, float).reshape(-1, 14), np.asarray(pts, float).reshape(-1, 3), np.asarray(obs, float).reshape(-1, 2)
    idx, off = np.asarray(idx), np.asarray(off)
    trk = np.repeat(np.arange(len(off) - 1), np.diff(off))
    c = cams[idx]
    d = pts[trk] - c[:, 0:3]
    pc = np.stack([c[:, 9] * d[:, 0] + c[:, 10] * d[:, 1] + c[:, 11] * d[:, 2],
                   c[:, 6] * d[:, 0] + c[:, 7] * d[:, 1] + c[:, 8] * d[:, 2],
                   c[:, 3] * d[:, 0] + c[:, 4] * d[:, 1] + c[:, 5] * d[:, 2]], axis=1)
    with np.errstate(all="ignore"):
        r = c[:, 12:14] * pc[:, :2] / pc[:, 2:3] - obs
    return r, pc


def used_set_v(cams, pts, idx, obs, off):
    r, pc = residuals_v(cams, pts, idx, obs, off)
    off = np.asarray(off)
    trk = np.repeat(np.arange(len(off) - 1), np.diff(off))
    pts = np.asarray(pts, float).reshape(-1, 3)
    u = np.isfinite(pts[trk]).all(axis=1) & (pc[:, 2] > 0) & np.isfinite(r).all(axis=1)
    return u & (np.bincount(trk, u, len(off) - 1) >= 2)[trk]


def cost_terms_v(cams, pts, idx, obs, off, used, delta=0.0):
    """rho of every used observation: cost_v is their numpy (pairwise) sum."""
    r, _ = residuals_v(cams, pts, idx, obs, off)
    return rho(r[used], delta)


def cost_v(cams, pts, idx, obs, off, used, delta=0.0):
    return float(cost_terms_v(cams, pts, idx, obs, off, used, delta).sum())


def cayley(w):
    a = np.asarray(w, float) / 2
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + (2 / (1 + a @ a)) * (K + K @ K)


def retract(c14, x6):
    """The camera moved by (omega, dc)."""
    out = np.array(c14, float)
    R = cayley(x6[:3]) @ rot(c14)
    out[9:12], out[6:9], out[3:6] = R[0], R[1], R[2]
    out[0:3] = c14[0:3] + x6[3:]
    return out


# ---- scenes ----

@dataclass
class Case:
    cams: np.ndarray
    idx: np.ndarray
    obs: np.ndarray
    off: np.ndarray
    pts: np.ndarray
    fixed: object = None
    cfg: dict = field(default_factory=dict)
    truth: tuple = None          # (cams, pts) the observations were made from

    def config(self):
        return N.BaConfig.default(**self.cfg)


def ring(nCam, focal=1.5, radius=6.0, rise=0.1):
    return CM.cameras_array([CM.lookAt((radius * np.cos(a), radius * np.sin(a), 1.0 + rise * i), (0, 0, 0), (0, 0, 1),
                                       (focal, focal)) for i, a in enumerate(2 * np.pi * np.arange(nCam) / nCam)])


def observe(cams, world, camLists, noise=0.0, rng=None):
    """CSR of tracks: track t sees world[t] from the cameras camLists[t], in that order."""
    idx = np.concatenate([np.asarray(c, np.int32) for c in camLists]).astype(np.int32)
    off = np.concatenate([[0], np.cumsum([len(c) for c in camLists])]).astype(np.int32)
    r, pc = residuals(cams, world, idx, np.zeros((len(idx), 2)), off)
    assert (pc[:, 2] > 0).all()
    obs = r + (rng.normal(0, noise, r.shape) if noise else 0.0)
    return idx, obs, off


def observe_v(cams, world, idx, off, noise=0.0, rng=None):
    """observe() for a CSR that is already laid out, through residuals_v."""
    r, pc = residuals_v(cams, world, idx, np.zeros((len(idx), 2)), off)
    assert (pc[:, 2] > 0).all()
    return r + (rng.normal(0, noise, r.shape) if noise else 0.0)


def perturbed(rng, cams, fixed, dCam):
    """scene()'s start: every camera that is not fixed moved by dCam = (rad, units)."""
    start = cams.copy()
    for j in np.nonzero(~np.asarray(fixed, bool))[0]:
        w = rng.normal(size=3)
        start[j] = retract(cams[j], np.concatenate([dCam[0] * w / np.linalg.norm(w), rng.uniform(-1, 1, 3) * dCam[1]]))
    return start


def scene(seed, nCam, T, lengths=None, noise=0.0, dCam=(0.02, 0.05), dPts=0.05, nFixed=2, **cfg):
    """A ring of cameras over T points in [-1, 1]^3; every track sees `lengths[t]` cameras (all of them
    by default; repeats when longer than the ring). Cameras beyond the first nFixed are moved by
    dCam = (rad, units), the points by dPts."""
    rng = np.random.default_rng(seed)
    cams = ring(nCam)
    world = rng.uniform(-1, 1, (T, 3))
    lengths = [nCam] * T if lengths is None else lengths
    lists = [(rng.permutation(nCam)[:L] if L <= nCam else rng.integers(0, nCam, L)) for L in lengths]
    idx, obs, off = observe(cams, world, lists, noise, rng)
    start = cams.copy()
    for j in range(nFixed, nCam):
        w = rng.normal(size=3)
        start[j] = retract(cams[j], np.concatenate([dCam[0] * w / np.linalg.norm(w), rng.uniform(-1, 1, 3) * dCam[1]]))
    pts = world + rng.uniform(-1, 1, world.shape) * dPts
    fixed = np.zeros(nCam, np.uint8)
    fixed[:nFixed] = 1
    return Case(start, idx, obs, off, pts, fixed, cfg, (cams, world))


def _with_outliers(c, seed, frac=0.1, size=0.3):
    rng = np.random.default_rng(seed)
    obs = c.obs.copy()
    bad = rng.random(len(obs)) < frac
    obs[bad] += rng.choice([-1, 1], (bad.sum(), 2)) * size
    return replace(c, obs=obs), bad


def _exclusions():
    c = scene(11, 5, 24, noise=1e-3, maxIterations=6)
    pts, idx, off = c.pts.copy(), c.idx.copy(), c.off.copy()
    pts[3] = np.nan                         # a NaN point of triangulateTracks
    pts[7] = 3.0 * c.cams[idx[off[7]], 0:3]  # beyond its first camera: behind it, and one track short
    keep = np.ones(len(idx), bool)
    keep[off[7] + 2:off[8]] = False         # track 7 keeps two observations, one of them behind
    keep[off[12] + 1:off[13]] = False       # track 12 keeps one observation
    lens = [int(keep[off[t]:off[t + 1]].sum()) for t in range(len(off) - 1)]
    return replace(c, pts=pts, idx=idx[keep], obs=c.obs[keep], off=np.concatenate([[0], np.cumsum(lens)]).astype(np.int32))


def _seg_edges():
    """Cameras 0..3 with kBaSeg - 1, kBaSeg, kBaSeg + 1 and 2 kBaSeg + 3 observations, camera 5 with none."""
    S = N.BA_SEG
    rng = np.random.default_rng(21)
    cams = ring(6)
    want = [S - 1, S, S + 1, 2 * S + 3, 700, 0]
    pool = rng.permutation(np.repeat(np.arange(6), want))
    lists, k = [], 0
    while k < len(pool):
        L = int(rng.integers(2, 6))
        if len(pool) - k - L < 2:
            L = len(pool) - k
        lists.append(pool[k:k + L])
        k += L
    world = rng.uniform(-1, 1, (len(lists), 3))
    idx, obs, off = observe(cams, world, lists, 1e-3, rng)
    assert np.bincount(idx, minlength=6).tolist() == want
    start = cams.copy()
    for j in range(1, 5):
        start[j] = retract(cams[j], rng.normal(0, 0.004, 6))
    return Case(start, idx, obs, off, world + rng.normal(0, 0.01, world.shape), np.array([1, 0, 0, 0, 0, 0], np.uint8),
                dict(maxIterations=3), (cams, world))


def camera_ring_special(nCam):
    """(the camera without an observation, the fixed camera beyond the two at the front) of camera_ring:
    the last two cameras, but the two before the last where the last camera is alone in its trip of the
    chains over j, j + 256, ... (nCam = 257, 513): that camera stays free and observed, so the trip adds
    a non-zero term to r.z, p.q and the cost. With 513 cameras both are beyond the first 256."""
    return (nCam - 3, nCam - 2) if nCam % 256 == 1 else (nCam - 2, nCam - 1)


def camera_ring(nCam, seed=None, perCam=None, **cfg):
    """A ring of nCam cameras (risen by 5 units over the whole ring) and tracks of 4 to 6 observations
    dealt from perCam shuffles of the cameras (about 2000 observations by default, at least 3 per
    camera), so every camera has at least perCam observations but one with none; cameras 0, 1 and one
    more are fixed (camera_ring_special); noise 1e-3, scene()'s perturbation."""
    rng = np.random.default_rng(1000 + nCam if seed is None else seed)
    cams = ring(nCam, rise=5.0 / nCam)
    empty, alsoFixed = camera_ring_special(nCam)
    seen = np.setdiff1d(np.arange(nCam), [empty])
    perCam = max(3, -(-2000 // nCam)) if perCam is None else perCam
    pool = np.concatenate([rng.permutation(seen) for _ in range(perCam)])
    lens, k = [], 0
    while k < len(pool):
        L = int(rng.integers(4, 7))
        if len(pool) - k - L < 4:
            L = len(pool) - k
        lens.append(L)
        k += L
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    idx = pool.astype(np.int32)
    world = rng.uniform(-1, 1, (len(lens), 3))
    obs = observe_v(cams, world, idx, off, 1e-3, rng)
    fixed = np.zeros(nCam, np.uint8)
    fixed[[0, 1, alsoFixed]] = 1
    start = perturbed(rng, cams, fixed, (0.02, 0.05))
    pts = world + rng.uniform(-1, 1, world.shape) * 0.05
    return Case(start, idx, obs, off, pts, fixed, dict(dict(maxIterations=3), **cfg), (cams, world))


SCALE_LONG, SCALE_SHORT, SCALE_CAMERAS = 4200, 84000, 70


def scale_scene(seed=77):
    """70 cameras, SCALE_LONG tracks of kBaShortMax + 1 observations among SCALE_SHORT tracks of 3 in a
    seeded shuffle, every track from distinct cameras: more observations than a grid of threads, more
    long tracks than the waves of the long-track kernels, several segments per camera. Noise 1e-3,
    scene()'s perturbation, Huber on, two iterations of one PCG chunk."""
    rng = np.random.default_rng(seed)
    nCam = SCALE_CAMERAS
    cams = ring(nCam)
    lens = np.concatenate([np.full(SCALE_LONG, N.BA_SHORT_MAX + 1), np.full(SCALE_SHORT, 3)])
    lens = lens[rng.permutation(len(lens))]
    T = len(lens)
    first = np.argsort(rng.random((T, nCam)), axis=1)             # a shuffle of the cameras per track
    idx = first[np.arange(nCam)[None, :] < lens[:, None]].astype(np.int32)   # row-major: track by track
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    world = rng.uniform(-1, 1, (T, 3))
    obs = observe_v(cams, world, idx, off, 1e-3, rng)
    fixed = np.zeros(nCam, np.uint8)
    fixed[:2] = 1
    start = perturbed(rng, cams, fixed, (0.02, 0.05))
    pts = world + rng.uniform(-1, 1, world.shape) * 0.05
    return Case(start, idx, obs, off, pts, fixed,
                dict(maxIterations=2, maxCgIterations=N.BA_CG_CHUNK, huberDelta=0.01), (cams, world))


def _zero_cost():
    """Axis-aligned cameras and dyadic coordinates: every residual is exactly zero."""
    cams = np.array([[0, 0, 0, 0, 0, 1, 0, 1, 0, 1, 0, 0, 1, 1], [1, 0, 0, 0, 0, 1, 0, 1, 0, 1, 0, 0, 1, 1]], float)
    pts = np.array([[0.5, 0.25, 2.0], [-0.5, 0.5, 4.0]])
    idx, off = np.array([0, 1, 0, 1], np.int32), np.array([0, 2, 4], np.int32)
    r, _ = residuals(cams, pts, idx, np.zeros((4, 2)), off)
    return Case(cams, idx, r, off, pts, None, {})


def _lambda_overflow():
    """Observations so large that every cost is +inf: no trial is ever accepted."""
    c = scene(31, 3, 8, nFixed=1)
    return replace(c, obs=np.full_like(c.obs, 1e200), truth=None)


def _nothing_used():
    c = scene(32, 3, 6)
    return replace(c, pts=np.full_like(c.pts, np.nan), truth=None)


CASES = {
    # the CPU tests' named cases
    "converge": lambda: scene(1, 6, 40, functionTolerance=0.0, cgTolerance=1e-10, maxIterations=50),
    "huber_on": lambda: replace(_with_outliers(scene(2, 6, 60, noise=1e-3, dCam=(0.005, 0.01), dPts=0.02), 3)[0],
                                cfg=dict(huberDelta=0.01, maxIterations=30)),
    "huber_off": lambda: replace(_with_outliers(scene(2, 6, 60, noise=1e-3, dCam=(0.005, 0.01), dPts=0.02), 3)[0],
                                 cfg=dict(maxIterations=30)),
    "exclusions": _exclusions,
    "rejected": lambda: scene(1, 5, 30, noise=1e-3, dCam=(0.8, 1.5), dPts=1.0, initialLambda=1e-9, maxIterations=30),
    # the shapes at every edge
    "T63": lambda: scene(5, 4, 63, noise=1e-3, maxIterations=4),
    "T64": lambda: scene(6, 4, 64, noise=1e-3, maxIterations=4),
    "T65": lambda: scene(7, 4, 65, noise=1e-3, maxIterations=4),
    "track_lengths": lambda: scene(8, 70, 12, lengths=[2, 63, 64, 65, 130, 600, 2, 3, 64, 65, 5, 70], noise=1e-3,
                                   maxIterations=4),
    "segment_edges": _seg_edges,
    "all_fixed": lambda: scene(9, 4, 30, noise=1e-3, nFixed=4, maxIterations=5),
    "none_fixed": lambda: scene(10, 4, 30, noise=1e-3, nFixed=0, maxIterations=5),
    # more cameras than one workgroup chains in one trip, and than one block of the per-camera kernels
    **{f"cameras_{n}": (lambda n=n: camera_ring(n)) for n in (255, 256, 257, 513)},
    # the termination codes reachable from valid input
    "term_function": lambda: scene(12, 5, 40, noise=1e-3),
    "term_iterations": lambda: scene(13, 5, 40, noise=1e-3, maxIterations=2),
    "term_zero_cost": _zero_cost,
    "term_lambda": _lambda_overflow,
    "term_nothing": _nothing_used,
}
TERMINATION = {"term_function": 1, "term_iterations": 2, "term_zero_cost": 3, "term_lambda": 4, "term_nothing": 5}

_cache = {}


def case(name) -> Case:
    """A named case, or "scale" (not in CASES: its tests ask more of it than the list's do)."""
    if name not in _cache:
        _cache[name] = scale_scene() if name == "scale" else CASES[name]()
    return _cache[name]


def permuted(c: Case, seed) -> tuple:
    """The same scene with its tracks in another order, and the order (new position -> old track)."""
    order = np.random.default_rng(seed).permutation(len(c.off) - 1)
    sl = [np.arange(c.off[t], c.off[t + 1]) for t in order]
    take = np.concatenate(sl) if sl else np.zeros(0, int)
    off = np.concatenate([[0], np.cumsum([len(s) for s in sl])]).astype(np.int32)
    return replace(c, idx=c.idx[take], obs=c.obs[take], off=off, pts=c.pts[order]), order


# ---- calls ----

def run(export, c: Case, cfg=None):
    """-> (return value, cameras, points, summary dict); the outputs start sentinel-filled."""
    cams = np.ascontiguousarray(c.cams, np.float64).reshape(-1, 14)
    idx = np.ascontiguousarray(c.idx, np.int32)
    obs = np.ascontiguousarray(c.obs, np.float64).reshape(-1, 2)
    off = np.ascontiguousarray(c.off, np.int32)
    pts = np.ascontiguousarray(c.pts, np.float64).reshape(-1, 3)
    fixed = None if c.fixed is None else np.ascontiguousarray(c.fixed, np.uint8)
    cfg = c.config() if cfg is None else cfg
    outC, outP = np.full((max(len(cams), 1), 14), SENTINEL), np.full((max(len(pts), 1), 3), SENTINEL)
    sm = N.BaSummary()
    sm.termination = -9
    ret = getattr(N.lib(), export)(cams.ctypes.data if cams.size else None, len(cams),
                                   None if fixed is None else fixed.ctypes.data, idx.ctypes.data if idx.size else None,
                                   obs.ctypes.data if obs.size else None, off.ctypes.data,
                                   len(off) - 1, pts.ctypes.data if pts.size else None, C.addressof(cfg),
                                   outC.ctypes.data, outP.ctypes.data, C.addressof(sm))
    return ret, outC[:len(cams)], outP[:len(pts)], sm.as_dict()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))
