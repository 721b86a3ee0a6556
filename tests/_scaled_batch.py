"""Shared by test_batch_scaled.py and test_gpu_batch_scaled.py: batches of findScaled problems built
from synthetic.scaled_problem, the raw calls of the batch exports with sentinel-filled outputs, and
the per-problem references (oracle, host twin, single call), each computed once per batch."""
import ctypes as C
import functools

import numpy as np

from minicv_amd import camera as CM, native as N, synthetic as S

# 32 observations are one 64-candidate block and one observation tile; 33 straddle both
MIXED_SIZES = (0, 1, 31, 32, 33, 63, 64, 65, 0, 200, 1001, 0)
# problem -> set: the first and the last problem on empty sets, set 8 used by none, the 200-row set 9
# by four poses, the 32-row set 3 by two; not monotone
MIXED_SET_IDX = (0, 9, 1, 2, 9, 3, 4, 10, 5, 9, 6, 7, 9, 3, 11)
SENT_D, SENT_I = -777.25, -777


def cam14(c):
    return np.concatenate([c.location, c.forward, c.up, c.right, c.focal]).astype(np.float64)


def variant(src, pose, k):
    """The k-th (camera, pose) on one set: 0 as generated; 1 the translation's sign flipped; 2 half
    the translation under a slightly different rotation; 3 another focal length."""
    if k % 4 == 1:
        return src, CM.CameraPose(pose.RotationIndex, pose.ScaleSign, pose.Rotation, -pose.Translation, False)
    if k % 4 == 2:
        R2 = S.rotation([1.0, -0.4, 0.2], np.deg2rad(1.5)) @ pose.Rotation
        return src, CM.CameraPose(2, -1, R2, 0.5 * pose.Translation, False)
    if k % 4 == 3:
        return CM.Camera(src.location, src.forward, src.up, src.right, src.focal * np.array([1.25, 0.9])), pose
    return src, pose


class Batch:
    """cams[P], poses[P], sets[S] = (world, obs) and setIdx[P] (None: set p)."""

    def __init__(self, cams, poses, sets, set_idx):
        self.cams, self.poses, self.sets = list(cams), list(poses), list(sets)
        self.set_idx = None if set_idx is None else np.asarray(set_idx, np.int32)
        self.P, self.S = len(self.poses), len(self.sets)
        self.cam_rows = np.ascontiguousarray(np.array([cam14(c) for c in self.cams]).reshape(-1, 14))
        self.rots = np.ascontiguousarray(np.array([p.Rotation.reshape(9) for p in self.poses]).reshape(-1, 9))
        self.trans = np.ascontiguousarray(np.array([p.Translation for p in self.poses]).reshape(-1, 3))
        self.offsets = np.zeros(self.S + 1, np.int32)
        self.offsets[1:] = np.cumsum([w.shape[0] for w, _ in self.sets])
        self.world = np.ascontiguousarray(np.concatenate([w for w, _ in self.sets] + [np.empty((0, 3))]))
        self.obs = np.ascontiguousarray(np.concatenate([o for _, o in self.sets] + [np.empty((0, 2))]))

    def set_of(self, p):
        return self.sets[p if self.set_idx is None else int(self.set_idx[p])]

    def sizes(self):
        return np.array([self.set_of(p)[0].shape[0] for p in range(self.P)], np.int64)

    def expanded(self):
        """The same problems with a set of their own each and setIdx = None."""
        return Batch(self.cams, self.poses, [self.set_of(p) for p in range(self.P)], None)

    def reversed(self):
        """The problems in reversed order (with setIdx = None the sets are reversed with them)."""
        if self.set_idx is None:
            return Batch(self.cams[::-1], self.poses[::-1], self.sets[::-1], None)
        return Batch(self.cams[::-1], self.poses[::-1], self.sets, self.set_idx[::-1].copy())


def make_sets(sizes, seed0):
    """One scaled_problem per set, with its own seed, focal length, outlier share and true scale (both
    cycle within a range in which the generator's rejection sampling still finds points both cameras see)."""
    out = []
    for s, n in enumerate(sizes):
        src, pose, W, O, _ = S.scaled_problem(max(n, 1), seed=seed0 + s, outlier_frac=(0.0, 0.3, 0.5)[s % 3],
                                              sigma=(1e-3, 0.0, 5e-3)[s % 3], true_scale=1.5 + 0.35 * (s % 7),
                                              focal=(1.0 + 0.05 * (s % 6), 1.0 + 0.03 * (s % 4)))
        out.append((src, pose, np.ascontiguousarray(W[:n]), np.ascontiguousarray(O[:n])))
    return out


def build(sizes, set_idx, seed0):
    sets = make_sets(sizes, seed0)
    idx = range(len(sizes)) if set_idx is None else set_idx
    seen = {}
    cams, poses = [], []
    for s in idx:
        k = seen.get(s, 0)
        seen[s] = k + 1
        c, p = variant(sets[s][0], sets[s][1], k)
        cams.append(c)
        poses.append(p)
    return Batch(cams, poses, [(W, O) for _, _, W, O in sets], set_idx)


@functools.lru_cache(maxsize=None)
def mixed():
    return build(MIXED_SIZES, MIXED_SET_IDX, 100)


@functools.lru_cache(maxsize=None)
def many():
    """67 problems of 40 observations: more problems than a wave has lanes."""
    return build((40,) * 67, None, 300)


def _ptr(a):
    return None if a is None else a.ctypes.data


def call(name, b, null=(), P=None, S=None, offsets=None, set_idx="own", evaluated=True):
    """A raw call of cvFindScaledPoseBatch / mcvHostFindScaledPoseBatch on sentinel-filled outputs.
    -> (return value, costs, scales, evaluated, untouched)"""
    P = b.P if P is None else P
    S = b.S if S is None else S
    n = max(P, b.P, 1)
    costs, scales, ev = np.full(n, SENT_D), np.full(n, SENT_D), np.full(n, SENT_I, np.int32)
    off = b.offsets if offsets is None else np.ascontiguousarray(offsets, np.int32)
    idx = b.set_idx if isinstance(set_idx, str) else (None if set_idx is None else
                                                      np.ascontiguousarray(set_idx, np.int32))
    world = b.world if b.world.size else np.zeros((1, 3))
    obs = b.obs if b.obs.size else np.zeros((1, 2))
    args = dict(cams=b.cam_rows, rots=b.rots, trans=b.trans, idx=idx, world=world, obs=obs, off=off, costs=costs,
                scales=scales, ev=ev if evaluated else None)
    for k in null:
        args[k] = None
    r = getattr(N.lib(), name)(_ptr(args["cams"]), _ptr(args["rots"]), _ptr(args["trans"]), _ptr(args["idx"]), P,
                               _ptr(args["world"]), _ptr(args["obs"]), _ptr(args["off"]), S, _ptr(args["costs"]),
                               _ptr(args["scales"]), _ptr(args["ev"]))
    untouched = bool(np.all(costs == SENT_D) and np.all(scales == SENT_D) and np.all(ev == SENT_I))
    return r, costs[:P], scales[:P], ev[:P], untouched


def call_costs(b):
    """cvFindScaledPoseBatchCosts -> (return value, scales, costs, start of every problem's entries)."""
    sizes = b.sizes()
    starts = 2 * np.concatenate([[0], np.cumsum(sizes)])
    sc, co = np.full(max(int(starts[-1]), 1), SENT_D), np.full(max(int(starts[-1]), 1), SENT_D)
    world = b.world if b.world.size else np.zeros((1, 3))
    obs = b.obs if b.obs.size else np.zeros((1, 2))
    r = N.lib().cvFindScaledPoseBatchCosts(_ptr(b.cam_rows), _ptr(b.rots), _ptr(b.trans), _ptr(b.set_idx), b.P,
                                           _ptr(world), _ptr(obs), _ptr(b.offsets), b.S, _ptr(sc), _ptr(co))
    return r, sc, co, starts


def oracle_results(oracle, b):
    """(costs, scales, evaluated) of every problem by oracle.find_scaled; the reference's empty list
    and a problem without a finite cost are +inf, 0.0."""
    costs, scales, ev = np.empty(b.P), np.empty(b.P), np.empty(b.P, np.int32)
    for p in range(b.P):
        W, O = b.set_of(p)
        if W.shape[0] == 0:
            costs[p], scales[p], ev[p] = np.inf, 0.0, 0
            continue
        c, s, k = oracle.find_scaled(cam14(b.cams[p]), W, O, b.poses[p].Rotation, b.poses[p].Translation)
        costs[p], scales[p], ev[p] = (c, s, k) if np.isfinite(c) else (np.inf, 0.0, k)
    return costs, scales, ev


def single_results(b):
    """(costs, scales, evaluated) of every problem by its own cvFindScaledPose call (GPU)."""
    costs, scales, ev = np.empty(b.P), np.empty(b.P), np.empty(b.P, np.int32)
    for p in range(b.P):
        W, O = b.set_of(p)
        cam = b.cams[p].to_c()
        R = N.M33d()
        R.M[:] = b.poses[p].Rotation.reshape(9)
        t = N.V3d(*b.poses[p].Translation)
        c, s = C.c_double(0), C.c_double(0)
        Wn = W if W.size else np.zeros((1, 3))
        On = O if O.size else np.zeros((1, 2))
        k = N.lib().cvFindScaledPose(0.5, C.addressof(cam), Wn.ctypes.data, On.ctypes.data, W.shape[0],
                                     C.addressof(R), C.addressof(t), C.addressof(c), C.addressof(s))
        assert k >= 0, N.last_error()
        costs[p], scales[p], ev[p] = c.value, s.value, k
    return costs, scales, ev


def host_costs(b, p):
    """mcvHostScaledCosts of problem p -> (scales[2n], costs[2n])."""
    W, O = b.set_of(p)
    n = W.shape[0]
    cam = b.cams[p].to_c()
    R = N.M33d()
    R.M[:] = b.poses[p].Rotation.reshape(9)
    t = N.V3d(*b.poses[p].Translation)
    sc, co = np.empty(max(2 * n, 1)), np.empty(max(2 * n, 1))
    Wn = W if W.size else np.zeros((1, 3))
    On = O if O.size else np.zeros((1, 2))
    assert N.lib().mcvHostScaledCosts(C.addressof(cam), Wn.ctypes.data, On.ctypes.data, n, C.addressof(R),
                                      C.addressof(t), sc.ctypes.data, co.ctypes.data) == n, N.last_error()
    return sc[:2 * n], co[:2 * n]


def assert_results(got, ref, what):
    for g, r, name in zip(got, ref, ("costs", "scales", "evaluated")):
        np.testing.assert_array_equal(g, r, err_msg=f"{what}: {name}")
