"""Host mirror of the reference's camera / pose records and CameraPose.findScaled
(/root/reference/src/MiniCV/Camera.fs, /root/reference/src/MiniCV/CameraPose.fs).

`findScaled` keeps the F# signature and semantics (CameraPose.fs:39-134): the O(N^2) scale
hypothesize-and-verify runs in libMiniCVNative.so on the GPU (cvFindScaledPose); this module only
marshals the records and builds the scaled pose, as the F# wrapper would. The
numpy helpers below (lookAt, project1, transformed_view) build test/bench inputs; they are not on
the product path.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field

import numpy as np

from . import native as N


def _v3(a) -> np.ndarray:
    return np.asarray(a, np.float64).reshape(3)


@dataclass
class Camera:
    """Camera.fs:7-14 (location, forward, up, right, focal)."""
    location: np.ndarray
    forward: np.ndarray
    up: np.ndarray
    right: np.ndarray
    focal: np.ndarray

    def to_c(self) -> N.Camera:
        c = N.Camera()
        for name in ("location", "forward", "up", "right"):
            v = _v3(getattr(self, name))
            setattr(c, name, N.V3d(*v))
        f = np.asarray(self.focal, np.float64).reshape(2)
        c.focal = N.V2d(f[0], f[1])
        return c


def lookAt(eye, center, sky, f) -> Camera:
    """Camera.lookAt (Camera.fs:93-104)."""
    eye, center, sky = _v3(eye), _v3(center), _v3(sky)
    fw = center - eye
    fw = fw / np.linalg.norm(fw)
    r = np.cross(fw, sky)
    r = r / np.linalg.norm(r)
    u = np.cross(r, fw)
    u = u / np.linalg.norm(u)
    return Camera(eye, fw, u, r, np.asarray(f, np.float64).reshape(2))


def project1(c: Camera, pts: np.ndarray):
    """Camera.project1 (Camera.fs:72-83), vectorised: (c[n, 2], visible[n])."""
    o = np.asarray(pts, np.float64).reshape(-1, 3) - c.location
    pc = np.stack([o @ c.right, o @ c.up, o @ c.forward], axis=1)
    xy = c.focal * pc[:, :2] / pc[:, 2:3]
    vis = (pc[:, 2] >= 0) & np.all(xy >= -1.0, axis=1) & np.all(xy <= 1.0, axis=1)
    return xy, vis


@dataclass
class CameraPose:
    """CameraPose.fs:7-16 (struct: the default value is all zero)."""
    RotationIndex: int = 0
    ScaleSign: int = 0
    Rotation: np.ndarray = field(default_factory=lambda: np.zeros((3, 3)))
    Translation: np.ndarray = field(default_factory=lambda: np.zeros(3))
    IsInverse: bool = False


def _sign(f: float) -> int:
    if math.isnan(f):   # F# `sign nan` throws (System.Math.Sign)
        raise ArithmeticError("sign of NaN")
    return int(f > 0) - int(f < 0)


def scale(f: float, pose: CameraPose) -> CameraPose:
    """CameraPose.scale (CameraPose.fs:31-33)."""
    return CameraPose(pose.RotationIndex, _sign(f) * pose.ScaleSign, pose.Rotation, f * _v3(pose.Translation),
                      pose.IsInverse)


def transformation(pose: CameraPose) -> np.ndarray:
    """CameraPose.transformation (CameraPose.fs:24-29): 4x4 forward matrix [R | R t]."""
    m = np.eye(4)
    R = np.asarray(pose.Rotation, np.float64).reshape(3, 3)
    m[:3, :3] = R
    m[:3, 3] = R @ _v3(pose.Translation)
    return m


def transformed_view(t: np.ndarray, c: Camera) -> Camera:
    """Camera.transformedView (Camera.fs:60-70) with a 4x4 forward matrix."""
    to_world = np.eye(4)
    to_world[:3, 0], to_world[:3, 1], to_world[:3, 2], to_world[:3, 3] = c.right, c.up, -c.forward, c.location
    m = to_world @ t
    nz = lambda v: v / np.linalg.norm(v)
    return Camera(m[:3, 3].copy(), nz(-m[:3, 2]), nz(m[:3, 1]), nz(m[:3, 0]), np.asarray(c.focal, np.float64))


def _split_observations(worldObservations):
    if isinstance(worldObservations, tuple) and len(worldObservations) == 2 and \
            isinstance(worldObservations[0], np.ndarray):
        world, obs = worldObservations
    else:
        pairs = list(worldObservations)
        world = np.array([p[0] for p in pairs], np.float64).reshape(-1, 3)
        obs = np.array([p[1] for p in pairs], np.float64).reshape(-1, 2)
    return (np.ascontiguousarray(world, np.float64).reshape(-1, 3),
            np.ascontiguousarray(obs, np.float64).reshape(-1, 2))


def findScaled(inlierThreshold: float, srcCam: Camera, worldObservations, pose: CameraPose):
    """CameraPose.findScaled (CameraPose.fs:39-134) -> (cost, scaled pose).

    worldObservations: a sequence of (V3d, V2d) pairs (the F# list) or a (world[n,3], obs[n,2])
    tuple of arrays. Raises RuntimeError when the native call fails (no CPU fallback)."""
    world, obs = _split_observations(worldObservations)
    n = world.shape[0]
    if n == 0:   # CameraPose.fs:42
        return math.inf, CameraPose()
    R = N.M33d()
    R.M[:] = np.asarray(pose.Rotation, np.float64).reshape(9)
    t = N.V3d(*_v3(pose.Translation))
    cost, s = C.c_double(0), C.c_double(0)
    cam = srcCam.to_c()
    k = N.lib().cvFindScaledPose(float(inlierThreshold), C.addressof(cam), world.ctypes.data, obs.ctypes.data, n,
                                 C.addressof(R), C.addressof(t), C.addressof(cost), C.addressof(s))
    if k < 0:
        raise RuntimeError(f"cvFindScaledPose failed: {N.last_error()}")
    return cost.value, scale(s.value, pose)


def findScaledCosts(srcCam: Camera, world: np.ndarray, obs: np.ndarray, pose: CameraPose):
    """Per-candidate (scales[2n], costs[2n]) of findScaled, in candidate order (analysis helper)."""
    world = np.ascontiguousarray(world, np.float64).reshape(-1, 3)
    obs = np.ascontiguousarray(obs, np.float64).reshape(-1, 2)
    n = world.shape[0]
    R = N.M33d()
    R.M[:] = np.asarray(pose.Rotation, np.float64).reshape(9)
    t = N.V3d(*_v3(pose.Translation))
    sc, co = np.empty(2 * n), np.empty(2 * n)
    cam = srcCam.to_c()
    if N.lib().cvFindScaledPoseCosts(C.addressof(cam), world.ctypes.data, obs.ctypes.data, n, C.addressof(R),
                                     C.addressof(t), sc.ctypes.data, co.ctypes.data) < 0:
        raise RuntimeError(f"cvFindScaledPoseCosts failed: {N.last_error()}")
    return sc, co


def _scaled_batch_args(srcCams, sets, poses, setIdx):
    """The arrays of cvFindScaledPoseBatch: cameras (P, 14), rotations (P, 9), translations (P, 3),
    setIdx (P,) or None, world (R, 3), obs (R, 2), offsets (S + 1,)."""
    cams = cameras_array(list(srcCams))
    poses = list(poses)
    P = len(poses)
    if cams.shape[0] != P:
        raise ValueError("srcCams and poses differ in length")
    rots = np.array([np.asarray(p.Rotation, np.float64).reshape(9) for p in poses], np.float64).reshape(P, 9)
    trans = np.array([_v3(p.Translation) for p in poses], np.float64).reshape(P, 3)
    split = [_split_observations(s) for s in sets]
    off = np.zeros(len(split) + 1, np.int32)
    off[1:] = np.cumsum([w.shape[0] for w, _ in split])
    world = np.concatenate([w for w, _ in split] + [np.empty((0, 3))])
    obs = np.concatenate([o for _, o in split] + [np.empty((0, 2))])
    idx = None if setIdx is None else np.ascontiguousarray(setIdx, np.int32).reshape(-1)
    if idx is not None and idx.shape[0] != P:
        raise ValueError("setIdx and poses differ in length")
    return cams, rots, trans, idx, np.ascontiguousarray(world), np.ascontiguousarray(obs), off


def findScaledBatch(inlierThreshold: float, srcCams, sets, poses, setIdx=None):
    """cvFindScaledPoseBatch: findScaled for P problems in one call -> [(cost, scaled pose)] equal to
    [findScaled(inlierThreshold, srcCams[p], sets[setIdx[p]], poses[p]) for p in range(P)].

    sets: the observation sets, each a sequence of (V3d, V2d) pairs or a (world[n,3], obs[n,2]) tuple;
    setIdx[p] names problem p's set (None: set p, one set per problem). Several problems may share a
    set. inlierThreshold is unused, as in findScaled. Raises NativeError when the native call fails."""
    cams, rots, trans, idx, world, obs, off = _scaled_batch_args(srcCams, sets, poses, setIdx)
    poses = list(poses)
    P = len(poses)
    if P == 0:
        return []
    cost, s = np.empty(P), np.empty(P)
    k = N.lib().cvFindScaledPoseBatch(cams.ctypes.data, rots.ctypes.data, trans.ctypes.data,
                                      None if idx is None else idx.ctypes.data, P,
                                      _nonnull(world, (1, 3)).ctypes.data, _nonnull(obs, (1, 2)).ctypes.data,
                                      off.ctypes.data, off.size - 1, cost.ctypes.data, s.ctypes.data, None)
    N.check(k >= 0, "cvFindScaledPoseBatch")
    sizes = np.diff(off)[np.arange(P) if idx is None else idx]
    return [(float(cost[p]), scale(float(s[p]), poses[p]) if sizes[p] > 0 else CameraPose())   # CameraPose.fs:42
            for p in range(P)]


def findScaledBatchCosts(srcCams, sets, poses, setIdx=None):
    """cvFindScaledPoseBatchCosts: per problem (scales[2n], costs[2n]) as findScaledCosts gives them."""
    cams, rots, trans, idx, world, obs, off = _scaled_batch_args(srcCams, sets, poses, setIdx)
    P = rots.shape[0]
    if P == 0:
        return []
    which = np.arange(P) if idx is None else idx
    if which.size and (which.min() < 0 or which.max() >= off.size - 1):
        raise ValueError("a problem's set is outside the sets given")
    sizes = np.diff(off)[which]
    total = 2 * int(sizes.sum())
    sc, co = np.empty(max(total, 1)), np.empty(max(total, 1))
    k = N.lib().cvFindScaledPoseBatchCosts(cams.ctypes.data, rots.ctypes.data, trans.ctypes.data,
                                           None if idx is None else idx.ctypes.data, P,
                                           _nonnull(world, (1, 3)).ctypes.data, _nonnull(obs, (1, 2)).ctypes.data,
                                           off.ctypes.data, off.size - 1, sc.ctypes.data, co.ctypes.data)
    N.check(k >= 0, "cvFindScaledPoseBatchCosts")
    ends = 2 * np.concatenate([[0], np.cumsum(sizes)])
    return [(sc[ends[p]:ends[p + 1]].copy(), co[ends[p]:ends[p + 1]].copy()) for p in range(P)]


def cameras_array(cameras) -> np.ndarray:
    """Cameras as (n, 14) float64 rows in mcvCamera's field order (location, forward, up, right, focal)."""
    if isinstance(cameras, np.ndarray):
        return np.ascontiguousarray(cameras, np.float64).reshape(-1, 14)
    return np.array([np.concatenate([_v3(c.location), _v3(c.forward), _v3(c.up), _v3(c.right),
                                     np.asarray(c.focal, np.float64).reshape(2)]) for c in cameras],
                    np.float64).reshape(-1, 14)


def unproject1(c: Camera, pt) -> np.ndarray:
    """Camera.unproject1 (Camera.fs:85-91) -> the ray as six doubles (origin, direction). Scalar
    Python floats in the managed evaluation order, as hyp_rays.h ray_unproject."""
    x, y = (float(v) for v in np.asarray(pt, np.float64).reshape(2))
    f = [float(v) for v in np.asarray(c.focal, np.float64).reshape(2)]
    r, u, fw = ([float(v) for v in _v3(a)] for a in (c.right, c.up, c.forward))
    a, b = x / f[0], y / f[1]
    d = [a * r[k] + b * u[k] + fw[k] for k in range(3)]
    l = math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    inv = 1.0 / l if l != 0.0 else 0.0
    return np.array([*(float(v) for v in _v3(c.location)), *(v * inv if l != 0.0 else 0.0 for v in d)])


def _offsets(offsets) -> np.ndarray:
    off = np.ascontiguousarray(offsets, np.int32).reshape(-1)
    if off.size < 1:
        raise ValueError("offsets needs T + 1 entries")
    return off


def _nonnull(a: np.ndarray, shape) -> np.ndarray:
    """An empty array may have no storage: the exports want real pointers."""
    return a if a.size else np.zeros(shape, a.dtype)


def intersectRays(rays, offsets):
    """cvIntersectRays: Ray.intersection (Utilities.fs:159-165) of T tracks given as a CSR over
    rays[n, 6] (origin, direction). -> (points[T, 3], pairCounts[T]); a track without a point (the
    F# None) has pairCounts 0 and a NaN point. Raises NativeError when the native call fails."""
    rays = np.ascontiguousarray(rays, np.float64).reshape(-1, 6)
    off = _offsets(offsets)
    T = off.size - 1
    pts, cnt = np.empty((T, 3)), np.empty(T, np.int32)
    k = N.lib().cvIntersectRays(_nonnull(rays, (1, 6)).ctypes.data, off.ctypes.data, T, _nonnull(pts, (1, 3)).ctypes.data,
                                _nonnull(cnt, 1).ctypes.data)
    N.check(k >= 0, "cvIntersectRays")
    return pts, cnt


def intersection(rays):
    """Ray.intersection (Utilities.fs:159-165): the point of one list of rays, or None."""
    rays = np.ascontiguousarray(rays, np.float64).reshape(-1, 6)
    pts, cnt = intersectRays(rays, [0, rays.shape[0]])
    return pts[0] if cnt[0] > 0 else None


def triangulateTracks(cameras, cameraIdx, obs, offsets, stats: bool = False):
    """cvTriangulateTracks: unproject1 of every observation and Ray.intersection per track.
    cameras: Camera records or (n, 14) rows; cameraIdx[n], obs[n, 2], offsets[T + 1] (CSR).
    -> (points[T, 3], pairCounts[T]), plus (cost[T], visible[T]) with stats=True."""
    cams = cameras_array(cameras)
    idx = np.ascontiguousarray(cameraIdx, np.int32).reshape(-1)
    obs = np.ascontiguousarray(obs, np.float64).reshape(-1, 2)
    off = _offsets(offsets)
    if idx.shape[0] != obs.shape[0]:
        raise ValueError("cameraIdx and obs differ in length")
    T = off.size - 1
    pts, cnt = np.empty((T, 3)), np.empty(T, np.int32)
    cost, vis = (np.empty(T), np.empty(T, np.int32)) if stats else (None, None)
    k = N.lib().cvTriangulateTracks(_nonnull(cams, (1, 14)).ctypes.data, cams.shape[0], _nonnull(idx, 1).ctypes.data,
                                    _nonnull(obs, (1, 2)).ctypes.data, off.ctypes.data, T,
                                    _nonnull(pts, (1, 3)).ctypes.data, _nonnull(cnt, 1).ctypes.data,
                                    _nonnull(cost, 1).ctypes.data if stats else None,
                                    _nonnull(vis, 1).ctypes.data if stats else None)
    N.check(k >= 0, "cvTriangulateTracks")
    return (pts, cnt, cost, vis) if stats else (pts, cnt)


def _build_tracks(export: str, featureCounts, imagePairs, pairs, offsets, mask=None, minLength: int = 2):
    counts = np.ascontiguousarray(featureCounts, np.int32).reshape(-1)
    ip = np.ascontiguousarray(imagePairs, np.int32).reshape(-1, 2)
    pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    off = _offsets(offsets)
    B = off.size - 1
    if ip.shape[0] != B:
        raise ValueError("imagePairs needs one row per problem")
    if pr.shape[0] < off[-1]:
        raise ValueError("pairs is shorter than offsets[B]")
    if mask is not None:
        mask = np.ascontiguousarray(mask).reshape(-1).astype(np.uint8, copy=False)
        if mask.shape[0] < off[-1]:
            raise ValueError("mask is shorter than offsets[B]")
    nodes = int(np.maximum(counts, 0).astype(np.int64).sum())
    maxObs = max(min(2 * max(int(off[-1]), 0), nodes), 0)   # the capacities that are always enough
    maxTracks = maxObs // 2
    toff, cam, feat = np.empty(maxTracks + 1, np.int32), np.empty(maxObs, np.int32), np.empty(maxObs, np.int32)
    tof, dropped = np.empty(nodes, np.int32), np.zeros(3, np.int64)
    T = getattr(N.lib(), export)(_nonnull(counts, 1).ctypes.data, counts.size, _nonnull(ip, (1, 2)).ctypes.data, B,
                                 _nonnull(pr, (1, 2)).ctypes.data, off.ctypes.data,
                                 None if mask is None else _nonnull(mask, 1).ctypes.data, int(minLength),
                                 toff.ctypes.data, maxTracks, _nonnull(cam, 1).ctypes.data,
                                 _nonnull(feat, 1).ctypes.data, maxObs, _nonnull(tof, 1).ctypes.data,
                                 dropped.ctypes.data)
    N.check(T >= 0, export)
    n = int(toff[T])
    return toff[:T + 1].copy(), cam[:n].copy(), feat[:n].copy(), tof, dropped


def buildTracks(featureCounts, imagePairs, pairs, offsets, mask=None, minLength: int = 2):
    """cvBuildTracks: the connected components of the match graph as tracks. featureCounts[nImages];
    imagePairs[B, 2], pairs[n, 2] and offsets[B + 1] as matchFeaturesBatch returns them; mask[n]
    (optional: matchAndFindModelBatch's inlier bytes). Components over MAX_TRACK_LEN nodes, with two
    features of one image, or under minLength nodes are dropped.
    -> (trackOffsets[T + 1], cameraIdx[nObs], featureIdx[nObs], trackOfFeature[sum(featureCounts)],
    dropped[3] = oversize, conflicts, short). trackOffsets and cameraIdx are triangulateTracks' CSR."""
    return _build_tracks("cvBuildTracks", featureCounts, imagePairs, pairs, offsets, mask, minLength)


def trackObservations(pointsPerImage, cameraIdx, featureIdx) -> np.ndarray:
    """The (nObs, 2) float64 observations of a track CSR: pointsPerImage[cameraIdx[k]][featureIdx[k]], so
    that triangulateTracks(cameras, cameraIdx, trackObservations(...), trackOffsets) is one line away."""
    cam = np.ascontiguousarray(cameraIdx, np.int64).reshape(-1)
    feat = np.ascontiguousarray(featureIdx, np.int64).reshape(-1)
    if cam.shape != feat.shape:
        raise ValueError("cameraIdx and featureIdx differ in length")
    obs = np.empty((cam.size, 2), np.float64)
    for i in np.unique(cam):
        sel = cam == i
        obs[sel] = np.asarray(pointsPerImage[int(i)], np.float64).reshape(-1, 2)[feat[sel]]
    return obs


def _bundle_adjust(export: str, cameras, cameraIdx, obs, offsets, points, fixed=None, cfg=None):
    cams = cameras_array(cameras)
    idx = np.ascontiguousarray(cameraIdx, np.int32).reshape(-1)
    obs = np.ascontiguousarray(obs, np.float64).reshape(-1, 2)
    off = _offsets(offsets)
    pts = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    T = off.size - 1
    if idx.shape[0] != obs.shape[0]:
        raise ValueError("cameraIdx and obs differ in length")
    if pts.shape[0] != T:
        raise ValueError("points needs one row per track")
    if fixed is not None:
        fixed = (np.asarray(fixed).reshape(-1) != 0).astype(np.uint8)
        if fixed.shape[0] != cams.shape[0]:
            raise ValueError("fixed needs one entry per camera")
    outC, outP, sm = np.empty_like(cams), np.empty_like(pts), N.BaSummary()
    k = getattr(N.lib(), export)(_nonnull(cams, (1, 14)).ctypes.data, cams.shape[0],
                                 None if fixed is None else _nonnull(fixed, 1).ctypes.data,
                                 _nonnull(idx, 1).ctypes.data, _nonnull(obs, (1, 2)).ctypes.data, off.ctypes.data, T,
                                 _nonnull(pts, (1, 3)).ctypes.data, None if cfg is None else C.addressof(cfg),
                                 _nonnull(outC, (1, 14)).ctypes.data, _nonnull(outP, (1, 3)).ctypes.data,
                                 C.addressof(sm))
    N.check(k >= 0, export)
    return outC, outP, sm.as_dict()


def bundleAdjust(cameras, cameraIdx, obs, offsets, points, fixed=None, cfg=None):
    """cvBundleAdjust: Levenberg-Marquardt over the cameras (rotation and location) and the track points.
    cameras: Camera records or (n, 14) rows; cameraIdx[n], obs[n, 2], offsets[T + 1] (buildTracks' CSR and
    trackObservations' rows); points[T, 3] (triangulateTracks' points, NaN rows included); fixed[nCameras]
    (optional: true keeps that camera constant); cfg: a native.BaConfig (None = the library's defaults).
    -> (cameras[n, 14], points[T, 3], summary dict of mcvBaSummary's fields)."""
    return _bundle_adjust("cvBundleAdjust", cameras, cameraIdx, obs, offsets, points, fixed, cfg)


def _bundle_adjust_focal(export: str, cameras, cameraIdx, obs, offsets, points, fixed=None, focalGroup=None,
                         fixedFocal=None, cfg=None):
    cams = cameras_array(cameras)
    idx = np.ascontiguousarray(cameraIdx, np.int32).reshape(-1)
    obs = np.ascontiguousarray(obs, np.float64).reshape(-1, 2)
    off = _offsets(offsets)
    pts = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    T = off.size - 1
    if idx.shape[0] != obs.shape[0]:
        raise ValueError("cameraIdx and obs differ in length")
    if pts.shape[0] != T:
        raise ValueError("points needs one row per track")

    def per_camera(a, what, dtype):
        if a is None:
            return None
        a = np.asarray(a).reshape(-1)
        a = (a != 0).astype(np.uint8) if dtype is np.uint8 else np.ascontiguousarray(a, dtype)
        if a.shape[0] != cams.shape[0]:
            raise ValueError(f"{what} needs one entry per camera")
        return a

    fixed = per_camera(fixed, "fixed", np.uint8)
    fixedFocal = per_camera(fixedFocal, "fixedFocal", np.uint8)
    focalGroup = per_camera(focalGroup, "focalGroup", np.int32)
    ptr = lambda a: None if a is None else _nonnull(a, 1).ctypes.data
    outC, outP, sm = np.empty_like(cams), np.empty_like(pts), N.BaFocalSummary()
    k = getattr(N.lib(), export)(_nonnull(cams, (1, 14)).ctypes.data, cams.shape[0], ptr(fixed), ptr(focalGroup),
                                 ptr(fixedFocal), _nonnull(idx, 1).ctypes.data, _nonnull(obs, (1, 2)).ctypes.data,
                                 off.ctypes.data, T, _nonnull(pts, (1, 3)).ctypes.data,
                                 None if cfg is None else C.addressof(cfg), _nonnull(outC, (1, 14)).ctypes.data,
                                 _nonnull(outP, (1, 3)).ctypes.data, C.addressof(sm))
    N.check(k >= 0, export)
    return outC, outP, sm.as_dict()


def bundleAdjustFocal(cameras, cameraIdx, obs, offsets, points, fixed=None, focalGroup=None, fixedFocal=None,
                      cfg=None):
    """cvBundleAdjustFocal: bundleAdjust that also refines the focal lengths. focalGroup[nCameras] (optional:
    cameras with the same value share one focal length; None = one group per camera); fixedFocal[nCameras]
    (optional: true keeps that camera's group constant; independent of fixed, which holds rotation and
    location); cfg: a native.BaFocalConfig (None = the defaults with focalMode 1: one scale per group;
    2 refines fx and fy on their own, 0 is bundleAdjust).
    -> (cameras[n, 14] with the refined focal, points[T, 3], summary dict of mcvBaFocalSummary's fields)."""
    return _bundle_adjust_focal("cvBundleAdjustFocal", cameras, cameraIdx, obs, offsets, points, fixed, focalGroup,
                                fixedFocal, cfg)
