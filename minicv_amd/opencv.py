"""Host-side mirror of the reference's managed wrappers (module `OpenCV`,
/root/reference/src/MiniCV/OpenCV.fs:855-1052): allocate caller-owned outputs, call the native
export, map the byte mask to bool, return tuples. New wrappers for the hot-path exports follow
the pattern of `OpenCV.recoverPose` (OpenCV.fs:855-861).

Everything here calls libMiniCVNative.so; errors surface as NativeError with the native message.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import native as N


@dataclass
class RansacParams:
    """RANSAC configuration (C struct RansacConfig). Defaults follow cv::findHomography
    (thr 3, maxIters 2000, confidence 0.995)."""
    threshold: float = 3.0
    confidence: float = 0.995
    max_iters: int = 2000
    method: int = N.METHOD_RANSAC
    seed: int = 0
    device_count: int = 1
    fixed_iters: bool = False
    refine: bool = True
    error_kind: int = N.FERR_SAMPSON
    fused_error: bool = False   # opt-in FMA-contracted error (default: OpenCV op-by-op order)
    seven_point: bool = False   # fundamental: OpenCV FM_RANSAC's 7-point minimal sets (<= 3 models each)
    fast_minimal: bool = False  # opt-in: H / 8-point F minimal solve by elimination (default: cv::eigen)
    cv_sampler: bool = False    # OpenCV's own sample stream (cv::RNG((uint64)-1) + getSubset); seed unused

    def to_c(self) -> N.RansacConfig:
        flags = (N.FLAG_FIXED_ITERS if self.fixed_iters else 0) | (0 if self.refine else N.FLAG_NO_REFINE) | \
            (N.FLAG_FUSED_ERROR if self.fused_error else 0) | (N.FLAG_SEVEN_POINT if self.seven_point else 0) | \
            (N.FLAG_FAST_MINIMAL if self.fast_minimal else 0) | (N.FLAG_CV_SAMPLER if self.cv_sampler else 0)
        return N.RansacConfig(self.threshold, self.confidence, int(self.max_iters), int(self.method),
                              int(self.seed) & 0xFFFFFFFFFFFFFFFF, int(self.device_count), flags,
                              int(self.error_kind), 0)


def _v2d(a) -> np.ndarray:
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError("points must be an (N, 2) array")
    return a


def findHomography(src, dst, params: RansacParams | None = None):
    """-> (inlierCount, H (3x3 float64), mask (bool[N])). Raises NativeError on failure.
    params.method: N.METHOD_RANSAC (default), N.METHOD_LSQ, or N.METHOD_LMEDS (cv::LMEDS: no threshold,
    the smallest median error wins)."""
    params = params or RansacParams()
    a, b = _v2d(src), _v2d(dst)
    n = a.shape[0]
    if b.shape[0] != n:
        raise ValueError("src/dst length mismatch")
    H = N.M33d()
    ms = np.zeros(max(n, 1), dtype=np.uint8)
    cfg = params.to_c()
    cnt = N.lib().cvFindHomography(a.ctypes.data, b.ctypes.data, n, N.C.addressof(cfg), N.C.addressof(H),
                                   ms.ctypes.data)
    N.check(cnt > 0, "cvFindHomography")
    return cnt, np.array(H.M[:], dtype=np.float64).reshape(3, 3), ms[:n] != 0


def findFundamentalMat(a, b, params: RansacParams | None = None):
    """8-point RANSAC (default), or OpenCV FM_RANSAC with params.seven_point (+ error_kind EPIPOLAR).
    params.method = N.METHOD_LMEDS: cv::LMEDS (no threshold); with seven_point it runs at any N >= 7.
    -> (inlierCount, F (3x3 float64), mask (bool[N]))."""
    params = params or RansacParams(threshold=3.0, confidence=0.99)
    pa, pb = _v2d(a), _v2d(b)
    n = pa.shape[0]
    F = N.M33d()
    ms = np.zeros(max(n, 1), dtype=np.uint8)
    cfg = params.to_c()
    cnt = N.lib().cvFindFundamentalMat(pa.ctypes.data, pb.ctypes.data, n, N.C.addressof(cfg), N.C.addressof(F),
                                       ms.ctypes.data)
    N.check(cnt > 0, "cvFindFundamentalMat")
    return cnt, np.array(F.M[:], dtype=np.float64).reshape(3, 3), ms[:n] != 0


def _estimate_affine(fn, name, from_, to, params):
    params = params or RansacParams(threshold=3.0, confidence=0.99, cv_sampler=True)
    a, b = _v2d(from_), _v2d(to)
    n = a.shape[0]
    if b.shape[0] != n:
        raise ValueError("from/to length mismatch")
    A = np.zeros(6, dtype=np.float64)
    ms = np.zeros(max(n, 1), dtype=np.uint8)
    cfg = params.to_c()
    cnt = fn(a.ctypes.data, b.ctypes.data, n, N.C.addressof(cfg), A.ctypes.data, ms.ctypes.data)
    N.check(cnt > 0, name)
    return A.reshape(2, 3), ms[:n] != 0, cnt


def estimateAffine2D(from_, to, params: RansacParams | None = None):
    """cv::estimateAffine2D (6 DoF, 3-point samples) -> (A (2x3 float64), mask (bool[N]), inlierCount).
    params.method: N.METHOD_RANSAC (default) or N.METHOD_LMEDS; params None: OpenCV's defaults (threshold 3,
    maxIters 2000, confidence 0.99, its own sample stream, refine on). Raises NativeError on failure."""
    return _estimate_affine(N.lib().cvEstimateAffine2D, "cvEstimateAffine2D", from_, to, params)


def estimateAffinePartial2D(from_, to, params: RansacParams | None = None):
    """cv::estimateAffinePartial2D (4-DoF similarity [a -b tx; b a ty], 2-point samples)
    -> (A (2x3 float64), mask (bool[N]), inlierCount). Parameters as estimateAffine2D."""
    return _estimate_affine(N.lib().cvEstimateAffinePartial2D, "cvEstimateAffinePartial2D", from_, to, params)


def findModelBatch(model: int, srcs, dsts, params: RansacParams | None = None):
    """cvFindModelBatch: B independent RANSAC problems of one family (N.MODEL_HOMOGRAPHY, N.MODEL_FUNDAMENTAL,
    N.MODEL_AFFINE, N.MODEL_SIMILARITY) in one call. srcs / dsts: lists of (N_p, 2) arrays.
    -> a list of (count, M (3x3 float64), mask (bool[N_p])) per problem, each equal to the single wrapper's
    result on that pair; a problem without a model gives (0, zeros, all-False) and N.last_error() names the
    first such problem. params None: the single export's own defaults. Raises NativeError when the whole
    call is refused."""
    if len(srcs) != len(dsts):
        raise ValueError("srcs/dsts length mismatch")
    B = len(srcs)
    pa = [_v2d(x) for x in srcs]
    pb = [_v2d(x) for x in dsts]
    for x, y in zip(pa, pb):
        if x.shape[0] != y.shape[0]:
            raise ValueError("src/dst length mismatch")
    offsets = np.zeros(B + 1, dtype=np.int32)
    offsets[1:] = np.cumsum([x.shape[0] for x in pa])
    total = int(offsets[B])
    a = np.ascontiguousarray(np.concatenate(pa, axis=0)) if total else np.zeros((1, 2))
    b = np.ascontiguousarray(np.concatenate(pb, axis=0)) if total else np.zeros((1, 2))
    models = np.zeros((max(B, 1), 9), dtype=np.float64)
    counts = np.zeros(max(B, 1), dtype=np.int32)
    ms = np.zeros(max(total, 1), dtype=np.uint8)
    cfg = params.to_c() if params is not None else None
    ret = N.lib().cvFindModelBatch(int(model), a.ctypes.data, b.ctypes.data, offsets.ctypes.data, B,
                                   N.C.addressof(cfg) if cfg is not None else None, models.ctypes.data,
                                   ms.ctypes.data, counts.ctypes.data)
    N.check(ret >= 0, "cvFindModelBatch")
    return [(int(counts[p]), models[p].reshape(3, 3).copy(), ms[offsets[p]:offsets[p + 1]] != 0) for p in range(B)]


def matchHamming(q, t, deviceCount: int = 1):
    """BFMatcher(NORM_HAMMING).knnMatch(k=2). q, t: uint8 [n][bytes]. -> (idx, dist, idx2, dist2).
    deviceCount > 1: cvMatchHammingMulti (query blocks over the visible GPUs, same answer)."""
    q = np.ascontiguousarray(q, dtype=np.uint8)
    t = np.ascontiguousarray(t, dtype=np.uint8)
    if q.ndim != 2 or t.ndim != 2 or q.shape[1] != t.shape[1]:
        raise ValueError("descriptor arrays must be [n][bytes] with equal widths")
    nq, nt, nb = q.shape[0], t.shape[0], q.shape[1]
    out = [np.empty(max(nq, 1), dtype=np.int32) for _ in range(4)]
    if deviceCount == 1:
        r = N.lib().cvMatchHamming(q.ctypes.data, nq, t.ctypes.data, nt, nb, *[o.ctypes.data for o in out])
    else:
        r = N.lib().cvMatchHammingMulti(q.ctypes.data, nq, t.ctypes.data, nt, nb, int(deviceCount),
                                        *[o.ctypes.data for o in out])
    N.check(r == nq, "cvMatchHamming")
    return tuple(o[:nq] for o in out)


def matchL2(q, t, deviceCount: int = 1):
    """BFMatcher(NORM_L2).knnMatch(k=2). q, t: float32 [n][dim]. -> (idx, dist, idx2, dist2).
    deviceCount > 1: cvMatchL2Multi (query blocks over the visible GPUs, same answer)."""
    q = np.ascontiguousarray(q, dtype=np.float32)
    t = np.ascontiguousarray(t, dtype=np.float32)
    if q.ndim != 2 or t.ndim != 2 or q.shape[1] != t.shape[1]:
        raise ValueError("descriptor arrays must be [n][dim] with equal widths")
    nq, nt, dim = q.shape[0], t.shape[0], q.shape[1]
    idx, idx2 = np.empty(max(nq, 1), np.int32), np.empty(max(nq, 1), np.int32)
    d, d2 = np.empty(max(nq, 1), np.float32), np.empty(max(nq, 1), np.float32)
    if deviceCount == 1:
        r = N.lib().cvMatchL2(q.ctypes.data, nq, t.ctypes.data, nt, dim, idx.ctypes.data, d.ctypes.data,
                              idx2.ctypes.data, d2.ctypes.data)
    else:
        r = N.lib().cvMatchL2Multi(q.ctypes.data, nq, t.ctypes.data, nt, dim, int(deviceCount), idx.ctypes.data,
                                   d.ctypes.data, idx2.ctypes.data, d2.ctypes.data)
    N.check(r == nq, "cvMatchL2")
    return idx[:nq], d[:nq], idx2[:nq], d2[:nq]


def matchL2U8(q, t, deviceCount: int = 1):
    """BFMatcher(NORM_L2).knnMatch(k=2) on uint8 descriptors (byte SIFT). q, t: uint8 [n][dim], dim <= 512.
    -> (idx, dist, idx2, dist2), exact: the outputs of matchL2 on the same bytes as float32.
    deviceCount > 1: cvMatchL2U8Multi (query blocks over the visible GPUs, same answer)."""
    q = np.ascontiguousarray(q, dtype=np.uint8)
    t = np.ascontiguousarray(t, dtype=np.uint8)
    if q.ndim != 2 or t.ndim != 2 or q.shape[1] != t.shape[1]:
        raise ValueError("descriptor arrays must be [n][dim] with equal widths")
    nq, nt, dim = q.shape[0], t.shape[0], q.shape[1]
    idx, idx2 = np.empty(max(nq, 1), np.int32), np.empty(max(nq, 1), np.int32)
    d, d2 = np.empty(max(nq, 1), np.float32), np.empty(max(nq, 1), np.float32)
    if deviceCount == 1:
        r = N.lib().cvMatchL2U8(q.ctypes.data, nq, t.ctypes.data, nt, dim, idx.ctypes.data, d.ctypes.data,
                                idx2.ctypes.data, d2.ctypes.data)
    else:
        r = N.lib().cvMatchL2U8Multi(q.ctypes.data, nq, t.ctypes.data, nt, dim, int(deviceCount), idx.ctypes.data,
                                     d.ctypes.data, idx2.ctypes.data, d2.ctypes.data)
    N.check(r == nq, "cvMatchL2U8")
    return idx[:nq], d[:nq], idx2[:nq], d2[:nq]


def recoverPoseConfig(focal: float = 1.0, pp=(0.0, 0.0), probability: float = 0.999,
                      threshold: float = 0.005) -> N.RecoverPoseConfig:
    """RecoverPoseConfig (OpenCV.fs:16-36); defaults = RecoverPoseConfig.Default (:33-34)."""
    return N.RecoverPoseConfig(float(focal), N.V2d(float(pp[0]), float(pp[1])), float(probability), float(threshold))


def findEssentialMat(a, b, focal: float = 1.0, pp=(0.0, 0.0), params: RansacParams | None = None):
    """cv::findEssentialMat(a, b, focal, pp, RANSAC, ...) on the GPU.
    -> (inlierCount, E (3x3 float64, unit Frobenius norm), mask (bool[N]))."""
    params = params or RansacParams(threshold=1.0, confidence=0.999, max_iters=1000)
    pa, pb = _v2d(a), _v2d(b)
    n = pa.shape[0]
    if pb.shape[0] != n:
        raise ValueError("a/b length mismatch")
    E = N.M33d()
    ms = np.zeros(max(n, 1), dtype=np.uint8)
    cfg = params.to_c()
    cnt = N.lib().cvFindEssentialMat(pa.ctypes.data, pb.ctypes.data, n, float(focal), N.V2d(*map(float, pp)),
                                     N.C.addressof(cfg), N.C.addressof(E), ms.ctypes.data)
    N.check(cnt > 0, "cvFindEssentialMat")
    return cnt, np.array(E.M[:], dtype=np.float64).reshape(3, 3), ms[:n] != 0


def recoverPose(cfg: N.RecoverPoseConfig, a, b):
    """OpenCV.recoverPose (OpenCV.fs:855-861): -> (res, R, t, mask bytes). res is the number of
    RANSAC inliers passing the cheirality test; the mask is the RANSAC mask (MiniCVNative.cpp:206-210).
    Raises NativeError when the export reports an error (the reference would throw inside OpenCV)."""
    pa, pb = _v2d(a), _v2d(b)
    m, t = N.M33d(), N.V3d(100, 123, 432)
    ms = np.zeros(max(pa.shape[0], 1), dtype=np.uint8)
    res = N.lib().cvRecoverPose(N.C.addressof(cfg), pa.shape[0], pa.ctypes.data, pb.ctypes.data,
                                N.C.addressof(m), N.C.addressof(t), ms.ctypes.data)
    if res <= 0 and N.last_error():
        raise N.NativeError(f"cvRecoverPose: {N.last_error()}")
    return res, np.array(m.M[:]).reshape(3, 3), np.array([t.X, t.Y, t.Z]), ms[:pa.shape[0]]


def _segments(as_, bs):
    """Lists of (N_p, 2) arrays -> (offsets int32[B + 1], a, b concatenated, total)."""
    if len(as_) != len(bs):
        raise ValueError("as/bs length mismatch")
    pa = [_v2d(x) for x in as_]
    pb = [_v2d(x) for x in bs]
    for x, y in zip(pa, pb):
        if x.shape[0] != y.shape[0]:
            raise ValueError("a/b length mismatch")
    B = len(pa)
    offsets = np.zeros(B + 1, dtype=np.int32)
    offsets[1:] = np.cumsum([x.shape[0] for x in pa])
    total = int(offsets[B])
    a = np.ascontiguousarray(np.concatenate(pa, axis=0)) if total else np.zeros((1, 2))
    b = np.ascontiguousarray(np.concatenate(pb, axis=0)) if total else np.zeros((1, 2))
    return offsets, a, b, total


def findEssentialMatBatch(as_, bs, focals, pps, params: RansacParams | None = None):
    """cvFindEssentialMatBatch: B independent findEssentialMat problems in one call. as_ / bs: lists of
    (N_p, 2) arrays; focals: B focal lengths; pps: B principal points.
    -> a list of (count, E (3x3 float64), mask (bool[N_p])) per problem, each equal to findEssentialMat's
    result on that pair; a problem without a model gives (0, zeros, all-False) and N.last_error() names the
    first such problem. params None: findEssentialMat's native defaults. Raises NativeError when the whole
    call is refused."""
    offsets, a, b, total = _segments(as_, bs)
    B = len(as_)
    f = np.ascontiguousarray(np.asarray(focals, dtype=np.float64).reshape(-1))
    pp = np.ascontiguousarray(np.asarray(pps, dtype=np.float64).reshape(-1, 2))
    if f.shape[0] != B or pp.shape[0] != B:
        raise ValueError("focals / pps must have one entry per problem")
    if B == 0:
        f, pp = np.zeros(1), np.zeros((1, 2))
    Es = np.zeros((max(B, 1), 9), dtype=np.float64)
    counts = np.zeros(max(B, 1), dtype=np.int32)
    ms = np.zeros(max(total, 1), dtype=np.uint8)
    cfg = params.to_c() if params is not None else None
    ret = N.lib().cvFindEssentialMatBatch(a.ctypes.data, b.ctypes.data, offsets.ctypes.data, B, f.ctypes.data,
                                          pp.ctypes.data, N.C.addressof(cfg) if cfg is not None else None,
                                          Es.ctypes.data, ms.ctypes.data, counts.ctypes.data)
    N.check(ret >= 0, "cvFindEssentialMatBatch")
    return [(int(counts[p]), Es[p].reshape(3, 3).copy(), ms[offsets[p]:offsets[p + 1]] != 0) for p in range(B)]


def recoverPoseBatch(cfgs, as_, bs):
    """cvRecoverPoseBatch: B independent recoverPose problems in one call. cfgs: one RecoverPoseConfig for
    all, or a list of B. -> a list of (good, R, t, mask bytes) per problem, each equal to recoverPose's result
    on that pair; a failed problem gives (0, zeros, zeros, zeros) and N.last_error() names the first one.
    Raises NativeError when the whole call is refused."""
    offsets, a, b, total = _segments(as_, bs)
    B = len(as_)
    if isinstance(cfgs, N.RecoverPoseConfig):
        cfgs = [cfgs] * B
    if len(cfgs) != B:
        raise ValueError("cfgs must be one config or one per problem")
    carr = (N.RecoverPoseConfig * max(B, 1))()
    for p, c in enumerate(cfgs):
        carr[p] = N.RecoverPoseConfig(c.FocalLength, N.V2d(c.PrincipalPoint.X, c.PrincipalPoint.Y), c.Probability,
                                      c.InlierThreshold)
    Rs = np.zeros((max(B, 1), 9), dtype=np.float64)
    ts = np.zeros((max(B, 1), 3), dtype=np.float64)
    good = np.zeros(max(B, 1), dtype=np.int32)
    ms = np.zeros(max(total, 1), dtype=np.uint8)
    ret = N.lib().cvRecoverPoseBatch(N.C.addressof(carr), a.ctypes.data, b.ctypes.data, offsets.ctypes.data, B,
                                     Rs.ctypes.data, ts.ctypes.data, ms.ctypes.data, good.ctypes.data)
    N.check(ret >= 0, "cvRecoverPoseBatch")
    return [(int(good[p]), Rs[p].reshape(3, 3).copy(), ts[p].copy(), ms[offsets[p]:offsets[p + 1]].copy())
            for p in range(B)]


def recoverPoses(cfg: N.RecoverPoseConfig, a, b):
    """OpenCV.recoverPoses (OpenCV.fs:863-870): -> (R1, R2, t, mask bytes); the bool result is
    ignored like the F# wrapper does (outputs keep their initial values on failure)."""
    pa, pb = _v2d(a), _v2d(b)
    m1, m2 = N.M33d(), N.M33d()
    m1.M[:] = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]
    m2.M[:] = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]
    t = N.V3d(100, 123, 432)
    ms = np.zeros(max(pa.shape[0], 1), dtype=np.uint8)
    N.lib().cvRecoverPoses(N.C.addressof(cfg), pa.shape[0], pa.ctypes.data, pb.ctypes.data, N.C.addressof(m1),
                           N.C.addressof(m2), N.C.addressof(t), ms.ctypes.data)
    return (np.array(m1.M[:]).reshape(3, 3), np.array(m2.M[:]).reshape(3, 3), np.array([t.X, t.Y, t.Z]),
            ms[:pa.shape[0]])


def recoverPoses2(cfg: N.RecoverPoseConfig, a, b):
    """OpenCV.recoverPoses2 (OpenCV.fs:872-909): NDC-like input (x, y) -> (x, -y), focal and
    threshold rescaled, result mapped back with C = diag(1, -1, -1).
    -> (list of (R, t) candidate poses, mask bool[N])."""
    scale = 2.0
    pa = np.stack([(0.5 * _v2d(a)[:, 0]) * scale, (-0.5 * _v2d(a)[:, 1]) * scale], axis=1)
    pb = np.stack([(0.5 * _v2d(b)[:, 0]) * scale, (-0.5 * _v2d(b)[:, 1]) * scale], axis=1)
    c = N.RecoverPoseConfig(scale * cfg.FocalLength / 2.0, N.V2d(0.0, 0.0), cfg.Probability,
                            scale * 0.5 * cfg.InlierThreshold)
    m1, m2, t, ms = recoverPoses(c, pa, pb)
    Cm = np.diag([1.0, -1.0, -1.0])
    m1 = Cm @ m1.T @ Cm
    m2 = Cm @ m2.T @ Cm
    t = Cm @ t
    poses = [(m1, t)] if np.array_equal(m1, m2) else [(m1, t), (m2, t)]
    return poses, ms != 0


def fivepoint(a, b):
    """OpenCV.fivepoint (OpenCV.fs:912-920): -> list of up to 10 essential matrices (3x3)."""
    pa, pb = _v2d(a), _v2d(b)
    if pa.shape[0] < 5 or pb.shape[0] < 5:
        raise ValueError("fivepoint needs 5 correspondences")
    Es = (N.M33d * 10)()
    cnt = N.lib().cvFivePoint(pa.ctypes.data, pb.ctypes.data, Es)
    if cnt <= 0 and N.last_error():
        raise N.NativeError(f"cvFivePoint: {N.last_error()}")
    return [np.array(Es[i].M[:]).reshape(3, 3) for i in range(max(cnt, 0))]


# ---- PnP (OpenCV.fs:922-1052; exports MiniCVNative.cpp:48-163, ap3p.cpp:282) -----------------
SOLVER_KIND = {"Iterative": 0, "EPNP": 1, "P3P": 2, "DLS": 3, "UPNP": 4, "AP3P": 5, "SQPNP": 6}


def _m33(K) -> N.M33d:
    K = np.ascontiguousarray(np.asarray(K, dtype=np.float64).reshape(9))
    m = N.M33d()
    m.M[:] = K.tolist()
    return m


def _dist4(d):
    d = np.zeros(4) if d is None else np.ascontiguousarray(np.asarray(d, dtype=np.float64).reshape(4))
    return d


def _v3d(a) -> np.ndarray:
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError("world points must be an (N, 3) array")
    return a


def solvePnPRansac(img, world, K, dist=None, kind: str = "AP3P", iterations: int = 100, reproj_error: float = 8.0,
                   confidence: float = 0.99, params: RansacParams | None = None):
    """cvSolvePnPRansac (solvePnPInternal with `ransac`, OpenCV.fs:976-1038).
    -> (ok, rvec, tvec, inlier indices int32[count]). With `params` the seeded cvSolvePnPRansacCfg
    export is used (threshold = reprojection error in pixels)."""
    pi, pw = _v2d(img), _v3d(world)
    n = pi.shape[0]
    if pw.shape[0] != n:
        raise ValueError("img/world length mismatch")
    d = _dist4(dist)
    t, r = N.V3d(), N.V3d()
    cnt = N.C.c_int(0)
    inl = np.zeros(max(n, 1), dtype=np.int32)
    if params is None:
        ok = N.lib().cvSolvePnPRansac(pi.ctypes.data, pw.ctypes.data, n, _m33(K), d.ctypes.data, SOLVER_KIND[kind],
                                      int(iterations), float(reproj_error), float(confidence), N.C.addressof(t),
                                      N.C.addressof(r), N.C.addressof(cnt), inl.ctypes.data)
    else:
        cfg = params.to_c()
        cfg.pnpKind = SOLVER_KIND[kind]
        ok = N.lib().cvSolvePnPRansacCfg(pi.ctypes.data, pw.ctypes.data, n, _m33(K), d.ctypes.data,
                                         N.C.addressof(cfg), N.C.addressof(t), N.C.addressof(r), N.C.addressof(cnt),
                                         inl.ctypes.data)
    if not ok and N.last_error() and "no pose" not in N.last_error():
        raise N.NativeError(f"cvSolvePnPRansac: {N.last_error()}")
    return bool(ok), np.array([r.X, r.Y, r.Z]), np.array([t.X, t.Y, t.Z]), inl[:cnt.value].copy()


def solvePnPRansacBatch(imgs, worlds, Ks, dists=None, kind: str = "AP3P", params: RansacParams | None = None):
    """cvSolvePnPRansacBatch: B independent solvePnPRansac problems in one call. imgs / worlds: lists of
    (N_p, 2) / (N_p, 3) arrays; Ks: B camera matrices; dists: None (no distortion) or B rows of (k1, k2, p1, p2).
    -> a list of (ok, rvec, tvec, inlier indices int32[count]) per problem, each equal to
    solvePnPRansac(..., kind=kind, params=params) on that problem; a problem without a pose gives
    (False, zeros, zeros, empty) and N.last_error() names the first such problem. params None: the native
    defaults (100 iterations, 8 px, 0.99, OpenCV's sample stream). Raises NativeError when the whole call is
    refused."""
    B, offsets, img, world, K, d = _pnp_batch_args(imgs, worlds, Ks, dists)
    total = int(offsets[B])
    cfg = None
    if params is not None or kind != "Iterative":
        cfg = params.to_c() if params is not None else _pnp_default_cfg()
        cfg.pnpKind = SOLVER_KIND[kind]
    ts = np.zeros((max(B, 1), 3), dtype=np.float64)
    rs = np.zeros((max(B, 1), 3), dtype=np.float64)
    counts = np.zeros(max(B, 1), dtype=np.int32)
    ms = np.zeros(max(total, 1), dtype=np.uint8)
    ret = N.lib().cvSolvePnPRansacBatch(img.ctypes.data, world.ctypes.data, offsets.ctypes.data, B, K.ctypes.data,
                                        d.ctypes.data if d is not None else None,
                                        N.C.addressof(cfg) if cfg is not None else None, ts.ctypes.data,
                                        rs.ctypes.data, ms.ctypes.data, counts.ctypes.data)
    N.check(ret >= 0, "cvSolvePnPRansacBatch")
    return [(bool(counts[p] > 0), rs[p].copy(), ts[p].copy(),
             np.flatnonzero(ms[offsets[p]:offsets[p + 1]]).astype(np.int32)) for p in range(B)]


def _pnp_default_cfg() -> N.RansacConfig:
    """cvSolvePnPRansac's configuration at its defaults (pnp_config(100, 8, 0.99, kind))."""
    c = N.RansacConfig()
    c.threshold, c.confidence, c.maxIters, c.method = 8.0, 0.99, 100, N.METHOD_RANSAC
    c.flags = N.FLAG_CV_SAMPLER
    return c


def solvePnP(img, world, K, dist=None, kind: str = "AP3P"):
    """cvSolvePnP -> (ok, rvec, tvec)."""
    pi, pw = _v2d(img), _v3d(world)
    d = _dist4(dist)
    t, r = N.V3d(), N.V3d()
    ok = N.lib().cvSolvePnP(pi.ctypes.data, pw.ctypes.data, pi.shape[0], _m33(K), d.ctypes.data, SOLVER_KIND[kind],
                            N.C.addressof(t), N.C.addressof(r))
    if not ok and N.last_error() and "no pose" not in N.last_error():
        raise N.NativeError(f"cvSolvePnP: {N.last_error()}")
    return bool(ok), np.array([r.X, r.Y, r.Z]), np.array([t.X, t.Y, t.Z])


def _refine(fn, img, world, K, dist, rvec, tvec):
    pi, pw = _v2d(img), _v3d(world)
    d = _dist4(dist)
    t, r = N.V3d(*map(float, tvec)), N.V3d(*map(float, rvec))
    fn(pi.ctypes.data, pw.ctypes.data, pi.shape[0], _m33(K), d.ctypes.data, N.C.addressof(t), N.C.addressof(r))
    if N.last_error():
        raise N.NativeError(N.last_error())
    return np.array([r.X, r.Y, r.Z]), np.array([t.X, t.Y, t.Z])


def refinePnPLM(img, world, K, dist, rvec, tvec):
    """cvRefinePnPLM with the given initial pose -> (rvec, tvec)."""
    return _refine(N.lib().cvRefinePnPLM, img, world, K, dist, rvec, tvec)


def refinePnPVVS(img, world, K, dist, rvec, tvec):
    """cvRefinePnPVVS -> (rvec, tvec)."""
    return _refine(N.lib().cvRefinePnPVVS, img, world, K, dist, rvec, tvec)


REFINE_KIND = {"LM": 0, "VVS": 1}


def solvePnPRansacWithRefine(img, world, K, dist=None, kind: str = "AP3P", refine: str = "LM", iterations: int = 100,
                             reproj_error: float = 8.0, confidence: float = 0.99,
                             params: RansacParams | None = None):
    """solvePnPRansacWithRefine (OpenCV.fs:1051, solvePnPInternal with `ransac` and `refinement`): solvePnPRansac,
    then the inliers gathered in index order (OpenCV.fs:1006-1007), then refinePnPLM / refinePnPVVS on them from
    the RANSAC pose. -> (ok, rvec, tvec, inlier indices); without a pose nothing is refined."""
    fn = {"LM": refinePnPLM, "VVS": refinePnPVVS}[refine]
    ok, r, t, inl = solvePnPRansac(img, world, K, dist, kind, iterations, reproj_error, confidence, params)
    if not ok:
        return ok, r, t, inl
    r, t = fn(_v2d(img)[inl], _v3d(world)[inl], K, dist, r, t)
    return ok, r, t, inl


def _pnp_batch_args(imgs, worlds, Ks, dists):
    """The segmented arrays of a PnP batch call -> (B, offsets, img, world, K, d or None)."""
    if len(imgs) != len(worlds):
        raise ValueError("imgs/worlds length mismatch")
    B = len(imgs)
    pi = [_v2d(x) for x in imgs]
    pw = [_v3d(x) for x in worlds]
    for x, y in zip(pi, pw):
        if x.shape[0] != y.shape[0]:
            raise ValueError("img/world length mismatch")
    offsets = np.zeros(B + 1, dtype=np.int32)
    offsets[1:] = np.cumsum([x.shape[0] for x in pi])
    total = int(offsets[B])
    img = np.ascontiguousarray(np.concatenate(pi, axis=0)) if total else np.zeros((1, 2))
    world = np.ascontiguousarray(np.concatenate(pw, axis=0)) if total else np.zeros((1, 3))
    K = np.ascontiguousarray(np.asarray(Ks, dtype=np.float64).reshape(-1, 9)) if B else np.zeros((1, 9))
    if B and K.shape[0] != B:
        raise ValueError("Ks must have one camera matrix per problem")
    d = None
    if dists is not None:
        d = np.ascontiguousarray(np.asarray(dists, dtype=np.float64).reshape(-1, 4)) if B else np.zeros((1, 4))
        if B and d.shape[0] != B:
            raise ValueError("dists must have one row of 4 coefficients per problem")
    return B, offsets, img, world, K, d


def refinePnPBatch(imgs, worlds, Ks, dists, rvecs, tvecs, kind: str = "LM", masks=None):
    """cvRefinePnPBatch: refinePnPLM / refinePnPVVS (kind "LM" / "VVS") of B problems in one call. imgs / worlds /
    Ks / dists as in solvePnPRansacBatch; rvecs / tvecs: B start poses; masks: None (all points) or B arrays of
    N_p bytes, non-zero = the row takes part (the rows are gathered in index order).
    -> a list of (refined, rvec, tvec): where refined, the pose of the single call on the selected rows; else
    the start pose, and N.last_error() names the first such problem. Raises NativeError when the whole call is
    refused."""
    B, offsets, img, world, K, d = _pnp_batch_args(imgs, worlds, Ks, dists)
    total = int(offsets[B])
    rs = np.zeros((max(B, 1), 3), dtype=np.float64)
    ts = np.zeros((max(B, 1), 3), dtype=np.float64)
    if B:
        rs[:B] = np.asarray(rvecs, dtype=np.float64).reshape(-1, 3)
        ts[:B] = np.asarray(tvecs, dtype=np.float64).reshape(-1, 3)
    m = None
    if masks is not None:
        if len(masks) != B:
            raise ValueError("masks must have one array per problem")
        ms = [np.ascontiguousarray(np.asarray(x)).astype(np.uint8).reshape(-1) for x in masks]
        for p, x in enumerate(ms):
            if x.shape[0] != offsets[p + 1] - offsets[p]:
                raise ValueError("a mask must have one byte per correspondence of its problem")
        m = np.ascontiguousarray(np.concatenate(ms)) if total else np.zeros(1, dtype=np.uint8)
    refined = np.zeros(max(B, 1), dtype=np.uint8)
    ret = N.lib().cvRefinePnPBatch(img.ctypes.data, world.ctypes.data, offsets.ctypes.data, B, K.ctypes.data,
                                   d.ctypes.data if d is not None else None, m.ctypes.data if m is not None else None,
                                   REFINE_KIND[kind], ts.ctypes.data, rs.ctypes.data, refined.ctypes.data)
    N.check(ret >= 0, "cvRefinePnPBatch")
    return [(bool(refined[p]), rs[p].copy(), ts[p].copy()) for p in range(B)]


def solvePnPRansacWithRefineBatch(imgs, worlds, Ks, dists=None, kind: str = "AP3P", refine: str = "LM",
                                  params: RansacParams | None = None):
    """cvSolvePnPRansacRefineBatch: solvePnPRansacWithRefine of B problems in one call (solvePnPRansacBatch, then
    refinePnPBatch on its masks, the points uploaded once). -> a list of (ok, rvec, tvec, inlier indices) per
    problem; a problem without a pose gives (False, zeros, zeros, empty) and is not refined."""
    B, offsets, img, world, K, d = _pnp_batch_args(imgs, worlds, Ks, dists)
    total = int(offsets[B])
    cfg = None
    if params is not None or kind != "Iterative":
        cfg = params.to_c() if params is not None else _pnp_default_cfg()
        cfg.pnpKind = SOLVER_KIND[kind]
    ts = np.zeros((max(B, 1), 3), dtype=np.float64)
    rs = np.zeros((max(B, 1), 3), dtype=np.float64)
    counts = np.zeros(max(B, 1), dtype=np.int32)
    ms = np.zeros(max(total, 1), dtype=np.uint8)
    ret = N.lib().cvSolvePnPRansacRefineBatch(img.ctypes.data, world.ctypes.data, offsets.ctypes.data, B,
                                              K.ctypes.data, d.ctypes.data if d is not None else None,
                                              N.C.addressof(cfg) if cfg is not None else None, REFINE_KIND[refine],
                                              ts.ctypes.data, rs.ctypes.data, ms.ctypes.data, counts.ctypes.data)
    N.check(ret >= 0, "cvSolvePnPRansacRefineBatch")
    return [(bool(counts[p] > 0), rs[p].copy(), ts[p].copy(),
             np.flatnonzero(ms[offsets[p]:offsets[p + 1]]).astype(np.int32)) for p in range(B)]


def solveAp3p(img, world, K):
    """OpenCV.solveAp3p (OpenCV.fs:385-431): 3 points, double arguments (F# `float` is System.Double)
    -> list of (R, t) as the reference returns them (R as stored by ap3p.cpp:245-250)."""
    img = np.asarray(img, dtype=np.float64)
    world = np.asarray(world, dtype=np.float64)
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    Rs, ts = (N.M33d * 4)(), (N.V3d * 4)()
    inv_fx, inv_fy = 1.0 / K[0, 0], 1.0 / K[1, 1]
    args = []
    for i in range(3):
        args += [img[i, 0], img[i, 1], world[i, 0], world[i, 1], world[i, 2]]
    args += [inv_fx, inv_fy, K[0, 2] * inv_fx, K[1, 2] * inv_fy]
    cnt = N.lib().solveAp3p(Rs, ts, *[float(a) for a in args])
    if cnt <= 0 and N.last_error():
        raise N.NativeError(f"solveAp3p: {N.last_error()}")
    return [(np.array(Rs[i].M[:]).reshape(3, 3), np.array([ts[i].X, ts[i].Y, ts[i].Z])) for i in range(max(cnt, 0))]


# ---- device-resident match -> RANSAC hand-off ------------------------------
class Features:
    """A DetectorResult (MiniCVNative.h:23-29) built from keypoint coordinates and descriptors, as
    cvDetectFeatures returns it: KeyPoint2d[N] + row-major descriptors, uint8 or float32. The matching
    calls pick the norm from the element type (uint8 -> Hamming, float32 -> L2) unless told otherwise:
    byte SIFT descriptors are uint8 and must be matched with norm=N.NORM_L2. Keeps the backing arrays
    alive while the struct is in use."""

    def __init__(self, points, descriptors):
        pts = np.asarray(points, dtype=np.float64)
        d = np.ascontiguousarray(descriptors)
        if d.dtype not in (np.uint8, np.float32):
            raise ValueError("descriptors must be uint8 (Hamming, or L2 with norm=NORM_L2) or float32 (L2)")
        n = pts.shape[0]
        self._kp = (N.KeyPoint2d * max(n, 1))()
        for i in range(n):
            self._kp[i].X, self._kp[i].Y = float(pts[i, 0]), float(pts[i, 1])
        self._d = d
        self.struct = N.DetectorResult(n, int(d.size), 0 if d.dtype == np.uint8 else 5,
                                       N.C.cast(self._kp, N.C.c_void_p), d.ctypes.data)


def _mcfg(ratio, cross_check, max_distance, model):
    return N.MatchConfig(float(ratio), int(bool(cross_check)), float(max_distance), int(model))


def matchFeatures(a: Features, b: Features, ratio: float = 0.8, cross_check: bool = False,
                  max_distance: float = 0.0, norm: int = N.NORM_AUTO):
    """cvMatchFeaturesNorm -> (pairs int32 [k][2] (index in a, index in b), dist float32 [k]).
    norm: N.NORM_AUTO (uint8 -> Hamming, float32 -> L2), N.NORM_L2 (uint8 rows too: byte SIFT) or
    N.NORM_HAMMING (uint8 only)."""
    n = a.struct.PointCount
    pairs = np.zeros((max(n, 1), 2), dtype=np.int32)
    dist = np.zeros(max(n, 1), dtype=np.float32)
    cfg = _mcfg(ratio, cross_check, max_distance, N.MODEL_HOMOGRAPHY)
    k = N.lib().cvMatchFeaturesNorm(N.C.addressof(a.struct), N.C.addressof(b.struct), N.C.addressof(cfg), int(norm),
                                    pairs.ctypes.data, dist.ctypes.data, max(n, 1))
    N.check(k >= 0, "cvMatchFeatures")
    return pairs[:k].copy(), dist[:k].copy()


def matchAndFindModel(a: Features, b: Features, model: int = N.MODEL_HOMOGRAPHY, ratio: float = 0.8,
                      cross_check: bool = False, max_distance: float = 0.0, params: RansacParams | None = None,
                      norm: int = N.NORM_AUTO):
    """cvMatchAndFindModelNorm -> (inliers, M 3x3, pairs [k][2], mask bool[k]). norm: as matchFeatures.
    model: N.MODEL_HOMOGRAPHY, N.MODEL_FUNDAMENTAL, N.MODEL_AFFINE or N.MODEL_SIMILARITY (the last two
    return the 2x3 matrix with the third row 0 0 1)."""
    n = a.struct.PointCount
    pairs = np.zeros((max(n, 1), 2), dtype=np.int32)
    mask = np.zeros(max(n, 1), dtype=np.uint8)
    M = N.M33d()
    mc = N.C.c_int(0)
    cfg = _mcfg(ratio, cross_check, max_distance, model)
    rc = (params or (RansacParams() if model == N.MODEL_HOMOGRAPHY else RansacParams(confidence=0.99))).to_c()
    cnt = N.lib().cvMatchAndFindModelNorm(N.C.addressof(a.struct), N.C.addressof(b.struct), N.C.addressof(cfg),
                                          int(norm), N.C.addressof(rc), N.C.addressof(M), pairs.ctypes.data,
                                          mask.ctypes.data, max(n, 1), N.C.addressof(mc))
    N.check(cnt > 0, "cvMatchAndFindModel")
    k = mc.value
    return cnt, np.array(M.M[:]).reshape(3, 3), pairs[:k].copy(), mask[:k] != 0


def _image_batch(images, pairs):
    structs = (N.DetectorResult * max(len(images), 1))(*[f.struct for f in images])
    ip = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    B = ip.shape[0]
    n_img = len(images)
    cap = sum(images[i].struct.PointCount for i in ip[:, 0] if 0 <= i < n_img)   # always enough
    return structs, ip, B, cap


def matchFeaturesBatch(images, pairs, ratio: float = 0.8, cross_check: bool = False, max_distance: float = 0.0,
                       norm: int = N.NORM_AUTO):
    """cvMatchFeaturesBatch: images = a list of Features (uint8 descriptors of one width), pairs = a list of
    (query image, train image) indices. One call for all pairs; every image goes to the device once.
    -> a list of (pairs int32 [k][2], dist float32 [k]) per pair, each equal to matchFeatures(images[i],
    images[j], ...) with the same settings."""
    structs, ip, B, cap = _image_batch(images, pairs)
    out = np.zeros((max(cap, 1), 2), dtype=np.int32)
    dist = np.zeros(max(cap, 1), dtype=np.float32)
    offsets = np.zeros(B + 1, dtype=np.int32)
    cfg = _mcfg(ratio, cross_check, max_distance, N.MODEL_HOMOGRAPHY)
    k = N.lib().cvMatchFeaturesBatch(N.C.addressof(structs), len(images), ip.ctypes.data, B, N.C.addressof(cfg),
                                     int(norm), out.ctypes.data, dist.ctypes.data, cap, offsets.ctypes.data)
    N.check(k >= 0, "cvMatchFeaturesBatch")
    return [(out[offsets[p]:offsets[p + 1]].copy(), dist[offsets[p]:offsets[p + 1]].copy()) for p in range(B)]


def matchAndFindModelBatch(images, pairs, model: int = N.MODEL_HOMOGRAPHY, ratio: float = 0.8,
                           cross_check: bool = False, max_distance: float = 0.0, params: RansacParams | None = None,
                           norm: int = N.NORM_AUTO):
    """cvMatchAndFindModelBatch: matchFeaturesBatch, then findModelBatch(model) on the matched keypoints of
    every pair. -> a list of (count, M 3x3, pairs int32 [k][2], mask bool[k]) per pair; a pair without a
    model gives (0, zeros, its pairs, all-False) and N.last_error() names the first such pair. params None:
    cvFindModelBatch's own defaults."""
    structs, ip, B, cap = _image_batch(images, pairs)
    out = np.zeros((max(cap, 1), 2), dtype=np.int32)
    mask = np.zeros(max(cap, 1), dtype=np.uint8)
    offsets = np.zeros(B + 1, dtype=np.int32)
    models = np.zeros((max(B, 1), 9), dtype=np.float64)
    counts = np.zeros(max(B, 1), dtype=np.int32)
    cfg = _mcfg(ratio, cross_check, max_distance, model)
    rc = params.to_c() if params is not None else None
    ret = N.lib().cvMatchAndFindModelBatch(N.C.addressof(structs), len(images), ip.ctypes.data, B, N.C.addressof(cfg),
                                           int(norm), N.C.addressof(rc) if rc is not None else None, out.ctypes.data,
                                           cap, offsets.ctypes.data, models.ctypes.data, mask.ctypes.data,
                                           counts.ctypes.data)
    N.check(ret >= 0, "cvMatchAndFindModelBatch")
    return [(int(counts[p]), models[p].reshape(3, 3).copy(), out[offsets[p]:offsets[p + 1]].copy(),
             mask[offsets[p]:offsets[p + 1]] != 0) for p in range(B)]


# ---- feature detection: SIFT on the GPU (cvDetectFeatures mode 4) ---------------------
KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                           ("octave", "<i4"), ("class_id", "<i4")])   # KeyPoint2d, 28 bytes


class DetectedFeatures(Features):
    """What cvDetectFeatures returned, copied out of the native result: a Features (so it goes straight
    into matchFeatures(..., norm=N.NORM_L2), matchFeaturesBatch and matchAndFindModel) that also carries
    keypoints (KEYPOINT_DTYPE [n]), points float32 [n][2], size, angle, response, octave and descriptors
    (uint8 or float32 [n][128])."""

    def __init__(self, keypoints, descriptors):
        kp = np.ascontiguousarray(keypoints, dtype=KEYPOINT_DTYPE).reshape(-1)
        n = len(kp)
        d = np.ascontiguousarray(descriptors)
        if d.dtype not in (np.uint8, np.float32):
            raise ValueError("descriptors must be uint8 or float32")
        d = d.reshape(n, -1) if n else d.reshape(0, 128)
        self._kp = (N.KeyPoint2d * max(n, 1))()
        if n:
            N.C.memmove(self._kp, kp.ctypes.data, n * KEYPOINT_DTYPE.itemsize)
        self._d = d
        self.struct = N.DetectorResult(n, int(d.size), 0 if d.dtype == np.uint8 else 5,
                                       N.C.cast(self._kp, N.C.c_void_p), d.ctypes.data)
        self.keypoints = kp
        self.points = np.stack([kp["x"], kp["y"]], axis=1)
        self.size, self.angle, self.response, self.octave = kp["size"], kp["angle"], kp["response"], kp["octave"]
        self.descriptors = d

    def __len__(self):
        return len(self.keypoints)


def _detect_features(export: str, img, mode: int, config) -> DetectedFeatures:
    a = np.ascontiguousarray(img)
    if a.dtype != np.uint8 or a.ndim not in (2, 3):
        raise ValueError("img must be a uint8 array [h][w] or [h][w][c]")
    h, w = a.shape[:2]
    ch = 1 if a.ndim == 2 else a.shape[2]
    L = N.lib()
    p = getattr(L, export)(a.ctypes.data, w, h, ch, int(mode), N.C.addressof(config) if config is not None else None)
    N.check(bool(p), export)
    try:
        r = N.C.cast(p, N.C.POINTER(N.DetectorResult)).contents
        n, f32 = r.PointCount, r.DescriptorElementType == 5
        kp = np.zeros(n, dtype=KEYPOINT_DTYPE)
        d = np.zeros((n, 128), dtype=np.float32 if f32 else np.uint8)
        if n:
            N.C.memmove(kp.ctypes.data, r.Points, kp.nbytes)
            N.C.memmove(d.ctypes.data, r.Descriptors, d.nbytes)
        assert r.DescriptorEntries == 128 * n
    finally:
        L.cvFreeFeatures(p)
    return DetectedFeatures(kp, d)


def detectFeatures(img, mode: int = N.FEATURE_SIFT, config: "N.SiftConfig | None" = None) -> DetectedFeatures:
    """cvDetectFeatures on a uint8 image [h][w] (grey) or [h][w][c] (c = 3, 4: RGB(A)). Only
    mode=N.FEATURE_SIFT is built; config: a N.SiftConfig, or None for cv::SIFT's defaults with byte
    descriptors. Raises N.NativeError where the library returns NULL."""
    return _detect_features("cvDetectFeatures", img, mode, config)


def _image_array(img, what: str):
    a = np.ascontiguousarray(img)
    if a.dtype != np.uint8 or a.ndim not in (2, 3):
        raise ValueError(f"{what} must be a uint8 array [h][w] or [h][w][c]")
    return a


def _copy_out(r) -> DetectedFeatures:
    """A filled native DetectorResult -> DetectedFeatures (the native arrays are copied, not kept)."""
    n, f32 = r.PointCount, r.DescriptorElementType == 5
    kp = np.zeros(n, dtype=KEYPOINT_DTYPE)
    d = np.zeros((n, 128), dtype=np.float32 if f32 else np.uint8)
    if n:
        N.C.memmove(kp.ctypes.data, r.Points, kp.nbytes)
        N.C.memmove(d.ctypes.data, r.Descriptors, d.nbytes)
    assert r.DescriptorEntries == 128 * n
    return DetectedFeatures(kp, d)


def detectFeaturesBatch(images, mode: int = N.FEATURE_SIFT, config: "N.SiftConfig | None" = None) -> list:
    """cvDetectFeaturesBatch: detectFeatures on every image of a list in one call, under one
    config; the images may differ in size and channels. -> a list of DetectedFeatures, element i equal to
    detectFeatures(images[i], mode, config) bit for bit, ready for matchFeaturesBatch and
    matchAndFindModelBatch. Raises N.NativeError where the library fails (one bad image fails the call)."""
    arrays = [_image_array(img, f"images[{i}]") for i, img in enumerate(images)]
    n = len(arrays)
    ims = (N.mcvImage * max(n, 1))()
    for i, a in enumerate(arrays):
        ims[i] = N.mcvImage(a.ctypes.data, a.shape[1], a.shape[0], 1 if a.ndim == 2 else a.shape[2], 0)
    res = (N.DetectorResult * max(n, 1))()
    L = N.lib()
    total = L.cvDetectFeaturesBatch(N.C.addressof(ims), n, int(mode), N.C.addressof(config) if config is not None else None,
                                    N.C.addressof(res))
    try:
        N.check(total >= 0, "cvDetectFeaturesBatch")
        out = [_copy_out(res[i]) for i in range(n)]
        assert sum(len(f) for f in out) == total
    finally:
        L.cvFreeFeaturesBatch(N.C.addressof(res), n)
    return out
