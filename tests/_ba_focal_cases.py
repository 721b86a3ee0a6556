"""Shared pieces of the focal bundle-adjustment tests (test_bundle_adjust_focal.py,
test_gpu_bundle_adjust_focal.py): the call wrapper of cvBundleAdjustFocal and its twin over _ba_cases'
scenes, the focal scenes, and a numpy restatement of DESIGN §7p's focal update. Nothing here calls the
GPU by itself."""
import ctypes as C
from dataclasses import dataclass, replace

import numpy as np

import _ba_cases as B
from minicv_amd import native as N

SENTINEL = B.SENTINEL


@dataclass
class Focal:
    """A _ba_cases.Case with what the focal export adds."""
    case: B.Case
    mode: int = 1
    group: object = None        # focalGroup[nCameras] or None
    fixedFocal: object = None   # bytes or None

    def config(self, **kw):
        return N.BaFocalConfig.default(self.mode, **dict(self.case.cfg, **kw))


def _ptr(a):
    return None if a is None or a.size == 0 else a.ctypes.data


def arrays(f: Focal):
    c = f.case
    return dict(cams=np.ascontiguousarray(c.cams, np.float64).reshape(-1, 14), idx=np.ascontiguousarray(c.idx, np.int32),
                obs=np.ascontiguousarray(c.obs, np.float64).reshape(-1, 2), off=np.ascontiguousarray(c.off, np.int32),
                pts=np.ascontiguousarray(c.pts, np.float64).reshape(-1, 3),
                fixed=None if c.fixed is None else np.ascontiguousarray(c.fixed, np.uint8),
                group=None if f.group is None else np.ascontiguousarray(f.group, np.int32),
                ff=None if f.fixedFocal is None else np.ascontiguousarray(f.fixedFocal, np.uint8))


def run(export, f: Focal, cfg=None):
    """-> (return value, cameras, points, summary dict); the outputs start sentinel-filled."""
    a = arrays(f)
    cfg = f.config() if cfg is None else cfg
    outC = np.full((max(len(a["cams"]), 1), 14), SENTINEL)
    outP = np.full((max(len(a["pts"]), 1), 3), SENTINEL)
    sm = N.BaFocalSummary()
    sm.base.termination = -9
    sm.freeFocalGroups = -9
    ret = getattr(N.lib(), export)(_ptr(a["cams"]), len(a["cams"]), _ptr(a["fixed"]), _ptr(a["group"]), _ptr(a["ff"]),
                                   _ptr(a["idx"]), _ptr(a["obs"]), a["off"].ctypes.data, len(a["off"]) - 1,
                                   _ptr(a["pts"]), C.addressof(cfg), outC.ctypes.data, outP.ctypes.data,
                                   C.addressof(sm))
    return ret, outC[:len(a["cams"])], outP[:len(a["pts"])], sm.as_dict()


def step(f: Focal, lam):
    """mcvHostBaFocalStep -> (PCG iterations, focalBlocks[n, 2], dCameras[nC, 6], dFocal[nC, 2], dPoints[T, 3])."""
    a = arrays(f)
    cfg = f.config()
    n, nC, T = len(a["idx"]), len(a["cams"]), len(a["pts"])
    u, dc, df, dp = np.full((n, 2), SENTINEL), np.full((nC, 6), SENTINEL), np.full((nC, 2), SENTINEL), np.full((T, 3), SENTINEL)
    it = N.lib().mcvHostBaFocalStep(_ptr(a["cams"]), nC, _ptr(a["fixed"]), _ptr(a["group"]), _ptr(a["ff"]),
                                    _ptr(a["idx"]), _ptr(a["obs"]), a["off"].ctypes.data, T, _ptr(a["pts"]),
                                    C.addressof(cfg), float(lam), u.ctypes.data, dc.ctypes.data, df.ctypes.data,
                                    dp.ctypes.data)
    return it, u, dc, df, dp


def with_focal(cams, params, mode):
    """The numpy restatement of the focal update: params[nC, 2] = (s, unused) in mode 1, (dfx, dfy) in mode 2."""
    out = np.array(cams, float)
    if mode == 1:
        out[:, 12:14] = out[:, 12:14] * (1.0 + params[:, 0:1])
    else:
        out[:, 12:14] = out[:, 12:14] + params
    return out


def off_focal(c: B.Case, factor=1.05) -> B.Case:
    """The case with every camera's focal length off by the factor (the observations stay the truth's)."""
    cams = c.cams.copy()
    cams[:, 12:14] *= factor
    return replace(c, cams=cams)


def convergence_scene():
    """The noise-free ring of _ba_cases' "converge" case with every focal length 5 % off and two cameras
    pose-fixed; points and free cameras start where scene() puts them."""
    return off_focal(B.scene(1, 6, 40, functionTolerance=0.0, cgTolerance=1e-10, maxIterations=50))


def same(a, b):
    """Bit equality of (ret, cameras, points, summary) tuples."""
    return a[0] == b[0] and B.same_bits(a[1], b[1]) and B.same_bits(a[2], b[2]) and a[3] == b[3]


# ---- the named cases of the GPU tests: (a _ba_cases case, its focal lengths off by 3 %, mode, groups) ----

def _groups_257():
    g = np.arange(257, dtype=np.int32)
    g[256] = 255    # cameras 255 and 256 share: the group's chain crosses the 256-camera trip
    return g


def _seg_groups(alone):
    """segment_edges has six cameras, camera 5 without an observation: it shares with camera 4, or is alone
    in a group that so has no used observation at all."""
    return np.array([0, 0, 3, 3, 5, 4 if alone else 5], np.int32)


def _one(n):
    return np.zeros(n, np.int32)


def _named(name, mode, group=None, fixedFocal=None, factor=1.03, **cfg):
    c = B.camera_ring(258) if name == "cameras_258" else B.case(name)
    c = off_focal(c, factor) if factor != 1.0 else c
    if cfg:
        c = replace(c, cfg=dict(c.cfg, **cfg))
    n = len(c.cams)
    group = group(n) if callable(group) else group
    return Focal(c, mode, group, fixedFocal)


FOCAL_CASES = {
    # T at the edges of a block of tracks; one group, two groups, null
    "T63_m1_one": lambda: _named("T63", 1, _one),
    "T64_m2_two": lambda: _named("T64", 2, lambda n: (np.arange(n) % 2).astype(np.int32)),
    "T65_m1_null": lambda: _named("T65", 1),
    "T65_m2_one": lambda: _named("T65", 2, _one),
    # tracks of 65 and 130 observations: the wave form of the per-point sums
    "track_lengths_m1_two": lambda: _named("track_lengths", 1, lambda n: (np.arange(n) % 2).astype(np.int32)),
    "track_lengths_m2_null": lambda: _named("track_lengths", 2),
    # cameras with kBaSeg - 1, kBaSeg, kBaSeg + 1 observations; a group with an unobserved camera, and one
    # with no used observation at all
    "segments_m1_shared_empty": lambda: _named("segment_edges", 1, _seg_groups(False)),
    "segments_m2_shared_empty": lambda: _named("segment_edges", 2, _seg_groups(False)),
    "segments_m1_alone_empty": lambda: _named("segment_edges", 1, _seg_groups(True)),
    "segments_m2_fixed_group": lambda: _named("segment_edges", 2, _seg_groups(True),
                                              np.array([0, 0, 1, 0, 0, 0], np.uint8)),
    # a group of cameras 255 and 256 of 257; 257 free groups of 258 cameras (groups 0 and 256 share a lane)
    "cameras_257_m1_pair": lambda: _named("cameras_257", 1, _groups_257()),
    "cameras_257_m2_pair": lambda: _named("cameras_257", 2, _groups_257()),
    "cameras_258_m1_null": lambda: _named("cameras_258", 1),
    "cameras_258_m2_null": lambda: _named("cameras_258", 2),
    "cameras_257_m1_one": lambda: _named("cameras_257", 1, _one),
    # Huber on and off, rejected steps
    "huber_on_m1": lambda: _named("huber_on", 1, _one),
    "huber_off_m2": lambda: _named("huber_off", 2, _one),
    "rejected_m2": lambda: _named("rejected", 2, _one),
    "rejected_m1_null": lambda: _named("rejected", 1),
    # the termination codes with free focal lengths
    "term_function": lambda: _named("term_function", 1, _one),
    "term_iterations": lambda: _named("term_iterations", 2),
    "term_zero_cost": lambda: _named("term_zero_cost", 1, _one, factor=1.0),
    "term_lambda": lambda: _named("term_lambda", 2, _one),
    "term_nothing": lambda: _named("term_nothing", 1),
}

_focal_cache = {}


def focal_case(name) -> Focal:
    if name not in _focal_cache:
        _focal_cache[name] = FOCAL_CASES[name]()
    return _focal_cache[name]


_twin_cache = {}


def twin_of(name):
    """The twin's result of a named case, computed once and left unchanged."""
    if name not in _twin_cache:
        _twin_cache[name] = run("mcvHostBundleAdjustFocal", focal_case(name))
    return _twin_cache[name]
