"""Helpers shared by tests/test_sift_batch.py and tests/test_gpu_sift_batch.py: the case list,
the raw calls of cvDetectFeaturesBatch and mcvTestSiftBatchPlan, and the comparison with the single call."""
import ctypes as C

import numpy as np

import _sift_ref as R
from minicv_amd import native as N
from minicv_amd import opencv

# the cases of tests/_sift_ref.py with no config override
DEFAULTS = ("blobs", "texture_97x61", "narrow_24x9", "one_pixel", "constant", "rgb", "rgba", "seam_257x33",
            "seam_129x65", "seam_128x32", "tall_9x300", "clamped_radius", "tiled")
assert all(not R.CASES[name][1] for name in DEFAULTS)
GPU = "cvDetectFeatures"


def channels(a):
    return 1 if a.ndim == 2 else a.shape[2]


def image_structs(arrays, reserved=0):
    ims = (N.mcvImage * max(len(arrays), 1))()
    for i, a in enumerate(arrays):
        ims[i] = N.mcvImage(a.ctypes.data, a.shape[1], a.shape[0], channels(a), reserved)
    return ims


def cfg_pointer(cfg):
    return None if cfg is None else C.addressof(cfg)


def plan_raw(ims, n, mode=4, cfg=None):
    """mcvTestSiftBatchPlan on an array of mcvImage -> (rc, out8, error)."""
    out = (C.c_longlong * 8)(*([-7] * 8))
    rc = N.lib().mcvTestSiftBatchPlan(C.addressof(ims) if ims is not None else None, n, mode, cfg_pointer(cfg), out)
    return rc, list(out), N.last_error()


def plan(arrays, **cfg):
    """The plan of a batch of numpy images under cfg overrides -> out8 (asserts success)."""
    rc, out, err = plan_raw(image_structs(arrays), len(arrays), 4, N.SiftConfig.default(**cfg) if cfg else None)
    assert rc == 0, err
    return out


def batch_raw(ims, n, mode=4, cfg=None):
    """cvDetectFeaturesBatch on an array of mcvImage -> (return value, the results array, error). The caller
    frees the results of a call that succeeded."""
    res = (N.DetectorResult * max(n, 1))()
    C.memset(res, 0xff, C.sizeof(res))   # the call must overwrite every struct
    ret = N.lib().cvDetectFeaturesBatch(C.addressof(ims) if ims is not None else None, n, mode, cfg_pointer(cfg),
                                        C.addressof(res))
    return ret, res, N.last_error()


def all_zero(res, n):
    return not any(bytes(res)[:n * C.sizeof(N.DetectorResult)])


def batch_stats():
    st = (C.c_longlong * 8)()
    assert N.lib().mcvTestSiftBatchStats(st) == 0
    return list(st)


def single_stats():
    st = (C.c_longlong * 8)()
    assert N.lib().mcvTestSiftStats(st) == 0
    return list(st)


def batch(arrays, **cfg):
    """detectFeaturesBatch under cfg overrides -> (list of DetectedFeatures, stats8)."""
    got = opencv.detectFeaturesBatch(arrays, config=N.SiftConfig.default(**cfg) if cfg else None)
    return got, batch_stats()


_singles = {}


def single(a, **cfg):
    """The single call on one image, computed once per (image, configuration) and left unchanged
    -> (keypoints, descriptors, stats8[4:])."""
    key = (a.shape, a.tobytes(), tuple(sorted(cfg.items())))
    if key not in _singles:
        f = R.run(GPU, a, cfg or None)
        _singles[key] = (f.keypoints, f.descriptors, single_stats()[4:])
    return _singles[key]


def blob(f):
    return f.keypoints.tobytes(), f.descriptors.tobytes(), f.descriptors.dtype.str


def assert_batch_equals_singles(got, arrays, what, **cfg):
    """Every results[i] bit equal to the single call on that image; -> the sums of the single calls' counts."""
    assert len(got) == len(arrays), what
    total = [0, 0, 0, 0]
    for i, a in enumerate(arrays):
        kp, desc, cnt = single(a, **cfg)
        R.assert_same(got[i], (kp, desc), f"{what}: image {i} ({a.shape[1]} x {a.shape[0]})")
        total = [x + y for x, y in zip(total, cnt)]
    return total
