"""What the four 2-D exports (cvFindHomography, cvFindFundamentalMat, cvEstimateAffine2D,
cvEstimateAffinePartial2D) refuse before they look for a device: the message, byte for byte, and the caller's
mask zeroed by then. No GPU is needed: every case is refused ahead of require_device."""
import ctypes as C

import numpy as np
import pytest

from minicv_amd import native

# export -> (minimal sample size, a method number it does not support)
EXPORTS = {
    "cvFindHomography": (4, 5),
    "cvFindFundamentalMat": (8, 5),
    "cvEstimateAffine2D": (3, native.METHOD_LSQ),
    "cvEstimateAffinePartial2D": (2, native.METHOD_LSQ),
}
F = "cvFindFundamentalMat"


def config(method=native.METHOD_RANSAC, confidence=0.99, flags=0):
    return native.RansacConfig(3.0, confidence, 100, method, 1, 1, flags, 0, 0)


def refused(name, n, cfg=None, null_model=False):
    """Calls the export on n correspondences with a mask of 0xFF; returns (message, mask)."""
    rng = np.random.default_rng(7)
    a = np.ascontiguousarray(rng.uniform(0, 100, (max(n, 1), 2)))
    b = np.ascontiguousarray(rng.uniform(0, 100, (max(n, 1), 2)))
    model = np.full(9, -1.0)
    mask = np.full(max(n, 1), 0xFF, np.uint8)
    r = getattr(native.lib(), name)(a.ctypes.data, b.ctypes.data, n, C.addressof(cfg) if cfg is not None else None,
                                    None if null_model else model.ctypes.data, mask.ctypes.data)
    assert r == 0
    assert np.all(model == -1.0)
    return native.last_error(), mask[:n]


@pytest.mark.parametrize("name", EXPORTS)
def test_null_model(name):
    msg, _ = refused(name, 16, config(), null_model=True)
    assert msg == f"{name}: null argument or negative N"


@pytest.mark.parametrize("name", EXPORTS)
def test_below_minimal_sample(name):
    m = EXPORTS[name][0]
    for cfg in (None, config()):
        msg, mask = refused(name, m - 1, cfg)
        assert msg == f"{name}: need at least {m} correspondences (N={m - 1})"
        assert not mask.any()


@pytest.mark.parametrize("name", EXPORTS)
def test_unsupported_method(name):
    method = EXPORTS[name][1]
    msg, mask = refused(name, 16, config(method=method))
    assert msg == f"{name}: unsupported method {method}"
    assert not mask.any()


@pytest.mark.parametrize("name", EXPORTS)
@pytest.mark.parametrize("confidence", [0.0, 1.0])
def test_confidence_outside_open_interval(name, confidence):
    for method in (native.METHOD_RANSAC, native.METHOD_LMEDS):
        msg, mask = refused(name, 16, config(method=method, confidence=confidence))
        assert msg == f"{name}: confidence must be in (0,1)"
        assert not mask.any()


def test_seven_point_rules():
    seven = native.FLAG_SEVEN_POINT
    # FM_RANSAC with the 7-point solver below 15 points (and not exactly 7) is refused first, whatever N
    for n in (6, 14):
        msg, mask = refused(F, n, config(flags=seven))
        assert msg == (f"{F}: 7-point FM_RANSAC needs N >= 15 (OpenCV uses LMeDS below that: use method 4; "
                       f"N={n})")
        assert not mask.any()
    # the minimal sample is 7 with the flag (LMedS reaches that check), 8 without
    msg, mask = refused(F, 6, config(method=native.METHOD_LMEDS, flags=seven))
    assert msg == f"{F}: need at least 7 correspondences (N=6)"
    assert not mask.any()
    msg, mask = refused(F, 7, config(method=native.METHOD_LMEDS))
    assert msg == f"{F}: need at least 8 correspondences (N=7)"
    assert not mask.any()
    # the method and confidence refusals come after the 7-point ones
    msg, _ = refused(F, 16, config(method=5, flags=seven))
    assert msg == f"{F}: unsupported method 5"
    msg, _ = refused(F, 16, config(confidence=1.0, flags=seven))
    assert msg == f"{F}: confidence must be in (0,1)"


def test_retired_flag_before_method():
    # check_flags runs before the method refusal in every export
    for name in EXPORTS:
        msg, mask = refused(name, 16, config(method=EXPORTS[name][1], flags=4))
        assert msg.startswith(f"{name}: flag bit 4 is retired")
        assert not mask.any()
