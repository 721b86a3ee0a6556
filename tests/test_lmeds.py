"""LMedS (method 4), CPU side: the host twin of the rank kernel (mcvHostErrorRank: the kernel's three
radix passes run sequentially) against the oracle's exact k-th error, the constant and the bindings."""
import numpy as np
import pytest

import _lmeds_ref as R
from minicv_amd import native as N
from minicv_amd import opencv, synthetic as S


def test_method_constant_and_hooks_exported(native):
    assert N.METHOD_LMEDS == 4
    L = native.lib()
    for name in ("mcvTestErrorRank", "mcvHostErrorRank"):
        assert name in N.SIGNATURES and getattr(L, name) is not None
    assert opencv.RansacParams(method=N.METHOD_LMEDS).to_c().method == 4


def test_host_rank_matches_kth(native, oracle):
    fn = native.lib().mcvHostErrorRank
    bad = []
    for label, model, kind, pts, models, ranks, exp in R.rank_cases():
        for i, r in enumerate(ranks):
            got = R.run_rank_hook(fn, model, kind, pts, models, r)
            for j in range(models.shape[0]):
                if not R.same_bits(got[j], exp[i, j]):
                    bad.append((label, r, j, float(got[j]), float(exp[i, j])))
    assert not bad, bad[:10]


def test_crafted_models_give_nan_and_inf(native, oracle):
    """The reference itself sees the NaN class (rank past the finite errors) and +inf medians."""
    seen_nan = seen_inf = False
    for label, model, kind, pts, models, ranks, exp in R.rank_cases():
        if "-x1-" in label:
            seen_nan |= bool(np.isnan(exp).any())
            seen_inf |= bool(np.isinf(exp).any())
    assert seen_nan and seen_inf


def test_host_rank_rejects_bad_arguments(native):
    L = native.lib()
    pts = np.zeros((4, 4), np.float32)
    m = np.zeros((1, 8), np.float32)
    v = np.zeros(1, np.float32)
    for model, kind, rank in ((N.MODEL_HOMOGRAPHY, 0, 4), (N.MODEL_HOMOGRAPHY, 0, -1), (N.MODEL_HOMOGRAPHY, 2, 0),
                              (N.MODEL_ESSENTIAL, 0, 0)):
        assert L.mcvHostErrorRank(model, pts.ctypes.data, 4, m.ctypes.data, 1, kind, rank, v.ctypes.data) == 0
        assert "mcvHostErrorRank" in native.last_error()


def test_lmeds_fails_loudly_without_gpu(native):
    if native.lib().mcvDeviceCount() > 0:
        pytest.skip("a GPU is visible")
    src, dst, _ = S.homography_problem(50, 1)
    with pytest.raises(N.NativeError, match="no HIP device"):
        opencv.findHomography(src, dst, opencv.RansacParams(method=N.METHOD_LMEDS))
    a, b, _, _ = S.fundamental_problem(50, 4)
    with pytest.raises(N.NativeError, match="no HIP device"):
        opencv.findFundamentalMat(a, b, opencv.RansacParams(method=N.METHOD_LMEDS, confidence=0.99))
