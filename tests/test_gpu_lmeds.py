"""LMedS (method 4) on the GPU (needs an MI355X): the rank kernel against the oracle's exact k-th error
and against its host twin; cvFindHomography / cvFindFundamentalMat with method 4 against lmeds_ref
(bit-exact masks, counts and unrefined models; refined H within the homography suite's 1e-6)."""
import numpy as np
import pytest

import _lmeds_ref as R
from minicv_amd import native as N
from minicv_amd import opencv, synthetic as S

pytestmark = pytest.mark.gpu
REL_TOL = 1e-6   # refined H, as tests/test_gpu_homography.py


def relf(A, B):
    return np.linalg.norm(np.asarray(A) - np.asarray(B)) / np.linalg.norm(B)


def test_rank_kernel_matches_kth_and_host(gpu, native, oracle):
    dev, host = native.lib().mcvTestErrorRank, native.lib().mcvHostErrorRank
    bad = []
    for label, model, kind, pts, models, ranks, exp in R.rank_cases():
        for i, r in enumerate(ranks):
            got = R.run_rank_hook(dev, model, kind, pts, models, r)
            twin = R.run_rank_hook(host, model, kind, pts, models, r)
            for j in range(models.shape[0]):
                if not (R.same_bits(got[j], exp[i, j]) and R.same_bits(got[j], twin[j])):
                    bad.append((label, r, j, float(got[j]), float(exp[i, j]), float(twin[j])))
    assert not bad, bad[:10]


H_CASES = [
    # n, outliers, seed, cv_sampler, fixed_iters, fused, noise sigma
    (5, 0.0, 1, False, False, False, 1e-3),
    (8, 0.2, 2, True, False, False, 1e-3),
    (50, 0.3, 3, False, True, False, 1e-3),
    (200, 0.45, 4, True, False, False, 1e-3),
    (1000, 0.4, 5, False, False, True, 1e-3),
    (5000, 0.45, 6, False, False, False, 1e-3),
    (200, 0.3, 7, False, False, False, 0.0),
    (1000, 0.2, 8, True, True, False, 1e-3),
]


@pytest.mark.parametrize("n,outl,seed,cv,fixed,fused,noise", H_CASES)
def test_find_homography_lmeds(gpu, oracle, n, outl, seed, cv, fixed, fused, noise):
    src, dst, _ = S.homography_problem(n, seed, outlier_frac=outl, sigma=noise)
    pts4 = oracle.pack4(src, dst)
    conf, iters = 0.995, (100 if fixed else 2000)
    ref = R.lmeds_ref(N.MODEL_HOMOGRAPHY, pts4, conf, iters, seed=seed, cv=cv, fixed=fixed, fused=fused)
    assert ref is not None
    if noise == 0.0:
        assert ref["sigma"] == 0.001   # the clamp
    p = dict(confidence=conf, max_iters=iters, method=N.METHOD_LMEDS, seed=seed, cv_sampler=cv, fixed_iters=fixed,
             fused_error=fused)
    cnt, H, mask = opencv.findHomography(src, dst, opencv.RansacParams(refine=False, **p))
    print(f"n={n} niters={ref['niters']} slot={ref['slot']} med={ref['med']} count={cnt} ref={ref['count']}")
    assert cnt == ref["count"]
    np.testing.assert_array_equal(mask, ref["mask"] != 0)
    np.testing.assert_array_equal(H, ref["model"])
    cnt2, H2, mask2 = opencv.findHomography(src, dst, opencv.RansacParams(**p))
    assert cnt2 == cnt
    np.testing.assert_array_equal(mask2, mask)
    _, H_ref, _, _ = oracle.find_homography(src[mask], dst[mask], method=0)
    print(f"refined relf={relf(H2, H_ref):.3e}")
    assert relf(H2, H_ref) < REL_TOL
    # cfg->threshold is not read
    cnt3, H3, mask3 = opencv.findHomography(src, dst, opencv.RansacParams(threshold=1e-9, **p))
    assert cnt3 == cnt2
    np.testing.assert_array_equal(mask3, mask2)
    np.testing.assert_array_equal(H3, H2)


F_CASES = [
    # n, seven_point, error_kind, outliers, seed, cv_sampler
    (9, False, N.FERR_SAMPSON, 0.0, 11, False),
    (50, False, N.FERR_EPIPOLAR, 0.2, 12, True),
    (1000, False, N.FERR_SAMPSON, 0.4, 13, False),
    (1000, False, N.FERR_EPIPOLAR, 0.4, 14, True),
    (8, True, N.FERR_EPIPOLAR, 0.0, 15, True),
    (12, True, N.FERR_EPIPOLAR, 0.1, 16, False),
    (14, True, N.FERR_SAMPSON, 0.1, 17, True),
    (200, True, N.FERR_EPIPOLAR, 0.4, 18, False),
]


@pytest.mark.parametrize("n,seven,ek,outl,seed,cv", F_CASES)
def test_find_fundamental_lmeds(gpu, oracle, n, seven, ek, outl, seed, cv):
    a, b, _, _ = S.fundamental_problem(n, seed=seed, outlier_frac=outl)
    pts4 = oracle.pack4(a, b)
    kind = oracle.f_kind(ek, unfused=True)
    ref = R.lmeds_ref(N.MODEL_FUNDAMENTAL, pts4, 0.99, 1000, seed=seed, cv=cv, kind=kind, seven=seven)
    assert ref is not None
    p = opencv.RansacParams(confidence=0.99, max_iters=1000, method=N.METHOD_LMEDS, seed=seed, cv_sampler=cv,
                            error_kind=ek, seven_point=seven, threshold=123.0)
    cnt, F, mask = opencv.findFundamentalMat(a, b, p)
    print(f"n={n} niters={ref['niters']} slot={ref['slot']} med={ref['med']} count={cnt} ref={ref['count']}")
    assert cnt == ref["count"]
    np.testing.assert_array_equal(mask, ref["mask"] != 0)
    np.testing.assert_array_equal(F, ref["model"])


@pytest.mark.parametrize("n,seven", [(8, False), (7, True)])
def test_minimal_n_takes_the_direct_path(gpu, n, seven):
    a, b, _, _ = S.fundamental_problem(n, seed=21, outlier_frac=0.0)
    base = dict(confidence=0.99, seven_point=seven, error_kind=N.FERR_EPIPOLAR)
    c4, F4, m4 = opencv.findFundamentalMat(a, b, opencv.RansacParams(method=N.METHOD_LMEDS, **base))
    c8, F8, m8 = opencv.findFundamentalMat(a, b, opencv.RansacParams(method=N.METHOD_RANSAC, **base))
    assert c4 == c8 == n and m4.all()
    np.testing.assert_array_equal(F4, F8)
    src, dst, _ = S.homography_problem(4, 22, outlier_frac=0.0)
    c, H4, m = opencv.findHomography(src, dst, opencv.RansacParams(method=N.METHOD_LMEDS))
    _, H8, _ = opencv.findHomography(src, dst, opencv.RansacParams(method=N.METHOD_RANSAC))
    assert c == 4 and m.all()
    np.testing.assert_array_equal(H4, H8)


def test_degenerate_set_fails_with_message(gpu):
    t = np.linspace(-1, 1, 40)
    src = np.stack([t, 2 * t + 0.1], axis=1)   # collinear: no subset passes the check
    for cv in (False, True):
        with pytest.raises(N.NativeError, match="LMedS"):
            opencv.findHomography(src, src * 1.5, opencv.RansacParams(method=N.METHOD_LMEDS, cv_sampler=cv, max_iters=50))


def test_seven_point_ransac_below_15_still_rejected(gpu):
    a, b, _, _ = S.fundamental_problem(12, seed=23, outlier_frac=0.0)
    with pytest.raises(N.NativeError, match="N >= 15"):
        opencv.findFundamentalMat(a, b, opencv.RansacParams(confidence=0.99, seven_point=True))


def test_device_count_two_gives_the_same_result(gpu):
    src, dst, _ = S.homography_problem(300, 24, outlier_frac=0.3)
    p = dict(method=N.METHOD_LMEDS, seed=5)
    c1, H1, m1 = opencv.findHomography(src, dst, opencv.RansacParams(device_count=1, **p))
    c2, H2, m2 = opencv.findHomography(src, dst, opencv.RansacParams(device_count=2, **p))
    assert c1 == c2
    np.testing.assert_array_equal(m1, m2)
    np.testing.assert_array_equal(H1, H2)


def test_other_entry_points_reject_method_4(gpu):
    import torch
    from minicv_amd import device as D
    a, b, *_ = S.essential_problem(50, seed=25)
    with pytest.raises(N.NativeError, match="RANSAC"):
        opencv.findEssentialMat(a, b, 800.0, (640.0, 360.0), opencv.RansacParams(method=N.METHOD_LMEDS, confidence=0.99))
    src, dst, _ = S.homography_problem(50, 26)
    dev = torch.device("cuda:0")
    pts = D.pack_points_tensor(src, dst, dev)
    plan = D.RansacPlan(N.MODEL_HOMOGRAPHY, 50, 64)
    key = torch.zeros(2, dtype=torch.int64, device=dev)
    with pytest.raises(N.NativeError, match="method 4"):
        plan.evaluate(pts, 50, opencv.RansacParams(method=N.METHOD_LMEDS).to_c(), 0, 64, key)
    plan.close()
