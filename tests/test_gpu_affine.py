"""GPU tests of the affine family (cvEstimateAffine2D / cvEstimateAffinePartial2D, MCV_MODEL_AFFINE /
MCV_MODEL_SIMILARITY): the packed inlier sweep, the generate kernel, the LMedS rank kernel, the exports
end to end and the match -> model pipeline, against the numpy restatement (tests/_affine_ref.py) and the
host twins. Counts, masks and unrefined models are exact; refined models are within 1e-6 relative of the
host refine with sequential sums and within the lstsq bound of tests/_affine_ref.py."""
import functools

import numpy as np
import pytest

import _affine_ref as R
from minicv_amd import native as N
from minicv_amd import opencv

pytestmark = pytest.mark.gpu

MODEL_NAME = {N.MODEL_AFFINE: "affine", N.MODEL_SIMILARITY: "similarity"}
K = N.A_SWEEP_K
REL_TOL = 1e-6


# ---- the packed sweep on given models --------------------------------------------------------------
def _sweep(pts4, models, thr2, fused):
    counts = np.full(models.shape[0], -7, dtype=np.int32)
    ok = N.lib().mcvTestAffineSweep(pts4.ctypes.data, pts4.shape[0], models.ctypes.data, models.shape[0],
                                    float(thr2), int(fused), counts.ctypes.data)
    assert ok == 1, N.last_error()
    return counts


def _sweep_points(n, rng):
    """Integer-valued correspondences (every operation of the error is exact): dst = src + (3, 4) for every
    third one, the first included (error exactly 25 under the identity, 0 under the shift), + (3, 5) for
    the next, + 0 for the third."""
    src = rng.integers(-50, 50, (n, 2)).astype(np.float32)
    off = np.array([[3, 4], [3, 5], [0, 0]], dtype=np.float32)[np.arange(n) % 3]
    return np.ascontiguousarray(np.concatenate([src, src + off], 1))


def _sweep_models(count, rng):
    base = [R.IDENTITY,                                                     # errors 25 (== thr2), 34, 0
            np.array([np.nan, 0, 0, 0, 1, 0], dtype=np.float32),             # NaN model
            np.array([np.inf, 0, 0, 0, 1, 0], dtype=np.float32),             # inf model
            np.array([1, 0, 3, 0, 1, 4], dtype=np.float32),                  # errors 0, 1, 25
            np.array([1, 0, 0, 0, 1, -1], dtype=np.float32)]                 # errors 34, 45, 1
    ms = [base[i % len(base)] if i < 2 * len(base) else rng.normal(0, 1, 6).astype(np.float32) for i in range(count)]
    return np.ascontiguousarray(np.stack(ms))


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 127, 128, 129, 257, 1000, 4099])
def test_sweep_counts_exact(gpu, n):
    rng = np.random.default_rng(n)
    pts4 = _sweep_points(n, rng)
    real, _, A = R.scene(N.MODEL_AFFINE, n, 300 + n)
    for nm in (1, K - 1, K, K + 1, 4 * K + 1):
        models = _sweep_models(nm, rng)
        near = np.ascontiguousarray(models.copy())
        near[-1] = A.ravel().astype(np.float32)
        for fused in (0, 1):
            exp = np.array([R.count(pts4, m, 25.0, bool(fused)) for m in models], dtype=np.int32)
            np.testing.assert_array_equal(_sweep(pts4, models, 25.0, fused), exp)
            exp = np.array([R.count(real, m, 4.0, bool(fused)) for m in near], dtype=np.int32)
            np.testing.assert_array_equal(_sweep(real, near, 4.0, fused), exp)
    # the ties are there: the identity counts the error-25 points as inliers at thr2 = 25
    e = R.errors(pts4, R.IDENTITY)
    assert e[0] == 25 and R.count(pts4, R.IDENTITY, 25.0) == int((e <= 25).sum()) > int((e < 25).sum())


@pytest.mark.parametrize("n", [65, 1000])
def test_sweep_subnormal_products(gpu, n):
    rng = np.random.default_rng(5)
    pts4 = R.subnormal_set(n, rng)
    models = np.ascontiguousarray(np.stack([R.IDENTITY] * (K + 1)))
    e = R.errors(pts4, R.IDENTITY)
    sub = (e > 0) & (e < np.float32(2.0**-126))
    assert sub.sum() > n // 2
    thr2 = float(np.sort(e[sub])[sub.sum() // 2])   # a subnormal threshold: inliers on both sides of it
    for fused in (0, 1):
        exp = R.count(pts4, R.IDENTITY, thr2, bool(fused))
        assert 0 < exp < n
        np.testing.assert_array_equal(_sweep(pts4, models, thr2, fused), np.full(K + 1, exp, dtype=np.int32))


# ---- generated hypotheses ------------------------------------------------------------------------
GEN_N, GEN_MAX, GEN_THR = 1000, 4097, 2.0


@functools.lru_cache(maxsize=None)
def _gen_reference(model, cv):
    """Statuses / counts of hypotheses [0, GEN_MAX) from the restatement, once per (model, sampler)."""
    pts4, _, _ = R.scene(model, GEN_N, 77, outlier_frac=0.4)
    samples = R.Samples(model, pts4, seed=4242, cv=cv, rows=GEN_MAX)
    thr2 = float(np.float32(GEN_THR * GEN_THR))
    out = np.empty(GEN_MAX, dtype=np.int32)
    for h in range(GEN_MAX):
        st, _, Af, _ = R.hypothesis(model, pts4, samples, h)
        out[h] = R.count(pts4, Af, thr2) if st == 1 else st
    return pts4, out


@pytest.fixture(scope="module")
def torch_dev(gpu):
    import torch
    return torch, torch.device("cuda:0")


@pytest.mark.parametrize("cv", [False, True], ids=["philox", "cv"])
@pytest.mark.parametrize("model", R.MODELS, ids=MODEL_NAME.get)
def test_generated_counts_exact(torch_dev, model, cv):
    torch, dev = torch_dev
    from minicv_amd import device as D
    pts4, ref = _gen_reference(model, cv)
    d_pts = torch.from_numpy(pts4).to(dev)
    cfg = opencv.RansacParams(threshold=GEN_THR, max_iters=GEN_MAX, seed=4242, cv_sampler=cv).to_c()
    for count in (1, 63, 64, 65, 1000, 4097):
        plan = D.RansacPlan(model, GEN_N, count)
        key = torch.zeros(2, dtype=torch.int64, device=dev)
        counts = torch.full((count,), -9, dtype=torch.int32, device=dev)
        plan.evaluate(d_pts, GEN_N, cfg, 0, count, key, counts)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(counts.cpu().numpy(), ref[:count])
        c, h = D.unpack_key(int(key.cpu()[0]))
        best = int(ref[:count].max())
        if best >= R.model_points(model):
            assert (c, h) == (best, int(np.argmax(ref[:count] == best)))
        plan.close()


# ---- the rank kernel -----------------------------------------------------------------------------
def test_error_rank_equals_host_twin(gpu):
    for label, fused, pts4, models, ranks, exp in R.rank_cases():
        for i, r in enumerate(ranks):
            model = R.MODELS[i % 2]
            got = R.run_rank_hook(N.lib().mcvTestErrorRank, model, fused, pts4, models, r)
            host = R.run_rank_hook(N.lib().mcvHostErrorRank, model, fused, pts4, models, r)
            for j in range(models.shape[0]):
                assert R.same_bits(got[j], host[j]), (label, r, j, got[j], host[j])
                assert R.same_bits(got[j], exp[i, j]), (label, r, j, got[j], exp[i, j])


# ---- end to end ----------------------------------------------------------------------------------
def _call(model, pts4, params):
    fn = opencv.estimateAffine2D if model == N.MODEL_AFFINE else opencv.estimateAffinePartial2D
    return fn(pts4[:, :2].astype(np.float64), pts4[:, 2:].astype(np.float64), params)


E2E = [(n, frac) for n in (20, 500, 5000) for frac in (0.3, 0.6)]


@pytest.mark.parametrize("cv", [False, True], ids=["philox", "cv"])
@pytest.mark.parametrize("method", [N.METHOD_RANSAC, N.METHOD_LMEDS], ids=["ransac", "lmeds"])
@pytest.mark.parametrize("n,frac", E2E)
@pytest.mark.parametrize("model", R.MODELS, ids=MODEL_NAME.get)
def test_end_to_end_vs_restatement(gpu, model, n, frac, method, cv):
    m = R.model_points(model)
    seed = 1000 * n + int(frac * 10)
    pts4, _, _ = R.scene(model, n, seed, outlier_frac=frac)
    thr, conf, iters = 2.0, 0.99, 2000
    if method == N.METHOD_RANSAC:
        ref = R.ransac_ref(model, pts4, thr, conf, iters, seed=seed, cv=cv)
    else:
        ref = R.lmeds_ref(model, pts4, conf, iters, seed=seed, cv=cv)
    p = opencv.RansacParams(threshold=thr, confidence=conf, max_iters=iters, method=method, seed=seed,
                            cv_sampler=cv, refine=False)
    if ref is None:
        with pytest.raises(N.NativeError):
            _call(model, pts4, p)
        return
    A, mask, cnt = _call(model, pts4, p)
    assert cnt == ref["count"]
    np.testing.assert_array_equal(mask, ref["mask"].astype(bool))
    np.testing.assert_array_equal(A.ravel().view(np.uint64), ref["A"].view(np.uint64))   # the closed form's bits
    p.refine = True
    A2, mask2, cnt2 = _call(model, pts4, p)
    assert cnt2 == cnt
    np.testing.assert_array_equal(mask2, mask)
    if cnt > m:
        host = R.host_refine(model, pts4, ref["mask"], ref["A"])
        dev_host = R.rel(A2, host)
        dev_lstsq = R.rel(A2, R.lstsq_model(model, pts4, ref["mask"]))
        print(f"refined: vs host twin {dev_host:.3e}, vs lstsq {dev_lstsq:.3e}")
        assert dev_host < REL_TOL
        assert dev_lstsq <= R.LSTSQ_BOUND
        assert R.cost(pts4, ref["mask"], A2.ravel()) <= R.cost(pts4, ref["mask"], ref["A"])
    else:
        np.testing.assert_array_equal(A2, A)


@pytest.mark.parametrize("model", R.MODELS, ids=MODEL_NAME.get)
def test_fused_error_end_to_end(gpu, model):
    pts4, _, _ = R.scene(model, 500, 31, outlier_frac=0.4)
    ref = R.ransac_ref(model, pts4, 2.0, 0.99, 500, seed=9, fused=True)
    p = opencv.RansacParams(threshold=2.0, confidence=0.99, max_iters=500, seed=9, fused_error=True, refine=False)
    A, mask, cnt = _call(model, pts4, p)
    assert cnt == ref["count"]
    np.testing.assert_array_equal(mask, ref["mask"].astype(bool))
    np.testing.assert_array_equal(A.ravel().view(np.uint64), ref["A"].view(np.uint64))


# ---- edge cases ----------------------------------------------------------------------------------
@pytest.mark.parametrize("model", R.MODELS, ids=MODEL_NAME.get)
def test_too_few_and_exactly_enough_points(gpu, model):
    m = R.model_points(model)
    pts4, _, _ = R.scene(model, m, 5, outlier_frac=0.0)
    with pytest.raises(N.NativeError, match=f"at least {m}"):
        _call(model, pts4[: m - 1], None)
    for method in (N.METHOD_RANSAC, N.METHOD_LMEDS):
        A, mask, cnt = _call(model, pts4, opencv.RansacParams(method=method))
        assert cnt == m and mask.all()
        st, A_ref, _ = R.solve(model, pts4, list(range(m)))
        assert st == 1
        np.testing.assert_array_equal(A.ravel().view(np.uint64), A_ref.view(np.uint64))


def test_all_collinear_affine_returns_zero(gpu):
    t = np.arange(40) * 2.0   # exact in float32: every triple is collinear after the conversion too
    src = np.ascontiguousarray(np.stack([t, 2 * t + 1], 1))
    A = np.zeros(6)
    mask = np.ones(40, dtype=np.uint8)
    for n in (40, 3):
        for flags in (0, N.FLAG_CV_SAMPLER):
            cfg = N.RansacConfig(2.0, 0.99, 50, N.METHOD_RANSAC, 3, 1, flags, 0, 0)
            cnt = N.lib().cvEstimateAffine2D(src.ctypes.data, src.ctypes.data, n, N.C.addressof(cfg), A.ctypes.data,
                                             mask.ctypes.data)
            assert cnt == 0 and N.last_error()
    assert not mask[:3].any()


@pytest.mark.parametrize("model", R.MODELS, ids=MODEL_NAME.get)
def test_device_count_8_equals_1(gpu, model):
    pts4, _, _ = R.scene(model, 3000, 12, outlier_frac=0.5)
    outs = []
    for dc in (1, 8):
        for fixed in (False, True):
            p = opencv.RansacParams(threshold=2.0, confidence=0.99, max_iters=3000, seed=5, device_count=dc,
                                    fixed_iters=fixed)
            outs.append((dc, fixed, _call(model, pts4, p)))
    for fixed in (False, True):
        (A1, m1, c1), (A8, m8, c8) = [o[2] for o in outs if o[1] == fixed]
        assert c1 == c8
        np.testing.assert_array_equal(m1, m8)
        np.testing.assert_array_equal(A1, A8)


@pytest.mark.parametrize("model", R.MODELS, ids=MODEL_NAME.get)
def test_null_config_takes_opencv_defaults(gpu, model):
    pts4, _, _ = R.scene(model, 800, 8, outlier_frac=0.4)
    a = np.ascontiguousarray(pts4[:, :2], dtype=np.float64)
    b = np.ascontiguousarray(pts4[:, 2:], dtype=np.float64)
    A = np.zeros(6)
    mask = np.zeros(800, dtype=np.uint8)
    fn = N.lib().cvEstimateAffine2D if model == N.MODEL_AFFINE else N.lib().cvEstimateAffinePartial2D
    cnt = fn(a.ctypes.data, b.ctypes.data, 800, None, A.ctypes.data, mask.ctypes.data)
    ref = R.ransac_ref(model, pts4, 3.0, 0.99, 2000, cv=True)
    assert cnt == ref["count"] > 0
    np.testing.assert_array_equal(mask, ref["mask"])
    host = R.host_refine(model, pts4, ref["mask"], ref["A"])   # refine on by default
    assert R.rel(A, host) < REL_TOL and not np.array_equal(A, ref["A"])


# ---- pipeline ------------------------------------------------------------------------------------
def _feature_pair(model, kind, seed, n=300):
    """300 x 300 keypoints with planted matches (80 % follow the scene's transform) and byte descriptors:
    32-byte binary rows (a few flipped bits) or 128-byte SIFT-like rows (small noise)."""
    from minicv_amd import synthetic as S
    rng = np.random.default_rng(seed)
    src, dst, _, _ = S.affine_problem(n, seed, outlier_frac=0.2, similarity=model == N.MODEL_SIMILARITY)
    perm = rng.permutation(n)
    pb = np.empty_like(dst)
    pb[perm] = dst
    if kind == "hamming":
        da = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        flip = np.zeros((n, 32), dtype=np.uint8)
        flip[np.arange(n), rng.integers(0, 32, n)] = 1 << rng.integers(0, 8, n)
        d = da ^ flip
    else:
        da = np.clip(np.abs(rng.normal(0, 40, (n, 128))), 0, 255).astype(np.uint8)
        d = np.clip(da.astype(np.int32) + rng.integers(-2, 3, (n, 128)), 0, 255).astype(np.uint8)
    db = np.empty_like(d)
    db[perm] = d
    return src, da, pb, db


@pytest.mark.parametrize("kind", ["hamming", "l2u8"])
@pytest.mark.parametrize("model", R.MODELS, ids=MODEL_NAME.get)
def test_pipeline_equals_match_then_estimate(gpu, model, kind):
    pa, da, pb, db = _feature_pair(model, kind, 40 + model)
    norm = N.NORM_AUTO if kind == "hamming" else N.NORM_L2
    Fa, Fb = opencv.Features(pa, da), opencv.Features(pb, db)
    p = opencv.RansacParams(threshold=2.0, confidence=0.99, max_iters=1000, seed=6)
    cnt, M, pairs, mask = opencv.matchAndFindModel(Fa, Fb, model=model, ratio=0.8, cross_check=True, params=p,
                                                   norm=norm)
    pairs2, _ = opencv.matchFeatures(Fa, Fb, ratio=0.8, cross_check=True, norm=norm)
    np.testing.assert_array_equal(pairs, pairs2)
    assert len(pairs) > 200
    src = pa[pairs[:, 0]].astype(np.float32).astype(np.float64)
    dst = pb[pairs[:, 1]].astype(np.float32).astype(np.float64)
    fn = opencv.estimateAffine2D if model == N.MODEL_AFFINE else opencv.estimateAffinePartial2D
    A, mask2, cnt2 = fn(src, dst, p)
    assert cnt == cnt2 > 100
    np.testing.assert_array_equal(mask, mask2)
    np.testing.assert_array_equal(M[:2], A)
    np.testing.assert_array_equal(M[2], [0.0, 0.0, 1.0])
