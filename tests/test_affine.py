"""estimateAffine2D / estimateAffinePartial2D on the CPU: the host-compiled twin of the per-hypothesis
device code (hyp_affine.h), OpenCV's sample stream for 2- and 3-point samples, the LMedS rank twin and
the refine's host twin, each against the independent numpy restatement (tests/_affine_ref.py). No GPU."""
import ctypes as C

import numpy as np
import pytest

import _affine_ref as R
from minicv_amd import native as N

MODEL_NAME = {N.MODEL_AFFINE: "affine", N.MODEL_SIMILARITY: "similarity"}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


_HYP_CASES = [(mo, n) for mo in R.MODELS for n in R.SIZES if n >= R.model_points(mo)]


@pytest.mark.parametrize("model,n", _HYP_CASES, ids=[f"{MODEL_NAME[mo]}-n{n}" for mo, n in _HYP_CASES])
def test_host_hypothesis_bit_exact_vs_restatement(native, model, n):
    """Status, fp64 model and fp32 model of 200 Philox hypotheses, bit for bit (N = 2 is below the affine
    sample size: test_size_below_sample_rejected)."""
    m = R.model_points(model)
    pts4, _, _ = R.scene(model, n, 7 + n)
    seed = 1234 + n
    solved = 0
    for hyp in list(range(198)) + [2**31 + 5, 2**32 - 1]:
        st, A, Af, idx = R.host_hypothesis(model, pts4, seed, hyp)
        assert st in (1, -1, -2)
        if st == -2:
            continue
        assert len(set(idx.tolist())) == m and (idx >= 0).all() and (idx < n).all()
        assert m == 2 or R.check_subset(pts4, idx)
        st2, A2, Af2 = R.solve(model, pts4, idx)
        assert st == st2
        if st == 1:
            solved += 1
            np.testing.assert_array_equal(_bits(A), _bits(A2))
            np.testing.assert_array_equal(_bits(Af), _bits(Af2))
    assert solved > 0


@pytest.mark.parametrize("model", R.MODELS, ids=MODEL_NAME.get)
def test_duplicated_point_pair_gives_no_model(native, model):
    """Every correspondence equal: the similarity's d = 1 / 0 (no model); the affine subset check rejects
    every sample (no sample)."""
    pts4 = np.ascontiguousarray(np.tile(np.array([[3.0, 4.0, 5.0, 6.0]], dtype=np.float32), (10, 1)))
    for hyp in range(20):
        st, _, _, idx = R.host_hypothesis(model, pts4, 99, hyp)
        if model == N.MODEL_SIMILARITY:
            assert st == -1
            assert R.solve(model, pts4, idx)[0] == -1
        else:
            assert st == -2


def test_size_below_sample_rejected(native):
    pts4 = np.zeros((1, 4), dtype=np.float32)
    A, Af = np.zeros(9), np.zeros(9, dtype=np.float32)
    for model in R.MODELS:
        st = N.lib().mcvHostHypothesis(model, pts4.ctypes.data, 1, 0, 0, A.ctypes.data, Af.ctypes.data, None)
        assert st < -2 and "N <" in N.last_error()


def _native_subsets(model, m, pts4, n, rows):
    out = np.zeros((max(rows, 1), m), dtype=np.int32)
    k = N.lib().mcvCvSubsets(model, m, 0 if pts4 is None else pts4.ctypes.data, n, rows, out.ctypes.data)
    assert k >= 0, N.last_error()
    return int(k), out[:rows]


@pytest.mark.parametrize("model", R.MODELS, ids=MODEL_NAME.get)
@pytest.mark.parametrize("kind", ["random", "grid", "line_heavy"])
def test_cv_subsets_vs_python_stream(native, model, kind):
    rng = np.random.default_rng(21)
    n = 400
    if kind == "random":
        p = rng.uniform(-1, 1, (n, 4))
    elif kind == "grid":
        g = np.stack(np.meshgrid(np.arange(20), np.arange(20)), -1).reshape(-1, 2) / 10.0 - 1
        p = np.concatenate([g, g[rng.permutation(n)]], 1)
    else:
        t = rng.uniform(-1, 1, n)
        p = np.stack([t, 0.5 * t + 0.1, rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)], 1)
        p[::10, 1] += rng.uniform(-1, 1, n // 10)
    pts4 = np.ascontiguousarray(p, dtype=np.float32)
    m = R.model_points(model)
    rows = 300
    k, got = _native_subsets(model, m, pts4, n, rows)
    k2, ref = R.cv_subsets(model, pts4, n, rows)
    assert k == k2 == rows
    np.testing.assert_array_equal(got, ref)


def test_cv_subsets_all_collinear_affine(native):
    n = 50
    t = np.linspace(-1, 1, n)
    pts4 = np.ascontiguousarray(np.stack([t, t, t, -t], 1), dtype=np.float32)
    k, got = _native_subsets(N.MODEL_AFFINE, 3, pts4, n, 3)
    assert k == 0 and (got == -1).all()
    assert R.cv_subsets(N.MODEL_AFFINE, pts4, n, 3, max_attempts=300)[0] == 0
    # the 2-point check is vacuous
    k, got = _native_subsets(N.MODEL_SIMILARITY, 2, None, n, 3)
    assert k == 3 and (got >= 0).all()


def test_host_error_rank_vs_restatement(native):
    """Ranks 0, N / 2, N - 1 at every size: spread, all-equal, NaN and subnormal errors, both error kinds,
    under both model ids (one stored model)."""
    sub = 0
    for label, fused, pts4, models, ranks, exp in R.rank_cases():
        if label.startswith("subnormal"):
            e = R.errors(pts4, R.IDENTITY)
            sub += int(((e > 0) & (e < np.float32(2.0**-126))).sum())
        for i, r in enumerate(ranks):
            for model in R.MODELS:
                got = R.run_rank_hook(N.lib().mcvHostErrorRank, model, fused, pts4, models, r)
                for j in range(models.shape[0]):
                    assert R.same_bits(got[j], exp[i, j]), (label, model, r, j, got[j], exp[i, j])
    assert sub > 0   # the subnormal sets do produce subnormal errors


def _refine_cases():
    for model in R.MODELS:
        for n, frac, seed in ((20, 0.3, 1), (500, 0.3, 2), (500, 0.6, 3), (5000, 0.3, 4), (5000, 0.6, 5), (64, 0.0, 6)):
            yield model, n, frac, seed


def _refine_inputs(model, n, frac, seed):
    pts4, inl, A = R.scene(model, n, 900 + seed, outlier_frac=frac)
    rng = np.random.default_rng(seed)
    start = A.ravel().copy()
    if model == N.MODEL_AFFINE:
        start += rng.normal(0, 1e-2, 6) * np.array([1, 1, 100, 1, 1, 100])
    else:
        a, b = start[0] + rng.normal(0, 1e-2), start[3] + rng.normal(0, 1e-2)
        start = np.array([a, -b, start[2] + rng.normal(0, 1), b, a, start[5] + rng.normal(0, 1)])
    return pts4, inl.astype(np.uint8), start


def measure_lstsq_deviation():
    """The largest relative (Frobenius) deviation of mcvHostAffineRefine from lstsq over this file's seeds."""
    worst = 0.0
    for model, n, frac, seed in _refine_cases():
        pts4, mask, start = _refine_inputs(model, n, frac, seed)
        got = R.host_refine(model, pts4, mask, start)
        worst = max(worst, R.rel(got, R.lstsq_model(model, pts4, mask)))
    return worst


@pytest.mark.parametrize("model,n,frac,seed", list(_refine_cases()))
def test_host_refine_vs_lstsq(native, model, n, frac, seed):
    pts4, mask, start = _refine_inputs(model, n, frac, seed)
    got = R.host_refine(model, pts4, mask, start)
    ref = R.lstsq_model(model, pts4, mask)
    dev = R.rel(got, ref)
    print(f"{MODEL_NAME[model]} n={n} outliers={frac}: relative deviation from lstsq {dev:.3e}")
    assert dev <= R.LSTSQ_BOUND
    assert R.cost(pts4, mask, got) <= R.cost(pts4, mask, start)
    if model == N.MODEL_SIMILARITY:
        assert got[0] == got[4] and got[1] == -got[3]


def test_abi_and_struct_sizes(native):
    L = native.lib()
    for name in ("cvEstimateAffine2D", "cvEstimateAffinePartial2D", "mcvTestAffineSweep", "mcvHostAffineRefine"):
        assert name in N.SIGNATURES and getattr(L, name) is not None
    assert L.mcvAbiVersion() == 3
    assert C.sizeof(N.RansacConfig) == 48 and C.sizeof(N.MatchConfig) == 16
    assert (N.MODEL_AFFINE, N.MODEL_SIMILARITY) == (4, 5)


def test_bad_arguments_rejected(native):
    L = native.lib()
    A = np.zeros(6)
    a = np.zeros((2, 2))
    assert L.cvEstimateAffine2D(None, None, 10, None, A.ctypes.data, None) == 0
    assert "null" in native.last_error()
    assert L.cvEstimateAffine2D(a.ctypes.data, a.ctypes.data, 2, None, A.ctypes.data, None) == 0
    assert "at least 3" in native.last_error()
    assert L.cvEstimateAffinePartial2D(a.ctypes.data, a.ctypes.data, 1, None, A.ctypes.data, None) == 0
    assert "at least 2" in native.last_error()
    assert L.mcvHostAffineRefine(N.MODEL_HOMOGRAPHY, a.ctypes.data, 1, None, A.ctypes.data) == -1
