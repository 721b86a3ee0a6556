"""GPU tests of cvFindModelBatch: B independent RANSAC problems of one family (homography, 8-point
fundamental, affine, similarity) in one call. The batched sweep is checked on given models against the
references and the single calls' sweeps; the export is checked bit for bit (count, mask, nine doubles)
against a loop over the single wrappers, against the project's references directly, and for the property
that makes it worth having: its launches and synchronisations do not grow with B."""
import functools

import numpy as np
import pytest

import _affine_ref as R
import _oracle as O
from minicv_amd import native as N
from minicv_amd import opencv
from minicv_amd import synthetic as S

pytestmark = pytest.mark.gpu

H, F, A, SIM = N.MODEL_HOMOGRAPHY, N.MODEL_FUNDAMENTAL, N.MODEL_AFFINE, N.MODEL_SIMILARITY
MODELS = (H, F, A, SIM)
NAME = {H: "homography", F: "fundamental", A: "affine", SIM: "similarity"}
SAMPLE = {H: 4, F: 8, A: 3, SIM: 2}
THR = {H: 5e-3, F: 5e-3, A: 2.0, SIM: 2.0}
REL_TOL = 1e-6   # refined H / F against the oracle: the bound of test_gpu_homography.py
TILE = N.BATCH_TILE


def relf(X, Y):
    return np.linalg.norm(np.asarray(X) - np.asarray(Y)) / np.linalg.norm(Y)


# ---- problems and the two ways to solve them --------------------------------------------------------
@functools.lru_cache(maxsize=None)
def problem(model, n, seed, outl=0.4):
    """(src, dst) float64 of one problem."""
    if model == H:
        src, dst, _ = S.homography_problem(n, seed, outlier_frac=outl)
    elif model == F:
        src, dst, _, _ = S.fundamental_problem(n, seed, outlier_frac=outl)
    else:
        p4, _, _ = R.scene(model, n, seed, outlier_frac=outl)
        src, dst = p4[:, :2].astype(np.float64), p4[:, 2:].astype(np.float64)
    src.setflags(write=False)
    dst.setflags(write=False)
    return src, dst


def single(model, src, dst, params):
    """The existing wrapper on one problem -> (count, M 3x3, mask); a failure -> (0, zeros, zeros)."""
    try:
        if model == H:
            return opencv.findHomography(src, dst, params)
        if model == F:
            return opencv.findFundamentalMat(src, dst, params)
        fn = opencv.estimateAffine2D if model == A else opencv.estimateAffinePartial2D
        A6, mask, cnt = fn(src, dst, params)
        return cnt, np.vstack([A6, [0.0, 0.0, 1.0]]), mask
    except N.NativeError:
        return 0, np.zeros((3, 3)), np.zeros(len(src), dtype=bool)


def assert_same(got, exp, what):
    assert got[0] == exp[0], (what, got[0], exp[0])
    np.testing.assert_array_equal(got[2], exp[2], err_msg=str(what))
    np.testing.assert_array_equal(got[1].view(np.uint64), exp[1].view(np.uint64), err_msg=str(what))   # the bits


def stats():
    s = np.zeros(16, dtype=np.int64)
    assert N.lib().mcvTestBatchStats(s.ctypes.data) == 1
    return dict(launches=int(s[0]), syncs=int(s[1]), rounds=int(s[2]), lm=int(s[3]), single=int(s[4]), B=int(s[5]))


# ---- the batched sweep on given models --------------------------------------------------------------
SWEEP_N = (1, 2, 63, 64, 65, 127, 128, 129, 257, TILE, TILE + 1)
SWEEP_MODELS = (1, 255, 256, 257)


def _sweep_points(n, rng):
    """The integer tie set of test_gpu_affine.py (every operation of the error is exact): dst = src + (3, 4)
    for every third correspondence, the first included (error exactly 25 under the identity, 0 under the
    shift), + (3, 5) for the next, + 0 for the third."""
    src = rng.integers(-50, 50, (n, 2)).astype(np.float32)
    off = np.array([[3, 4], [3, 5], [0, 0]], dtype=np.float32)[np.arange(n) % 3]
    return np.ascontiguousarray(np.concatenate([src, src + off], 1))


def _sweep_models(count, rng):
    """The model set of test_gpu_affine.py: identity, a NaN model, an inf model, two shifts, then random."""
    base = [R.IDENTITY,                                                     # errors 25 (== thr2), 34, 0
            np.array([np.nan, 0, 0, 0, 1, 0], dtype=np.float32),
            np.array([np.inf, 0, 0, 0, 1, 0], dtype=np.float32),
            np.array([1, 0, 3, 0, 1, 4], dtype=np.float32),                  # errors 0, 1, 25
            np.array([1, 0, 0, 0, 1, -1], dtype=np.float32)]                 # errors 34, 45, 1
    ms = [base[i % len(base)] if i < 2 * len(base) else rng.normal(0, 1, 6).astype(np.float32) for i in range(count)]
    return np.ascontiguousarray(np.stack(ms))


def batch_sweep(model, pts_list, model_list, thr2, kind):
    offsets = np.zeros(len(pts_list) + 1, dtype=np.int32)
    offsets[1:] = np.cumsum([p.shape[0] for p in pts_list])
    moff = np.zeros(len(model_list) + 1, dtype=np.int32)
    moff[1:] = np.cumsum([m.shape[0] for m in model_list])
    pts = np.ascontiguousarray(np.concatenate(pts_list))
    mdl = np.ascontiguousarray(np.concatenate(model_list))
    counts = np.full(int(moff[-1]), -7, dtype=np.int32)
    ok = N.lib().mcvTestBatchSweep(model, pts.ctypes.data, offsets.ctypes.data, len(pts_list), mdl.ctypes.data,
                                   moff.ctypes.data, float(thr2), kind, counts.ctypes.data)
    assert ok == 1, N.last_error()
    return [counts[moff[i]:moff[i + 1]] for i in range(len(pts_list))]


def single_sweep(hook, pts4, models, thr2, mode):
    counts = np.full(models.shape[0], -7, dtype=np.int32)
    assert hook(pts4.ctypes.data, pts4.shape[0], models.ctypes.data, models.shape[0], float(thr2), mode,
                counts.ctypes.data) == 1, N.last_error()
    return counts


def to_h8(a6):
    """An affine model as a homography model (h6 = h7 = 0: ww = 1, the same error values)."""
    return np.ascontiguousarray(np.concatenate([a6, np.zeros((a6.shape[0], 2), np.float32)], 1))


@pytest.mark.parametrize("model", [A, SIM, H], ids=NAME.get)
def test_sweep_integer_ties_nan_inf(gpu, model):
    """Integer-valued points (errors exactly 0, 1, 25, 34, 45; thr2 = 25 is hit exactly), NaN and inf
    models, every per-problem N and model count at once."""
    rng = np.random.default_rng(11)
    pts = [_sweep_points(n, rng) for n in SWEEP_N]
    a6 = [_sweep_models(SWEEP_MODELS[i % 4], rng) for i in range(len(SWEEP_N))]
    mdl = [to_h8(m) for m in a6] if model == H else a6
    got = batch_sweep(model, pts, mdl, 25.0, 0)
    for p, m6, m, g in zip(pts, a6, mdl, got):
        exp = np.array([R.count(p, x, 25.0) for x in m6], dtype=np.int32)
        np.testing.assert_array_equal(g, exp)
        if model == H:
            np.testing.assert_array_equal(g, [O.h_count(p, x, 25.0) for x in m])
            for mode in (0, 3):   # the scalar sweep and the certified default sweep of the single call
                np.testing.assert_array_equal(g, single_sweep(N.lib().mcvTestHomographySweep, p, m, 25.0, mode))
        else:
            np.testing.assert_array_equal(g, single_sweep(N.lib().mcvTestAffineSweep, p, m, 25.0, 0))
    e = R.errors(pts[2], R.IDENTITY)
    assert (e == 25).any() and got[2][0] == int((e <= 25).sum()) > int((e < 25).sum())   # the ties count


@pytest.mark.parametrize("model", [A, H], ids=NAME.get)
def test_sweep_real_scenes_and_subnormals(gpu, model):
    rng = np.random.default_rng(12)
    pts, mdl, thr2s = [], [], []
    for i, n in enumerate(SWEEP_N):
        if model == H:
            src, dst = problem(H, max(n, 4), 100 + n)
            p = O.pack4(src, dst)[:n]
            ms = rng.normal(0, 1, (SWEEP_MODELS[i % 4], 8)).astype(np.float32)
            ms[:, 6:] *= 0.1
            ms[0] = (S.H_TRUE / S.H_TRUE[2, 2]).ravel()[:8].astype(np.float32)
        else:
            p, _, At = R.scene(A, n, 300 + n)
            ms = rng.normal(0, 1, (SWEEP_MODELS[i % 4], 6)).astype(np.float32)
            ms[0] = At.ravel().astype(np.float32)
        pts.append(np.ascontiguousarray(p))
        mdl.append(np.ascontiguousarray(ms))
    thr2 = float(np.float32(THR[model] ** 2))
    got = batch_sweep(model, pts, mdl, thr2, 0)
    for p, m, g in zip(pts, mdl, got):
        if model == H:
            np.testing.assert_array_equal(g, [O.h_count(p, x, thr2) for x in m])
            np.testing.assert_array_equal(g, single_sweep(N.lib().mcvTestHomographySweep, p, m, thr2, 3))
        else:
            np.testing.assert_array_equal(g, [R.count(p, x, thr2) for x in m])
            np.testing.assert_array_equal(g, single_sweep(N.lib().mcvTestAffineSweep, p, m, thr2, 0))
    assert max(int(g.max()) for g in got) > 0
    # subnormal products: a subnormal threshold with inliers on both sides of it
    for n in (65, 1000):
        p = R.subnormal_set(n, rng)
        e = R.errors(p, R.IDENTITY)
        sub = (e > 0) & (e < np.float32(2.0**-126))
        t2 = float(np.sort(e[sub])[sub.sum() // 2])
        exp = R.count(p, R.IDENTITY, t2)
        assert 0 < exp < n
        ident = np.ascontiguousarray(np.stack([R.IDENTITY] * 257))
        g = batch_sweep(model, [p, p[:33]], [to_h8(ident) if model == H else ident] * 2, t2, 0)
        np.testing.assert_array_equal(g[0], np.full(257, exp, dtype=np.int32))
        np.testing.assert_array_equal(g[1], np.full(257, R.count(p[:33], R.IDENTITY, t2), dtype=np.int32))


@pytest.mark.parametrize("error_kind", [N.FERR_SAMPSON, N.FERR_EPIPOLAR], ids=["sampson", "epipolar"])
def test_sweep_fundamental(gpu, error_kind):
    rng = np.random.default_rng(13)
    kind = O.f_kind(error_kind, True)
    thr2 = float(np.float32(THR[F] ** 2))
    pts, mdl = [], []
    for i, n in enumerate(SWEEP_N):
        a, b, _, Ft = S.fundamental_problem(max(n, 8), 200 + n, outlier_frac=0.4)
        ms = rng.normal(0, 1, (SWEEP_MODELS[i % 4], 9))
        ms[0] = Ft.ravel()
        if ms.shape[0] > 3:
            ms[1, 4] = np.nan
            ms[2, 0] = np.inf
            ms[3] = 0.0
        pts.append(np.ascontiguousarray(O.pack4(a, b)[:n]))
        mdl.append(np.ascontiguousarray(ms))
    got = batch_sweep(F, pts, mdl, thr2, kind)
    for p, m, g in zip(pts, mdl, got):
        np.testing.assert_array_equal(g, [O.f_count(p, x, thr2, kind) for x in m])
    assert max(int(g[0]) for g in got) > 100   # the true F counts its inliers


# ---- batch == single call, bit for bit --------------------------------------------------------------
SIZES = (None, 63, 64, 65, 129, 257, 513, 1000)   # None = m + 1
SAMPLERS = {"philox1": dict(seed=1), "philox2": dict(seed=0x9E3779B97F4A7C15), "cv": dict(cv_sampler=True)}
FLAGS = {"plain": {}, "fixed": dict(fixed_iters=True), "norefine": dict(refine=False)}
SHAPES = ((1, 1), (1, 257), (2, 255), (2, 2000), (65, 257), (65, 2000))   # (B, maxIters)


def batch_problems(model, B, salt):
    rng = np.random.default_rng(1000 * model + salt)
    out = []
    for p in range(B):
        n = SIZES[(p + salt) % len(SIZES)] or SAMPLE[model] + 1
        out.append(problem(model, n, int(rng.integers(1, 50)), float(rng.choice([0.0, 0.3, 0.6]))))
    return out


@pytest.mark.parametrize("sampler", SAMPLERS, ids=list(SAMPLERS))
@pytest.mark.parametrize("model,error_kind", [(H, 0), (F, N.FERR_SAMPSON), (F, N.FERR_EPIPOLAR), (A, 0), (SIM, 0)],
                         ids=["homography", "fundamental-sampson", "fundamental-epipolar", "affine", "similarity"])
def test_batch_equals_single_calls(gpu, model, error_kind, sampler):
    conf = 0.995 if model == H else 0.99
    solved = refined = 0
    for fi, (fname, fl) in enumerate(FLAGS.items()):
        for si, (B, iters) in enumerate(SHAPES):
            probs = batch_problems(model, B, fi + 3 * si)
            p = opencv.RansacParams(threshold=THR[model], confidence=conf, max_iters=iters, error_kind=error_kind,
                                    **SAMPLERS[sampler], **fl)
            got = opencv.findModelBatch(model, [s for s, _ in probs], [d for _, d in probs], p)
            st = stats()
            assert st["single"] == 0 and st["B"] == B and st["rounds"] == 1
            for k, (src, dst) in enumerate(probs):
                exp = single(model, src, dst, p)
                assert_same(got[k], exp, (fname, B, iters, k, len(src)))
                solved += exp[0] > 0
            refined += st["lm"]
    assert solved > 50
    assert (refined > 0) == (model != F)   # the lockstep refine ran (F has none)


CLAMP_N = 256 * 1024 + 1   # the first N past reduce.h's block-count clamp (1024 blocks of 256 threads)


@pytest.mark.parametrize("model", [H, A, SIM], ids=NAME.get)   # F has no refine
def test_batch_equals_single_calls_past_the_reduction_clamp(gpu, model):
    """The refine's reductions where a block strides over more than one trip of points (the clamp is code the
    single and the batched pass share), beside a problem far below it in the same launches."""
    probs = [problem(model, CLAMP_N, 41, 0.3), problem(model, 257, 42, 0.3)]
    p = opencv.RansacParams(threshold=THR[model], confidence=0.995 if model == H else 0.99, max_iters=64,
                            fixed_iters=True, **SAMPLERS["philox1"])
    got = opencv.findModelBatch(model, [s for s, _ in probs], [d for _, d in probs], p)
    st = stats()
    assert st["single"] == 0 and st["B"] == 2 and st["lm"] > 0
    for k, (src, dst) in enumerate(probs):
        exp = single(model, src, dst, p)
        assert exp[0] > SAMPLE[model]   # a winner with inliers beyond its sample: both calls refined it
        assert_same(got[k], exp, (k, len(src)))


@pytest.mark.parametrize("model", MODELS, ids=NAME.get)
def test_null_config_is_the_single_exports_default(gpu, model):
    probs = batch_problems(model, 5, 7)
    got = opencv.findModelBatch(model, [s for s, _ in probs], [d for _, d in probs], None)
    fn = {H: N.lib().cvFindHomography, F: N.lib().cvFindFundamentalMat, A: N.lib().cvEstimateAffine2D,
          SIM: N.lib().cvEstimateAffinePartial2D}[model]
    for k, (src, dst) in enumerate(probs):
        a, b = np.ascontiguousarray(src), np.ascontiguousarray(dst)
        M = np.zeros(9)
        M[8] = 1.0 if model in (A, SIM) else 0.0
        mask = np.zeros(len(a), dtype=np.uint8)
        cnt = fn(a.ctypes.data, b.ctypes.data, len(a), None, M.ctypes.data, mask.ctypes.data)
        exp = (cnt, M.reshape(3, 3), mask != 0) if cnt > 0 else (0, np.zeros((3, 3)), np.zeros(len(a), dtype=bool))
        assert_same(got[k], exp, k)


# ---- a batch of everything that can happen to a problem ------------------------------------------------
@pytest.mark.parametrize("model", MODELS, ids=NAME.get)
def test_mixed_batch(gpu, model):
    m = SAMPLE[model]
    full = problem(model, 300, 5, 0.0)
    same = (np.tile(full[0][:1], (50, 1)), np.tile(full[1][:1], (50, 1)))   # every point identical
    probs = [(full[0][:m - 1], full[1][:m - 1]),          # 0: N < m
             (full[0][:m], full[1][:m]),                  # 1: N == m, the direct solve
             same,                                        # 2: degenerate: the single call finds no model
             full,                                        # 3: all inliers: stops early
             problem(model, 1000, 6, 0.9),                # 4: 90 % outliers
             (full[0][:0], full[1][:0]),                  # 5: empty slice
             problem(model, 257, 8, 0.3)]                 # 6: an ordinary problem after the failures
    p = opencv.RansacParams(threshold=THR[model], confidence=0.99, max_iters=2000, seed=3)
    srcs, dsts = [s for s, _ in probs], [d for _, d in probs]
    offsets = np.zeros(len(probs) + 1, dtype=np.int32)
    offsets[1:] = np.cumsum([len(s) for s in srcs])
    a, b = np.ascontiguousarray(np.concatenate(srcs)), np.ascontiguousarray(np.concatenate(dsts))
    models = np.full((len(probs), 9), 7.0)
    counts = np.full(len(probs), -7, dtype=np.int32)
    mask = np.full(int(offsets[-1]), 9, dtype=np.uint8)
    cfg = p.to_c()
    ret = N.lib().cvFindModelBatch(model, a.ctypes.data, b.ctypes.data, offsets.ctypes.data, len(probs),
                                   N.C.addressof(cfg), models.ctypes.data, mask.ctypes.data, counts.ctypes.data)
    err = N.last_error()
    exp = [single(model, s, d, p) for s, d in probs]
    for k, e in enumerate(exp):
        got = (int(counts[k]), models[k].reshape(3, 3), mask[offsets[k]:offsets[k + 1]] != 0)
        assert_same(got, e, k)
        assert set(np.unique(mask[offsets[k]:offsets[k + 1]])) <= {0, 1}
    succ = [e[0] > 0 for e in exp]
    assert succ[:4] == [False, True, False, True] and succ[5:] == [False, True]   # (the 90 % case: as the single call)
    assert exp[1][0] == m and exp[1][2].all() and exp[3][0] > 150
    assert ret == sum(succ)
    assert "problem 0:" in err and f"at least {m}" in err
    assert stats()["single"] == 1
    # without the first failure the message names the next one
    got = opencv.findModelBatch(model, srcs[1:], dsts[1:], p)
    assert "problem 1:" in N.last_error() and [g[0] > 0 for g in got] == succ[1:]
    # and a batch without failures leaves no message
    opencv.findModelBatch(model, [srcs[3], srcs[6]], [dsts[3], dsts[6]], p)
    assert N.last_error() == ""


# ---- against the references themselves -----------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, N.FLAG_CV_SAMPLER, N.FLAG_NO_REFINE], ids=["philox", "cv", "norefine"])
def test_homography_batch_vs_oracle(gpu, oracle, flags):
    probs = [problem(H, n, s, o) for n, s, o in ((200, 3, 0.5), (65, 4, 0.3), (1000, 5, 0.6), (513, 6, 0.0))]
    p = opencv.RansacParams(threshold=5e-3, confidence=0.995, max_iters=2000, seed=21,
                            cv_sampler=bool(flags & N.FLAG_CV_SAMPLER), refine=not flags & N.FLAG_NO_REFINE)
    got = opencv.findModelBatch(H, [s for s, _ in probs], [d for _, d in probs], p)
    for (src, dst), (cnt, M, mask) in zip(probs, got):
        cnt_o, H_o, mask_o, _ = oracle.find_homography(src, dst, thr=5e-3, conf=0.995, max_iters=2000, seed=21,
                                                       flags=flags)
        assert cnt == cnt_o > 0
        np.testing.assert_array_equal(mask, mask_o.astype(bool))
        assert relf(M, H_o) < REL_TOL
        if flags & N.FLAG_NO_REFINE:
            np.testing.assert_array_equal(M, H_o)   # the same fp64 minimal solve


@pytest.mark.parametrize("error_kind", [N.FERR_SAMPSON, N.FERR_EPIPOLAR], ids=["sampson", "epipolar"])
@pytest.mark.parametrize("flags", [0, N.FLAG_CV_SAMPLER], ids=["philox", "cv"])
def test_fundamental_batch_vs_oracle(gpu, oracle, flags, error_kind):
    probs = [problem(F, n, s, o) for n, s, o in ((200, 3, 0.5), (65, 4, 0.3), (1000, 5, 0.5), (129, 6, 0.0))]
    p = opencv.RansacParams(threshold=5e-3, confidence=0.99, max_iters=1000, seed=22, error_kind=error_kind,
                            cv_sampler=bool(flags & N.FLAG_CV_SAMPLER))
    got = opencv.findModelBatch(F, [s for s, _ in probs], [d for _, d in probs], p)
    for (src, dst), (cnt, M, mask) in zip(probs, got):
        cnt_o, F_o, mask_o, _ = oracle.find_fundamental(src, dst, thr=5e-3, conf=0.99, max_iters=1000, seed=22,
                                                        flags=flags, error_kind=error_kind)
        assert cnt == cnt_o > 0
        np.testing.assert_array_equal(mask, mask_o.astype(bool))
        assert relf(M, F_o) < REL_TOL
        np.testing.assert_array_equal(M, F_o)   # F is the winning sample's solve: the same bits


@pytest.mark.parametrize("cv", [False, True], ids=["philox", "cv"])
@pytest.mark.parametrize("model", R.MODELS, ids=NAME.get)
def test_affine_batch_vs_restatement(gpu, model, cv):
    """As test_gpu_affine.py's end-to-end test: unrefined bits equal the restatement's, the refined model
    is within 1e-6 of the host refine with sequential sums and within the lstsq bound."""
    m = SAMPLE[model]
    scenes = [R.scene(model, n, 1000 * n + 3, outlier_frac=f)[0] for n, f in ((20, 0.3), (500, 0.6), (65, 0.3), (1000, 0.3))]
    srcs = [s[:, :2].astype(np.float64) for s in scenes]
    dsts = [s[:, 2:].astype(np.float64) for s in scenes]
    p = opencv.RansacParams(threshold=2.0, confidence=0.99, max_iters=2000, seed=77, cv_sampler=cv, refine=False)
    raw = opencv.findModelBatch(model, srcs, dsts, p)
    p.refine = True
    ref = opencv.findModelBatch(model, srcs, dsts, p)
    for pts4, (cnt, M, mask), (cnt2, M2, mask2) in zip(scenes, raw, ref):
        r = R.ransac_ref(model, pts4, 2.0, 0.99, 2000, seed=77, cv=cv)
        assert r is not None and cnt == cnt2 == r["count"] > m
        np.testing.assert_array_equal(mask, r["mask"].astype(bool))
        np.testing.assert_array_equal(mask2, mask)
        np.testing.assert_array_equal(M[:2].ravel().view(np.uint64), r["A"].view(np.uint64))
        np.testing.assert_array_equal(M[2], [0.0, 0.0, 1.0])
        host = R.host_refine(model, pts4, r["mask"], r["A"])
        assert R.rel(M2[:2], host) < REL_TOL
        assert R.rel(M2[:2], R.lstsq_model(model, pts4, r["mask"])) <= R.LSTSQ_BOUND
        assert R.cost(pts4, r["mask"], M2[:2].ravel()) <= R.cost(pts4, r["mask"], r["A"])


# ---- batching is real ----------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS, ids=NAME.get)
def test_launches_and_synchronisations_do_not_grow_with_b(gpu, model):
    src, dst = problem(model, 500, 9, 0.4)
    p = opencv.RansacParams(threshold=THR[model], confidence=0.99, max_iters=2000, seed=5)
    out = {}
    for B in (4, 64):
        got = opencv.findModelBatch(model, [src] * B, [dst] * B, p)
        out[B] = (got, stats())
    (g4, s4), (g64, s64) = out[4], out[64]
    assert s4["launches"] == s64["launches"] > 0 and s4["syncs"] == s64["syncs"] > 0
    assert s4["single"] == s64["single"] == 0 and s4["rounds"] == s64["rounds"] == 1
    assert s4["lm"] == s64["lm"] and (s4["lm"] > 0) == (model != F)
    # generate + sweep, re-solve + mask, and per refine round one reduction pair (H: + the refit's 8)
    assert s64["launches"] == 4 + 2 * s64["lm"] + (8 if model == H else 0)
    assert s64["syncs"] == 2 + s64["lm"] + (1 if model == H else 0)
    exp = single(model, src, dst, p)
    assert exp[0] > 100
    for g in g4 + g64:
        assert_same(g, exp, "replica")


@pytest.mark.parametrize("fixed", [False, True], ids=["adaptive", "fixed"])
@pytest.mark.parametrize("model", MODELS, ids=NAME.get)
def test_workspace_cap_forces_rounds(gpu, model, fixed):
    probs = batch_problems(model, 9, 2) + [problem(model, 400, 12, 0.85)]
    srcs, dsts = [s for s, _ in probs], [d for _, d in probs]
    p = opencv.RansacParams(threshold=THR[model], confidence=0.99, max_iters=700, seed=8, fixed_iters=fixed)
    whole = opencv.findModelBatch(model, srcs, dsts, p)
    assert stats()["rounds"] == 1
    prev = N.lib().mcvTestBatchCap(len(probs) * 100)   # 100 hypotheses per problem per round
    try:
        capped = opencv.findModelBatch(model, srcs, dsts, p)
        st = stats()
    finally:
        N.lib().mcvTestBatchCap(prev)
    assert 2 <= st["rounds"] <= 7 and (st["rounds"] == 7 or not fixed)
    for k, (g, w) in enumerate(zip(capped, whole)):
        assert_same(g, w, k)
    assert sum(w[0] > 0 for w in whole) >= 5
