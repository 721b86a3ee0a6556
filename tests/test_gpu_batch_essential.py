"""GPU tests of cvFindEssentialMatBatch / cvRecoverPoseBatch: B independent essential-matrix problems in one
call. The batched sweep is checked on given models against the oracle's count; the exports are checked bit for
bit (count, mask, the doubles of E or of R and t) against a loop over the single wrappers, against the oracle
directly, and for the property that makes them worth having: their launches and synchronisations do not grow
with B."""
import functools

import numpy as np
import pytest

import _oracle as O
from minicv_amd import native as N
from minicv_amd import opencv
from minicv_amd import synthetic as S

pytestmark = pytest.mark.gpu

FOCAL, PP = 800.0, (640.0, 360.0)
TILE = N.BATCH_E_TILE
CV = "cv"   # OpenCV's own sample stream instead of a Philox seed


# ---- problems and the two ways to solve them --------------------------------------------------------
def camera(p):
    """Problem p's own focal length and principal point."""
    return 600.0 + 37.0 * (p % 11), (640.0 - 13.0 * (p % 7), 360.0 + 9.0 * (p % 5))


@functools.lru_cache(maxsize=None)
def problem(n, seed, outl=0.4, focal=FOCAL, pp=PP):
    a, b, *_ = S.essential_problem(n, seed=seed, outlier_frac=outl, focal=focal, pp=pp)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def sizes(B):
    """N from 6 to ~600, odd and even, across the sweep's tile of 512."""
    base = [6, 599, 7, 50, 512, 128, 513, 33, 300, 64, 511, 9, 200]
    return [base[p % len(base)] + (p // len(base)) for p in range(B)]


def params(sampler, iters, fixed, thr=1.0, conf=0.999):
    return opencv.RansacParams(threshold=thr, confidence=conf, max_iters=iters, seed=0 if sampler == CV else sampler,
                               fixed_iters=fixed, cv_sampler=sampler == CV)


def single_find(a, b, focal, pp, p):
    """findEssentialMat on one problem -> (count, E, mask); a failure -> (0, zeros, zeros)."""
    try:
        return opencv.findEssentialMat(a, b, focal, pp, p)
    except N.NativeError:
        return 0, np.zeros((3, 3)), np.zeros(len(a), dtype=bool)


def single_pose(cfg, a, b):
    """recoverPose on one problem -> (good, R, t, ms); a failure -> zeros."""
    try:
        return opencv.recoverPose(cfg, a, b)
    except (N.NativeError, ValueError):
        return 0, np.zeros((3, 3)), np.zeros(3), np.zeros(len(a), dtype=np.uint8)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def assert_same_find(got, exp, what):
    assert got[0] == exp[0], (what, got[0], exp[0])
    np.testing.assert_array_equal(got[2], exp[2], err_msg=str(what))
    np.testing.assert_array_equal(bits(got[1]), bits(exp[1]), err_msg=str(what))


def assert_same_pose(got, exp, what):
    assert got[0] == exp[0], (what, got[0], exp[0])
    np.testing.assert_array_equal(got[3], exp[3], err_msg=str(what))
    np.testing.assert_array_equal(bits(got[1]), bits(exp[1]), err_msg=str(what))
    np.testing.assert_array_equal(bits(got[2]), bits(exp[2]), err_msg=str(what))


def stats():
    s = np.zeros(16, dtype=np.int64)
    assert N.lib().mcvTestBatchStats(s.ctypes.data) == 1
    return dict(launches=int(s[0]), syncs=int(s[1]), rounds=int(s[2]), single=int(s[4]), B=int(s[5]),
                problem_rounds=int(s[8]))


# ---- 1. the batched sweep on given models ------------------------------------------------------------
SWEEP_N = (1, 5, 511, TILE, TILE + 1, 2 * TILE + 1)
SWEEP_MODELS = (1, 255, 256, 257)


def batch_sweep(pts_list, model_list, thr2, kind):
    offsets = np.zeros(len(pts_list) + 1, dtype=np.int32)
    offsets[1:] = np.cumsum([p.shape[0] for p in pts_list])
    moff = np.zeros(len(model_list) + 1, dtype=np.int32)
    moff[1:] = np.cumsum([m.shape[0] for m in model_list])
    pts = np.ascontiguousarray(np.concatenate(pts_list))
    mdl = np.ascontiguousarray(np.concatenate(model_list))
    thr2 = np.ascontiguousarray(thr2, dtype=np.float32)
    counts = np.full(int(moff[-1]), -7, dtype=np.int32)
    ok = N.lib().mcvTestBatchSweepE(pts.ctypes.data, offsets.ctypes.data, len(pts_list), mdl.ctypes.data,
                                    moff.ctypes.data, thr2.ctypes.data, kind, counts.ctypes.data)
    assert ok == 1, N.last_error()
    return [counts[moff[i]:moff[i + 1]] for i in range(len(pts_list))]


def _sampson_np(F, x):
    """The op-by-op Sampson error as test_e_counts_at_exact_threshold_boundary restates it, cast to fp32."""
    ax = F[0] * x[:, 0] + F[1] * x[:, 1] + F[2] * 1.0
    ay = F[3] * x[:, 0] + F[4] * x[:, 1] + F[5] * 1.0
    az = F[6] * x[:, 0] + F[7] * x[:, 1] + F[8] * 1.0
    bx = F[0] * x[:, 2] + F[3] * x[:, 3] + F[6] * 1.0
    by = F[1] * x[:, 2] + F[4] * x[:, 3] + F[7] * 1.0
    c = x[:, 2] * ax + x[:, 3] * ay + 1.0 * az
    return (c * c / (ax * ax + ay * ay + bx * bx + by * by)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def sweep_case():
    """Per-problem N across the 512-point tile, model counts across the workgroup, a problem without models,
    NaN and inf models, a NaN coordinate, and a threshold per problem; problem 5's is the fp32 error of one of
    its points under its first model."""
    rng = np.random.default_rng(5)
    pts, mdl, thr2 = [], [], []
    for i, n in enumerate(SWEEP_N):
        a, b, _, _, _, E = S.essential_problem(max(n, 8), seed=40 + i, outlier_frac=0.3)
        p = O.pack_e(a, b, FOCAL, PP)[:n].copy()
        k = SWEEP_MODELS[i % 4]
        m = E.reshape(1, 9) + rng.normal(0, 2e-3, (k, 9)) * (np.arange(k) % 3 != 0)[:, None]
        if k > 4:
            m[1, 0] = np.nan
            m[2, 4] = np.inf
            m[3] = 0.0
        pts.append(p)
        mdl.append(np.ascontiguousarray(m))
        thr2.append(np.float32((1.0 + 0.5 * i) / FOCAL) ** 2)
    pts[3][17, 2] = np.nan                                    # one point with a NaN coordinate
    pts.insert(2, pts[0].copy())                              # a problem with points and no models
    mdl.insert(2, np.zeros((0, 9)))
    thr2.insert(2, thr2[0])
    n0, E90, _ = O.e_hypothesis(pts[6], 13, 0)                # the boundary: problem 6 = SWEEP_N[5]
    assert n0 >= 1
    mdl[6][0] = E90[0]
    err = _sampson_np(E90[0], pts[6])
    target = np.float32(np.quantile(err, 0.4, method="nearest"))
    thr2[6] = target
    return pts, mdl, thr2, err, target


@pytest.mark.parametrize("kind", [0, 1], ids=["fused", "op_by_op"])
def test_sweep_against_oracle_count(gpu, oracle, kind):
    pts, mdl, thr2, err, target = sweep_case()
    got = batch_sweep(pts, mdl, thr2, kind)
    assert len(got[2]) == 0
    for p, m, t2, g in zip(pts, mdl, thr2, got):
        exp = np.array([oracle.e_count(p, x, float(t2), kind) for x in m], dtype=np.int32)
        np.testing.assert_array_equal(g, exp)
    assert got[4][0] < len(pts[4])                            # the NaN point is no inlier of the true model
    assert (got[1][[1, 2, 3]] == 0).all()                     # NaN, inf and zero models count nothing
    if kind == 1:
        # thr2 equal to a point's fp32 error: that point is counted
        hit = int(np.flatnonzero(err == target)[0])
        assert got[6][0] == int((err <= target).sum())
        below = np.nextafter(target, np.float32(0))
        lower = batch_sweep(pts, mdl, thr2[:6] + [below], kind)[6][0]
        assert lower == int((err <= below).sum()) and got[6][0] - lower == int((err == target).sum()) >= 1
        assert err[hit] <= thr2[6]


# ---- 2. batch == loop of single calls, bit for bit ---------------------------------------------------
# (B, sampler, hypotheses per problem, fixed): every sampler with and without FIXED_ITERS at every B, the
# hypothesis counts across the 64-lane wave that appends models
FIND_CASES = [(1, 1, 1, True), (1, 2, 63, False), (1, CV, 64, True), (1, 1, 65, False), (1, 2, 300, True),
              (1, CV, 1000, False),
              (2, 1, 64, False), (2, 2, 1, True), (2, CV, 63, False), (2, 1, 1000, True), (2, 2, 65, False),
              (2, CV, 300, True),
              (65, 1, 300, False), (65, 2, 1000, True), (65, CV, 65, False), (65, 1, 63, True), (65, 2, 64, False),
              (65, CV, 1000, True)]


@pytest.mark.parametrize("B,sampler,iters,fixed", FIND_CASES)
def test_find_batch_equals_single_calls(gpu, B, sampler, iters, fixed):
    ns = sizes(B)
    cams = [camera(p) for p in range(B)]
    prob = [problem(n, 100 + p, 0.4, *cams[p]) for p, n in enumerate(ns)]
    par = params(sampler, iters, fixed, thr=1.5)
    got = opencv.findEssentialMatBatch([x[0] for x in prob], [x[1] for x in prob], [c[0] for c in cams],
                                       [c[1] for c in cams], par)
    assert len(got) == B
    for p in range(B):
        exp = single_find(prob[p][0], prob[p][1], cams[p][0], cams[p][1], par)
        assert_same_find(got[p], exp, (p, ns[p]))
    assert any(g[0] > 0 for g in got)
    s = stats()
    assert s["B"] == B and s["single"] == 0 and s["rounds"] == 1


@pytest.mark.parametrize("B", [1, 2, 65])
def test_pose_batch_equals_single_calls(gpu, B):
    """Per-problem focal, principal point, threshold and probability, all different."""
    ns = sizes(B)
    cams = [camera(p) for p in range(B)]
    prob = [problem(n, 300 + p, 0.3, *cams[p]) for p, n in enumerate(ns)]
    cfgs = [opencv.recoverPoseConfig(cams[p][0], cams[p][1], 0.9 + 0.0015 * p, 0.5 + 0.03 * p) for p in range(B)]
    got = opencv.recoverPoseBatch(cfgs, [x[0] for x in prob], [x[1] for x in prob])
    assert len(got) == B
    for p in range(B):
        assert_same_pose(got[p], single_pose(cfgs[p], *prob[p]), (p, ns[p]))
    assert any(g[0] > 0 for g in got)


def test_null_cfg_and_null_mask(gpu):
    """cfg NULL = cvFindEssentialMat's own defaults (OpenCV's stream); the mask is optional."""
    import ctypes as C
    ns = [40, 200]
    prob = [problem(n, 500 + p) for p, n in enumerate(ns)]
    a = np.ascontiguousarray(np.concatenate([x[0] for x in prob]))
    b = np.ascontiguousarray(np.concatenate([x[1] for x in prob]))
    offsets = np.array([0, 40, 240], dtype=np.int32)
    focal = np.array([FOCAL, FOCAL])
    pp = np.array([PP, PP], dtype=np.float64)
    E = np.zeros((2, 9))
    counts = np.zeros(2, dtype=np.int32)
    ret = N.lib().cvFindEssentialMatBatch(a.ctypes.data, b.ctypes.data, offsets.ctypes.data, 2, focal.ctypes.data,
                                          pp.ctypes.data, None, E.ctypes.data, None, counts.ctypes.data)
    assert ret == 2, N.last_error()
    for p in range(2):
        e1 = N.M33d()
        ms = np.zeros(ns[p], dtype=np.uint8)
        pa, pb = np.ascontiguousarray(prob[p][0]), np.ascontiguousarray(prob[p][1])
        c = N.lib().cvFindEssentialMat(pa.ctypes.data, pb.ctypes.data, ns[p], FOCAL, N.V2d(*PP), None, C.addressof(e1),
                                       ms.ctypes.data)
        assert c == counts[p] > 0
        np.testing.assert_array_equal(bits(E[p]), bits(np.array(e1.M[:])))


# ---- 3. a mixed batch --------------------------------------------------------------------------------
N5_SEEDS = (0, 1)


def n5_expected(seed):
    """What cvFindEssentialMat returns for the five points of `seed`, by the oracle, as test_find_essential_n5
    takes it: 5 with a single solution, else 0. det B(z) has its real roots in pairs, so generic points give
    0, 2, 4, ... solutions: none of 3000 synthetic and 3000 uniform five-point sets gave exactly one. The
    single-solution branch is therefore checked wherever the oracle reports it and is otherwise reached only
    through the routing, which hands such a problem to the single export unchanged."""
    a, b = problem(5, seed, 0.0)
    return O.find_essential(a, b, FOCAL, PP)[0]


def mixed_problems():
    same = (np.tile([[100.0, 200.0]], (50, 1)), np.tile([[110.0, 190.0]], (50, 1)))   # test_recover_edge_cases
    empty = (np.zeros((0, 2)), np.zeros((0, 2)))
    prob = [problem(150, 1, 0.0),                 # 0 all inliers
            problem(5, N5_SEEDS[0], 0.0),         # 1 N == 5 (several solutions, see n5_expected)
            problem(4, 1, 0.0),                   # 2 N < 5
            problem(5, N5_SEEDS[1], 0.0),         # 3 N == 5
            same,                                 # 4 all points identical: models, every point an inlier
            problem(400, 2, 0.9),                 # 5 90 % outliers
            empty,                                # 6 empty
            problem(120, 3, 0.3),                 # 7 focal 0
            problem(80, 4, 0.3)]                  # 8
    focals = [FOCAL] * 9
    focals[7] = 0.0
    return prob, focals


def first_failure():
    """The first failed problem of mixed_problems and a word of its message."""
    return (2, "at least 5") if n5_expected(N5_SEEDS[0]) == 5 else (1, "solutions")


def test_mixed_batch_find(gpu):
    prob, focals = mixed_problems()
    par = params(CV, 1000, False)
    got = opencv.findEssentialMatBatch([x[0] for x in prob], [x[1] for x in prob], focals, [PP] * 9, par)
    err = N.last_error()
    first, word = first_failure()
    assert f"cvFindEssentialMatBatch: problem {first}:" in err and word in err
    for p in range(9):
        assert_same_find(got[p], single_find(prob[p][0], prob[p][1], focals[p], PP, par), p)
    for p in (2, 6, 7):                           # failed: count 0, zero model, zero mask
        assert got[p][0] == 0 and not got[p][1].any() and not got[p][2].any()
    for p, seed in ((1, N5_SEEDS[0]), (3, N5_SEEDS[1])):
        if n5_expected(seed) == 5:
            assert got[p][0] == 5 and got[p][2].all() and got[p][1].any()
        else:
            assert got[p][0] == 0 and not got[p][1].any() and not got[p][2].any()
    assert got[0][0] >= 100 and got[4][0] == 50 and got[4][2].all()
    assert 5 <= got[5][0] < 120
    s = stats()
    assert s["single"] == 2 and s["B"] == 9
    got2 = opencv.findEssentialMatBatch([prob[7][0]], [prob[7][1]], [float("inf")], [PP], par)
    assert got2[0][0] == 0 and "problem 0" in N.last_error() and "focal" in N.last_error()


def test_mixed_batch_pose(gpu):
    prob, focals = mixed_problems()
    cfgs = [opencv.recoverPoseConfig(focals[p], PP, 0.999, 1.0) for p in range(9)]
    got = opencv.recoverPoseBatch(cfgs, [x[0] for x in prob], [x[1] for x in prob])
    err = N.last_error()
    first, word = first_failure()
    assert f"cvRecoverPoseBatch: problem {first}:" in err and word in err
    for p in range(9):
        exp = single_pose(cfgs[p], *prob[p])
        if p in (1, 3) and n5_expected(N5_SEEDS[p // 2]) != 5:
            # the documented difference: the single call leaves ms all 1, the batch zeroes the slice
            assert got[p][0] == 0 and not got[p][1].any() and not got[p][2].any() and not got[p][3].any()
            continue
        assert_same_pose(got[p], exp, p)
    for p in (2, 6, 7):
        assert got[p][0] == 0 and not got[p][1].any() and not got[p][2].any() and not got[p][3].any()
    assert got[0][0] >= 90 and got[4][3].all()


# ---- 4. against the oracle directly ------------------------------------------------------------------
def test_batch_against_oracle(gpu, oracle):
    ns = [6, 60, 333, 513, 600]
    cams = [camera(p + 3) for p in range(5)]
    prob = [problem(n, 700 + p, 0.35, *cams[p]) for p, n in enumerate(ns)]
    thr = [0.8, 1.0, 1.3, 0.7, 2.0]
    par = params(CV, 1000, False, thr=1.25)
    got = opencv.findEssentialMatBatch([x[0] for x in prob], [x[1] for x in prob], [c[0] for c in cams],
                                       [c[1] for c in cams], par)
    for p in range(5):
        rc, Er, rmask, _ = oracle.find_essential(*prob[p], cams[p][0], cams[p][1], thr=1.25, conf=0.999,
                                                 max_iters=1000, flags=N.FLAG_CV_SAMPLER)
        assert got[p][0] == rc
        np.testing.assert_array_equal(got[p][1], Er)
        np.testing.assert_array_equal(got[p][2], rmask != 0)
    cfgs = [opencv.recoverPoseConfig(cams[p][0], cams[p][1], 0.999, thr[p]) for p in range(5)]
    pose = opencv.recoverPoseBatch(cfgs, [x[0] for x in prob], [x[1] for x in prob])
    for p in range(5):
        rc, Er, rmask, _ = oracle.find_essential(*prob[p], cams[p][0], cams[p][1], thr=thr[p], conf=0.999,
                                                 max_iters=1000, flags=N.FLAG_CV_SAMPLER)
        np.testing.assert_array_equal(pose[p][3], rmask)
        rres, Rr, tr, _ = oracle.recover_pose(*prob[p], Er, rmask, cams[p][0], cams[p][1])
        assert pose[p][0] == rres
        np.testing.assert_array_equal(pose[p][1], Rr)
        np.testing.assert_array_equal(pose[p][2], tr)


# ---- 5. launch and synchronisation counts ------------------------------------------------------------
def test_launches_and_syncs_do_not_grow_with_B(gpu):
    seen = {}
    for B in (4, 64):
        prob = [problem(100 + p, 900 + p) for p in range(B)]
        a, b = [x[0] for x in prob], [x[1] for x in prob]
        opencv.findEssentialMatBatch(a, b, [FOCAL] * B, [PP] * B, params(1, 300, False))
        f = stats()
        opencv.recoverPoseBatch(opencv.recoverPoseConfig(FOCAL, PP, 0.999, 1.0), a, b)
        r = stats()
        assert f["B"] == r["B"] == B
        seen[B] = (f["launches"], f["syncs"], r["launches"], r["syncs"])
    assert seen[4] == seen[64]
    # one round: pack, the generate's three kernels, the sweep, the winners' fetch, the mask (+ the cheirality)
    assert seen[4] == (1 + 4 + 2, 2, 1 + 4 + 2 + 1, 3)


# ---- 6. several rounds -------------------------------------------------------------------------------
def test_several_rounds_under_a_lowered_cap(gpu):
    """8 problems x 1000 hypotheses under a cap of 8 x 64: up to 16 rounds. The all-inlier problems stop after
    the first and drop out, the 90 % outlier problem needs the whole budget; nothing changes in the results."""
    prob = [problem(100 + 10 * p, 950 + p, 0.0 if p % 2 == 0 else (0.9 if p == 3 else 0.4)) for p in range(8)]
    a, b = [x[0] for x in prob], [x[1] for x in prob]
    cfgs = [opencv.recoverPoseConfig(FOCAL, PP, 0.999, 1.0 + 0.1 * p) for p in range(8)]
    par = params(2, 1000, False)
    find0 = opencv.findEssentialMatBatch(a, b, [FOCAL] * 8, [PP] * 8, par)
    assert stats()["rounds"] == 1
    pose0 = opencv.recoverPoseBatch(cfgs, a, b)
    prev = N.lib().mcvTestBatchCap(8 * 64)
    try:
        find1 = opencv.findEssentialMatBatch(a, b, [FOCAL] * 8, [PP] * 8, par)
        s = stats()
        pose1 = opencv.recoverPoseBatch(cfgs, a, b)
        sp = stats()
    finally:
        N.lib().mcvTestBatchCap(prev)
    assert N.lib().mcvTestBatchCap(prev) == prev == N.BATCH_SLOT_CAP   # restored
    for st in (s, sp):
        assert 2 <= st["rounds"] <= 16
        assert 8 < st["problem_rounds"] < 8 * st["rounds"]               # somebody dropped out early
    for p in range(8):
        assert_same_find(find1[p], find0[p], p)
        assert_same_pose(pose1[p], pose0[p], p)
        assert_same_find(find1[p], single_find(prob[p][0], prob[p][1], FOCAL, PP, par), p)
    opencv.findEssentialMatBatch(a, b, [FOCAL] * 8, [PP] * 8, par)
    assert stats()["rounds"] == 1                                         # the default cap is back


def test_large_adaptive_batch_starts_with_a_small_round(gpu):
    """From 2^16 hypotheses in a full round on, an adaptive batch runs 256 hypotheses per problem first and the
    rest of the budget only for the problems still searching: one round more at most, at B = 80 as at B = 160,
    and the results are those of the single calls. A fixed budget stays one round."""
    B = 160
    prob = [problem(30 + (p % 50), 1200 + p, 0.9 if p % 40 == 7 else 0.3) for p in range(B)]
    a, b = [x[0] for x in prob], [x[1] for x in prob]
    par = params(1, 1000, False)
    got = opencv.findEssentialMatBatch(a, b, [FOCAL] * B, [PP] * B, par)
    s = stats()
    assert s["rounds"] == 2 and B < s["problem_rounds"] < 2 * B and s["launches"] in (11, 12)   # the fetch is per round
    for p in range(B):
        assert_same_find(got[p], single_find(prob[p][0], prob[p][1], FOCAL, PP, par), p)
    half = opencv.findEssentialMatBatch(a[:80], b[:80], [FOCAL] * 80, [PP] * 80, par)
    assert stats()["rounds"] == 2
    for p in range(80):
        assert_same_find(half[p], got[p], p)
    opencv.findEssentialMatBatch(a, b, [FOCAL] * B, [PP] * B, params(1, 1000, True))
    assert stats()["rounds"] == 1


# ---- 7. the wrappers ---------------------------------------------------------------------------------
def test_wrappers_return_the_single_wrappers_results(gpu):
    prob = [problem(90, 21), problem(45, 22, 0.2)]
    cfg = opencv.recoverPoseConfig(FOCAL, PP, 0.999, 1.0)
    pose = opencv.recoverPoseBatch(cfg, [x[0] for x in prob], [x[1] for x in prob])      # one config for all
    find = opencv.findEssentialMatBatch([x[0] for x in prob], [x[1] for x in prob], [FOCAL, FOCAL], [PP, PP])
    for p in range(2):
        res, R, t, ms = opencv.recoverPose(cfg, *prob[p])
        assert pose[p][0] == res and pose[p][3].dtype == np.uint8
        np.testing.assert_array_equal(pose[p][1], R)
        np.testing.assert_array_equal(pose[p][2], t)
        np.testing.assert_array_equal(pose[p][3], ms)
        cnt, E, mask = opencv.findEssentialMat(*prob[p], FOCAL, PP, opencv.RansacParams(
            threshold=1.0, confidence=0.999, max_iters=1000, cv_sampler=True))           # the native NULL-cfg defaults
        assert find[p][0] == cnt and find[p][2].dtype == bool
        np.testing.assert_array_equal(find[p][1], E)
        np.testing.assert_array_equal(find[p][2], mask)
    import minicv_amd
    assert minicv_amd.findEssentialMatBatch is opencv.findEssentialMatBatch
    assert minicv_amd.recoverPoseBatch is opencv.recoverPoseBatch
