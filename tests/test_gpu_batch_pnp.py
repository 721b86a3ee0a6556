"""GPU tests of cvSolvePnPRansacBatch: B independent solvePnPRansac problems in one call. The batched sweep is
checked on given poses against the oracle's count; the export is checked bit for bit (success, inlier set, the
doubles of rvec and tvec) against a loop over the single wrapper, against the oracle directly, and for the
property that makes it worth having: its launches, synchronisations and copies do not grow with B."""
import functools

import numpy as np
import pytest

import _oracle as O
from minicv_amd import native as N
from minicv_amd import opencv
from minicv_amd import synthetic as S

pytestmark = pytest.mark.gpu

TILE = N.BATCH_PNP_TILE
W = N.BATCH_PNP_WIDTH
CV = "cv"   # OpenCV's own sample stream instead of a Philox seed
KINDS = {5: "AP3P", 1: "EPNP", 0: "Iterative"}
DIST = (0.08, -0.03, 0.002, -0.001)


# ---- problems and the two ways to solve them --------------------------------------------------------
def camera(p):
    """Problem p's own camera matrix and distortion (every third problem has none)."""
    K = np.array([[700.0 + 31.0 * (p % 11), 0, 640.0 - 13.0 * (p % 7)],
                  [0, 720.0 + 29.0 * (p % 5), 360.0 + 9.0 * (p % 5)], [0, 0, 1.0]])
    d = np.zeros(4) if p % 3 == 0 else np.array(DIST) * (1.0 + 0.25 * (p % 4))
    return K, d


@functools.lru_cache(maxsize=None)
def problem(n, seed, outl=0.4, cam=0):
    K, d = camera(cam)
    img, Wp, *_ = S.pnp_problem(n, seed=seed, outlier_frac=outl, sigma=0.3, K=K, dist=d)
    img.setflags(write=False)
    Wp.setflags(write=False)
    return img, Wp, K, d


def sizes(B):
    """N from 6 to ~600, odd and even, across the sweep's tile of 512."""
    base = [6, 599, 7, 50, 512, 128, 513, 33, 300, 64, 511, 9, 200]
    return [base[p % len(base)] + (p // len(base)) for p in range(B)]


def params(sampler, iters, fixed, refine=True, thr=2.0, conf=0.99):
    return opencv.RansacParams(threshold=thr, confidence=conf, max_iters=iters, seed=0 if sampler == CV else sampler,
                               fixed_iters=fixed, refine=refine, cv_sampler=sampler == CV)


def single(img, Wp, K, d, kind, p):
    """solvePnPRansac on one problem -> (ok, rvec, tvec, indices); a failure -> (False, zeros, zeros, empty)."""
    try:
        ok, r, t, idx = opencv.solvePnPRansac(img, Wp, K, d, kind=KINDS[kind], params=p)
    except (N.NativeError, ValueError):
        ok = False
    if not ok:
        return False, np.zeros(3), np.zeros(3), np.zeros(0, dtype=np.int32)
    return ok, r, t, idx


def loop(probs, kind, p):
    return [single(img, Wp, K, d, kind, p) for img, Wp, K, d in probs]


def batch(probs, kind, p):
    return opencv.solvePnPRansacBatch([q[0] for q in probs], [q[1] for q in probs], [q[2] for q in probs],
                                      [q[3] for q in probs], kind=KINDS[kind], params=p)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def assert_same(got, exp, what):
    assert len(got) == len(exp)
    for i, (g, e) in enumerate(zip(got, exp)):
        assert g[0] == e[0], (what, i, g[0], e[0])
        np.testing.assert_array_equal(g[3], e[3], err_msg=str((what, i)))
        np.testing.assert_array_equal(bits(g[1]), bits(e[1]), err_msg=str((what, i, "rvec")))
        np.testing.assert_array_equal(bits(g[2]), bits(e[2]), err_msg=str((what, i, "tvec")))


def stats():
    s = np.zeros(16, dtype=np.int64)
    assert N.lib().mcvTestBatchStats(s.ctypes.data) == 1
    return dict(launches=int(s[0]), syncs=int(s[1]), rounds=int(s[2]), lm_rounds=int(s[3]), single=int(s[4]),
                B=int(s[5]), problem_rounds=int(s[8]), copies=int(s[9]))


def mixed_sizes(B, seed0):
    return [problem(n, seed0 + i, 0.3 + 0.05 * (i % 5), cam=i) for i, n in enumerate(sizes(B))]


# ---- 1. the batched sweep on given poses -------------------------------------------------------------
SWEEP_N = (1, 5, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)
SWEEP_POSES = (1, W - 1, W, W + 1)


def batch_sweep(pts_list, cams, pose_list, thr2):
    offsets = np.zeros(len(pts_list) + 1, dtype=np.int32)
    offsets[1:] = np.cumsum([p.shape[0] for p in pts_list])
    poff = np.zeros(len(pose_list) + 1, dtype=np.int32)
    poff[1:] = np.cumsum([m.shape[0] for m in pose_list])
    pts = np.ascontiguousarray(np.concatenate(pts_list), dtype=np.float32)
    poses = np.ascontiguousarray(np.concatenate(pose_list), dtype=np.float64)
    cam8 = np.ascontiguousarray(np.stack(cams), dtype=np.float64)
    counts = np.full(int(poff[-1]), -7, dtype=np.int32)
    ok = N.lib().mcvTestBatchSweepPnp(pts.ctypes.data, offsets.ctypes.data, len(pts_list), cam8.ctypes.data,
                                      poses.ctypes.data, poff.ctypes.data, float(thr2), counts.ctypes.data)
    assert ok == 1, N.last_error()
    return [counts[poff[i]:poff[i + 1]] for i in range(len(pts_list))]


def cam8_of(K, d):
    return np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2], d[0], d[1], d[2], d[3]])


@functools.lru_cache(maxsize=None)
def sweep_case():
    """Per-problem N across the 512-row tile, pose counts across the 64-lane workgroup, a problem without poses,
    NaN, inf and zero poses, a pose that puts the points behind the camera, a NaN coordinate, cameras with and
    without distortion."""
    rng = np.random.default_rng(5)
    pts, cams, poses = [], [], []
    for i, n in enumerate(SWEEP_N):
        K, d = camera(i)
        img, Wp, _, _, _, R, t = S.pnp_problem(max(n, 8), seed=40 + i, outlier_frac=0.3, sigma=0.3, K=K, dist=d)
        k = SWEEP_POSES[i % 4]
        m = np.tile(np.concatenate([R.ravel(), t]), (k, 1))
        m += rng.normal(0, 2e-4, (k, 12)) * (np.arange(k) % 3 != 0)[:, None]
        if k > 5:
            m[1, 0] = np.nan
            m[2, 10] = np.inf
            m[3] = 0.0
            m[4, 9:] = [0.0, 0.0, -20.0]          # every point behind the camera
        pts.append(O.pack_pnp(img, Wp)[:n].copy())
        cams.append(cam8_of(K, d))
        poses.append(np.ascontiguousarray(m))
    pts[3][17, 1] = np.nan                                    # one point with a NaN coordinate
    pts.insert(2, pts[0].copy())                              # a problem with points and no poses
    cams.insert(2, cams[0].copy())
    poses.insert(2, np.zeros((0, 12)))
    return pts, cams, poses


def oracle_counts(pts, cams, poses, thr2):
    return [np.array([O.pnp_count(p, c, m[:9], m[9:], float(thr2))[0] for m in ms], dtype=np.int32)
            for p, c, ms in zip(pts, cams, poses)]


def boundary_thr2(pts1, cam, pose):
    """The fp32 error of one point under a pose: the smallest float32 threshold at which the oracle counts it
    (float32 bit patterns of non-negative values are ordered)."""
    lo, hi = 0, int(np.float32(1e30).view(np.uint32))
    assert O.pnp_count(pts1, cam, pose[:9], pose[9:], float(np.uint32(hi).view(np.float32)))[0] == 1
    while lo < hi:
        mid = (lo + hi) // 2
        if O.pnp_count(pts1, cam, pose[:9], pose[9:], float(np.uint32(mid).view(np.float32)))[0] == 1:
            hi = mid
        else:
            lo = mid + 1
    return np.uint32(lo).view(np.float32)


def test_batch_sweep_matches_oracle(gpu, oracle):
    pts, cams, poses = sweep_case()
    assert sorted(p.shape[0] for p in pts) == sorted(SWEEP_N + (1,))
    assert {m.shape[0] for m in poses} == set(SWEEP_POSES) | {0}
    for thr2 in (np.float32(4.0), np.float32(0.25)):
        got = batch_sweep(pts, cams, poses, thr2)
        exp = oracle_counts(pts, cams, poses, thr2)
        for i, (g, e) in enumerate(zip(got, exp)):
            np.testing.assert_array_equal(g, e, err_msg=f"problem {i} thr2 {thr2}")
    assert any(e.max(initial=0) > 0.5 * p.shape[0] for p, e in zip(pts, exp))   # the true poses do fit
    k = [i for i, m in enumerate(poses) if m.shape[0] > 5][0]
    assert exp[k][1] == 0 and exp[k][2] == 0          # a NaN or inf pose has no inliers


def test_batch_sweep_threshold_boundary(gpu, oracle):
    """thr2 equal to one point's fp32 error: the point counts (<=), and at the next float32 below it does not."""
    pts, cams, poses = sweep_case()
    i = len(pts) - 1            # the problem of 2 TILE + 1 points; its point in the third tile
    j = 2 * TILE
    e = boundary_thr2(pts[i][j:j + 1], cams[i], poses[i][0])
    assert 0 < e < 1e6
    below = np.nextafter(e, np.float32(0), dtype=np.float32)
    at = batch_sweep(pts, cams, poses, e)
    under = batch_sweep(pts, cams, poses, below)
    exp_at = oracle_counts(pts, cams, poses, e)
    exp_under = oracle_counts(pts, cams, poses, below)
    for g, x in zip(at + under, exp_at + exp_under):
        np.testing.assert_array_equal(g, x)
    assert at[i][0] - under[i][0] >= 1


# ---- 2. batch == loop of the single call, bit for bit --------------------------------------------------
@pytest.mark.parametrize("B", [1, 2, 65])
@pytest.mark.parametrize("sampler", [7, 123456789, CV])
@pytest.mark.parametrize("kind", [5, 1, 0])
def test_batch_equals_loop(gpu, kind, sampler, B):
    probs = mixed_sizes(B, 100)
    for fixed, refine, iters in ((False, True, 100), (True, True, 37), (False, False, 300), (True, False, 1)):
        p = params(sampler, iters, fixed, refine)
        got = batch(probs, kind, p)
        assert_same(got, loop(probs, kind, p), (kind, sampler, B, fixed, refine, iters))
        if iters >= 37:
            assert sum(g[0] for g in got) >= 0.5 * sum(q[0].shape[0] >= 30 for q in probs)


@pytest.mark.parametrize("kind", [5, 1, 0])
def test_batch_equals_loop_large_inlier_sets(gpu, kind):
    """N ~ 2300 at 10 % outliers has more than kEpnpBlock = 1024 inliers (the inlier EPnP sums two blocks);
    N = 257 and N = 1025 cross the reduction's and the EPnP pass's block sizes."""
    probs = [problem(2300, 61, 0.1, cam=1), problem(257, 62, 0.3, cam=2), problem(1025, 63, 0.3, cam=3)]
    for sampler in (CV, 11):
        p = params(sampler, 100, False)
        got = batch(probs, kind, p)
        assert got[0][0] and len(got[0][3]) > 1024
        assert_same(got, loop(probs, kind, p), (kind, sampler))


# ---- 3. a mixed batch ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mixed_case():
    """The problems of the mixed batch; MIXED_OK says which of them have a pose."""
    K, d = camera(1)
    K0 = K.copy()
    K0[0, 0] = 0.0
    full = problem(60, 70, 0.0, cam=1)
    rng = np.random.default_rng(9)
    same_img = np.tile(full[0][:1], (40, 1))
    same_w = np.tile(full[1][:1], (40, 1))
    probs = [
        (np.zeros((0, 2)), np.zeros((0, 3)), K, d),                                  # 0: N = 0
        (full[0][:3], full[1][:3], K, d),                                            # 1: N = 3
        (full[0][:4], full[1][:4], K, d),                                            # 2: N = 4: direct solve
        (full[0][:5], full[1][:5], K, d),                                            # 3: N = 5: direct (EPnP) / RANSAC (AP3P)
        (same_img, same_w, K, d),                                                    # 4: all points identical
        full,                                                                        # 5: all inliers
        problem(400, 71, 0.9, cam=1),                                                # 6: 90 % outliers
        (rng.uniform(0, 1200, (80, 2)), rng.uniform(-3, 3, (80, 3)), K, d),          # 7: pure noise
        (full[0], full[1], K0, d),                                                   # 8: fx = 0
        problem(200, 72, 0.5, cam=1),                                                # 9: an ordinary problem
        problem(400, 73, 0.7, cam=1),                                                # 10: 70 % outliers
    ]
    return probs


MIXED_ITERS, MIXED_THR = 300, 1.5
# What the definition (the oracle) returns for mixed_case() with this budget, per kind; the test checks it on the
# CPU before the GPU runs. 300 hypotheses do not find a pose at 90 % outliers; at 70 % the 4-point AP3P samples
# do and the 5-point EPnP samples do not. Identical points give no pose.
MIXED_OK = {0: False, 1: False, 2: True, 3: True, 4: False, 5: True, 6: False, 7: False, 8: False, 9: True,
            10: {5: True, 1: False}}


def mixed_ok(i, kind):
    v = MIXED_OK[i]
    return v[kind] if isinstance(v, dict) else v


@pytest.mark.parametrize("kind", [5, 1])
def test_mixed_batch(gpu, oracle, kind):
    probs = mixed_case()
    assert sorted(MIXED_OK) == list(range(len(probs)))          # no problem is skipped
    for i, (img, Wp, K, d) in enumerate(probs):
        rc = oracle.solve_pnp_ransac(img, Wp, K, d, thr=MIXED_THR, conf=0.99, max_iters=MIXED_ITERS, seed=3,
                                     flags=N.FLAG_FIXED_ITERS, kind=kind)[0]
        assert (rc > 0) == mixed_ok(i, kind), (i, rc)
    p = params(3, MIXED_ITERS, True, thr=MIXED_THR)
    got = batch(probs, kind, p)
    st, err = stats(), N.last_error()
    assert_same(got, loop(probs, kind, p), ("mixed", kind))
    for i in range(len(probs)):
        assert got[i][0] == mixed_ok(i, kind), (i, got[i][0])
        if not got[i][0]:
            assert not got[i][1].any() and not got[i][2].any() and len(got[i][3]) == 0
    assert "problem 0" in err and "cvSolvePnPRansacBatch" in err
    assert list(got[2][3]) == [0, 1, 2, 3]
    assert st["single"] == (2 if kind == 1 else 1) and st["B"] == len(probs)


# ---- 4. the oracle directly ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [5, 1, 0])
@pytest.mark.parametrize("refine", [True, False])
def test_batch_vs_oracle(gpu, oracle, kind, refine):
    probs = mixed_sizes(9, 200) + [problem(1500, 64, 0.5, cam=4)]
    iters, thr, seed = 150, 2.0, 5
    got = batch(probs, kind, params(seed, iters, False, refine, thr=thr))
    nok = 0
    for i, ((img, Wp, K, d), (ok, r, t, idx)) in enumerate(zip(probs, got)):
        rc, rr, rt, rmask, _ = oracle.solve_pnp_ransac(img, Wp, K, d, thr=thr, conf=0.99, max_iters=iters, seed=seed,
                                                       flags=0 if refine else N.FLAG_NO_REFINE, kind=kind)
        assert ok == (rc > 0), i
        if not ok:
            continue
        nok += 1
        np.testing.assert_array_equal(idx, np.nonzero(rmask)[0], err_msg=str(i))
        if not refine or kind != 0:
            np.testing.assert_allclose(r, rr, rtol=0, atol=1e-14, err_msg=str(i))
            np.testing.assert_array_equal(t, rt, err_msg=str(i))
        else:
            np.testing.assert_allclose(r, rr, rtol=1e-6, atol=1e-9, err_msg=str(i))
            np.testing.assert_allclose(t, rt, rtol=1e-6, atol=1e-9, err_msg=str(i))
    assert nok >= 6


# ---- 5. launches, synchronisations and copies do not depend on B ---------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
def test_stats_independent_of_B(gpu, kind):
    seen = []
    for B in (4, 64):
        probs = [problem(120 + (i % 7), 300 + i, 0.3, cam=i) for i in range(B)]
        got = batch(probs, kind, params(9, 60, True))
        assert all(g[0] for g in got)
        st = stats()
        assert st["B"] == B and st["single"] == 0 and st["rounds"] == 1 and st["problem_rounds"] == B
        assert st["lm_rounds"] <= 21
        seen.append(st)
    if kind == 1:
        assert seen[0]["lm_rounds"] == 0
        for key in ("launches", "syncs", "copies"):
            assert seen[0][key] == seen[1][key], (key, seen)
        assert seen[0]["syncs"] == 6
    else:
        # the LM steps of a batch are those of its slowest problem: 2 launches, 2 copies and 1
        # synchronisation each, whatever B is
        for s in seen:
            assert 1 <= s["lm_rounds"] <= 21
            assert s["syncs"] == 2 + s["lm_rounds"]
            assert s["launches"] == seen[0]["launches"] + 2 * (s["lm_rounds"] - seen[0]["lm_rounds"])
            assert s["copies"] == seen[0]["copies"] + 2 * (s["lm_rounds"] - seen[0]["lm_rounds"])


# ---- 6. a lowered cap: several rounds, problems dropping out ------------------------------------------
@pytest.mark.parametrize("kind", [5, 1, 0])
def test_lowered_cap_same_results(gpu, kind):
    probs = mixed_sizes(13, 400)
    p = params(CV, 200, False)
    ref = batch(probs, kind, p)
    one_round = stats()
    prev = N.lib().mcvTestBatchCap(13 * 16)
    try:
        got = batch(probs, kind, p)
        st = stats()
    finally:
        N.lib().mcvTestBatchCap(prev)
    assert_same(got, ref, ("cap", kind))
    assert one_round["rounds"] == 1
    assert st["rounds"] > 2 and st["problem_rounds"] < st["rounds"] * 13   # some problems stopped early
    assert_same(batch(probs, kind, p), ref, ("cap restored", kind))
    assert stats()["rounds"] == 1


# ---- 7. the Python wrapper -----------------------------------------------------------------------------
def test_wrapper_defaults_equal_loop(gpu):
    """params None: the native defaults (100 iterations, 8 px, 0.99, OpenCV's stream), as solvePnPRansac's."""
    probs = mixed_sizes(5, 500)
    for kind in ("AP3P", "EPNP", "Iterative"):
        got = opencv.solvePnPRansacBatch([q[0] for q in probs], [q[1] for q in probs], [q[2] for q in probs],
                                         [q[3] for q in probs], kind=kind)
        exp = [opencv.solvePnPRansac(*q, kind=kind) for q in probs]
        assert_same(got, exp, kind)
        assert all(g[3].dtype == np.int32 for g in got)
    nd = [(q[0], q[1], q[2], np.zeros(4)) for q in probs]
    got = opencv.solvePnPRansacBatch([q[0] for q in nd], [q[1] for q in nd], [q[2] for q in nd], None, kind="EPNP")
    assert_same(got, [opencv.solvePnPRansac(q[0], q[1], q[2], None, kind="EPNP") for q in nd], "no distortion")
