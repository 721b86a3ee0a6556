"""The homography sweep in self-pruning stages (key-only evaluations): the packed key, and everything
downstream of it, equals the unstaged sweep's and the oracle's.

Every staged case forces staging on (mcvTestHStaging mode 1), so the small shapes here take the staged
path, and compares both words of the key with (a) the same call made with a `counts` tensor, which is
never staged, and (b) the first maximum / first sampler failure of oracle.h_counts.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from minicv_amd import native as N
from minicv_amd import opencv, synthetic as S

pytestmark = pytest.mark.gpu

REL_TOL = 1e-6   # relative Frobenius tolerance on refined H (as tests/test_gpu_homography.py)
THR = 5e-3
NO_FAIL = 2**63 - 1
# stats[0] of mcvTestHStaging
PRUNED, NO_CANDIDATE, SAMPLER_FAILURE, LATE, FORCED_OFF, NOT_APPLICABLE = 0, 1, 2, 3, 4, 5

CASES = [
    # n, outlier fraction, sigma, thr, seed, maxIters, conf, flags (the first seven rows of
    # tests/test_gpu_homography.py's table)
    (4, 0.0, 1e-3, 5e-3, 1, 2000, 0.995, 0),
    (5, 0.2, 1e-3, 5e-3, 2, 2000, 0.995, 0),
    (8, 0.5, 1e-3, 5e-3, 3, 2000, 0.995, 0),
    (50, 0.5, 1e-3, 5e-3, 4, 2000, 0.995, 0),
    (200, 0.5, 1e-3, 5e-3, 5, 2000, 0.995, 0),
    (1000, 0.7, 1e-3, 5e-3, 6, 5000, 0.999, 0),
    (1000, 0.5, 1e-3, 5e-3, 7, 300, 0.995, N.FLAG_FIXED_ITERS),
]


def relf(A, B):
    return np.linalg.norm(np.asarray(A) - np.asarray(B)) / np.linalg.norm(B)


@pytest.fixture(scope="module")
def torch_dev(gpu):
    import torch
    return torch, torch.device("cuda:0")


def set_mode(mode):
    N.lib().mcvTestHStaging(mode, None)


def read_stats():
    """The calling thread's last homography evaluate: dict of mcvTestHStaging's stats."""
    st = (C.c_longlong * 16)()
    N.lib().mcvTestHStaging(-1, C.addressof(st))
    v = [int(x) for x in st]
    ns = v[2]
    return {"reason": v[0], "B": v[1], "stages": ns, "bounds": v[3:3 + ns + 1], "alive": v[10:10 + ns], "raw": v}


def evaluate(torch_dev, src, dst, seed, begin, count, thr, mode, with_counts=False):
    """-> (key words, stats, counts or None) of one mcvRansacEvaluate under staging mode `mode`."""
    torch, dev = torch_dev
    from minicv_amd import device as D
    n = src.shape[0]
    pts = D.pack_points_tensor(src, dst, dev)
    plan = D.RansacPlan(N.MODEL_HOMOGRAPHY, n, count)
    cfg = opencv.RansacParams(threshold=thr, seed=seed, fixed_iters=True, max_iters=max(count, 1)).to_c()
    key = torch.zeros(2, dtype=torch.int64, device=dev)
    counts = torch.zeros(count, dtype=torch.int32, device=dev) if with_counts else None
    set_mode(mode)
    try:
        plan.evaluate(pts, n, cfg, begin, count, key, counts)
        torch.cuda.synchronize()
        stats = read_stats()
    finally:
        set_mode(0)
    out = [int(v) for v in key.cpu().numpy()], stats, (counts.cpu().numpy() if with_counts else None)
    plan.close()
    return out


def oracle_key(oracle, src, dst, seed, begin, count, thr):
    """Key words from the oracle's counts: first maximum among counts >= 4 before the first failure."""
    ref = oracle.h_counts(oracle.pack4(src, dst), seed, begin, count, float(np.float32(thr * thr)))
    fail = np.nonzero(ref == -2)[0]
    lim = fail[0] if len(fail) else count
    k0 = 0
    if (ref[:lim] >= 4).any():
        c = ref[:lim].max()
        i = int(np.nonzero(ref[:lim] == c)[0][0])
        k0 = (int(c) << 32) | (0xFFFFFFFF - (begin + i))
    return [k0, begin + int(fail[0]) if len(fail) else NO_FAIL], ref


def check_keys(torch_dev, oracle, src, dst, seed, begin, count, thr, mode=1):
    """Staged key == unstaged key (counts tensor) == oracle key; -> (stats, oracle counts)."""
    key_s, stats, _ = evaluate(torch_dev, src, dst, seed, begin, count, thr, mode)
    key_u, stats_u, counts_u = evaluate(torch_dev, src, dst, seed, begin, count, thr, mode, with_counts=True)
    key_o, ref = oracle_key(oracle, src, dst, seed, begin, count, thr)
    assert stats_u["reason"] == NOT_APPLICABLE   # a caller that reads counts is never staged
    np.testing.assert_array_equal(counts_u, ref)
    assert key_u == key_o
    assert key_s == key_u
    return stats, ref


@pytest.mark.parametrize("n", [4, 5, 127, 128, 129, 255, 257, 1000])
def test_trip_edges(torch_dev, oracle, n):
    """Odd N, N below one trip (128 points), one point either side of a trip."""
    src, dst, _ = S.homography_problem(n, 40 + n % 7, outlier_frac=0.5)
    stats, _ = check_keys(torch_dev, oracle, src, dst, 40 + n % 7, 0, 2048, THR)
    assert stats["reason"] in (PRUNED, NO_CANDIDATE, SAMPLER_FAILURE, LATE)   # the staged path ran
    assert stats["stages"] >= 3 and stats["bounds"][0] == 0 and stats["bounds"][-1] == n


def test_pruning_is_not_vacuous(torch_dev, oracle):
    src, dst, _ = S.homography_problem(20000, 10)
    stats, ref = check_keys(torch_dev, oracle, src, dst, 10, 0, 4096, THR)
    print("stats", stats)
    assert stats["reason"] == PRUNED
    assert 0 < stats["B"] <= min(10009, int(ref.max()))   # 10009: the oracle's best count on these inputs
    alive = stats["alive"]
    assert alive[0] == alive[1] == 4096
    assert alive[2] / 4096 < 0.5
    assert all(a >= b for a, b in zip(alive, alive[1:]))
    assert all(a <= b for a, b in zip(stats["bounds"], stats["bounds"][1:]))
    assert alive[-1] >= 1   # the winner is never dropped


def test_ties_keep_lowest_index(torch_dev, oracle):
    src, dst, _ = S.homography_problem(500, 41, outlier_frac=0.0, sigma=0.0)
    stats, ref = check_keys(torch_dev, oracle, src, dst, 41, 0, 512, THR)
    full = int((ref == 500).sum())
    assert full > 1   # many hypotheses reach count N
    assert stats["reason"] == PRUNED and stats["B"] == 500
    # everyone who ties survives every compaction
    assert all(a >= full for a in stats["alive"])


def test_late_boundary_switches_itself_off(torch_dev, oracle):
    src, dst, _ = S.homography_problem(5000, 8, outlier_frac=0.9, sigma=2e-3)
    key_o, _ = oracle_key(oracle, src, dst, 8, 0, 4096, 1e-2)
    key0, stats0, _ = evaluate(torch_dev, src, dst, 8, 0, 4096, 1e-2, 0)
    assert stats0["reason"] != PRUNED
    assert key0 == key_o
    stats1, _ = check_keys(torch_dev, oracle, src, dst, 8, 0, 4096, 1e-2, mode=1)
    assert stats1["reason"] == LATE   # forced past the size rule, the boundary rule still holds
    assert stats1["alive"][2:] == [0] * (stats1["stages"] - 2)


def test_offsets_and_ragged_counts(torch_dev, oracle):
    src, dst, _ = S.homography_problem(3001, 42, outlier_frac=0.4)
    stats, _ = check_keys(torch_dev, oracle, src, dst, 42, 12345, 4099, THR)   # 4099 = 6 * 683 + 1
    assert stats["reason"] == PRUNED


def test_out_of_domain_models_and_non_finite_points(torch_dev, oracle):
    """The point set of test_counts_extreme_points: the bound's domain fails (non-finite extent), every
    slot takes the exact recount under staging."""
    src, dst, _ = S.homography_problem(300, 25, outlier_frac=0.3)
    rng = np.random.default_rng(25)
    src[:40] = src[40:80] * (1 + 1e-7 * rng.standard_normal((40, 2)))   # near-duplicates
    src[80:90, 1] = 0.5 * src[80:90, 0] + 0.1                           # collinear run
    src[90:95] *= 1e6
    dst[95:100] *= 1e-6
    src[100, 0] = np.nan
    dst[101, 1] = np.inf
    src[102] = [1e30, -1e30]
    check_keys(torch_dev, oracle, src, dst, 25, 0, 4096, THR)
    # the same set without the non-finite points: huge coordinates, finite extent
    keep = np.ones(300, dtype=bool)
    keep[[100, 101]] = False
    check_keys(torch_dev, oracle, src[keep], dst[keep], 25, 0, 4096, THR)


def test_sampler_failure_unstages_the_chunk(torch_dev, oracle):
    x = np.linspace(-1, 1, 30)
    src = np.stack([x, 0.25 * x], axis=1)
    dst = np.stack([x, -x], axis=1)
    key_s, stats, _ = evaluate(torch_dev, src, dst, 0, 0, 2048, 0.01, 1)
    key_o, ref = oracle_key(oracle, src, dst, 0, 0, 2048, 0.01)
    assert key_o[1] != NO_FAIL and (ref == -2).any()
    assert key_s[1] == key_o[1]
    assert stats["reason"] in (SAMPLER_FAILURE, NO_CANDIDATE)
    # the host falls back to the chunk's counts, which must be full: the oracle's outcome (no model)
    assert oracle.find_homography(src, dst, thr=0.01, flags=N.FLAG_FIXED_ITERS)[0] == 0
    set_mode(1)
    try:
        with pytest.raises(N.NativeError):
            opencv.findHomography(src, dst, opencv.RansacParams(threshold=0.01, fixed_iters=True))
    finally:
        set_mode(0)


@pytest.mark.parametrize("n,outl,sigma,thr,seed,iters,conf,flags", CASES)
def test_find_homography_fixed_iters_staged(gpu, oracle, n, outl, sigma, thr, seed, iters, conf, flags):
    src, dst, _ = S.homography_problem(n, seed, outlier_frac=outl, sigma=sigma)
    cnt_o, H_o, mask_o, _ = oracle.find_homography(src, dst, thr=thr, conf=conf, max_iters=iters, seed=seed,
                                                   flags=flags | N.FLAG_FIXED_ITERS)
    p = opencv.RansacParams(threshold=thr, confidence=conf, max_iters=iters, seed=seed, fixed_iters=True)
    set_mode(1)
    try:
        cnt, H, mask = opencv.findHomography(src, dst, p)
        if n > 4:   # N == 4 is the direct fit: no sweep; otherwise the staged path ran
            assert read_stats()["reason"] in (PRUNED, NO_CANDIDATE, SAMPLER_FAILURE, LATE)
    finally:
        set_mode(0)
    assert cnt == cnt_o
    np.testing.assert_array_equal(mask, mask_o.astype(bool))
    assert relf(H, H_o) < REL_TOL


def test_repeatable(torch_dev):
    src, dst, _ = S.homography_problem(20000, 10)
    k1, s1, _ = evaluate(torch_dev, src, dst, 10, 0, 4096, THR, 1)
    k2, s2, _ = evaluate(torch_dev, src, dst, 10, 0, 4096, THR, 1)
    assert k1 == k2
    assert s1 == s2


def test_mode_2_restores_the_single_sweep(torch_dev, oracle):
    src, dst, _ = S.homography_problem(20000, 10)
    k2, s2, _ = evaluate(torch_dev, src, dst, 10, 0, 4096, THR, 2)
    ku, _, _ = evaluate(torch_dev, src, dst, 10, 0, 4096, THR, 2, with_counts=True)
    assert s2["reason"] == FORCED_OFF
    assert k2 == ku == oracle_key(oracle, src, dst, 10, 0, 4096, THR)[0]
