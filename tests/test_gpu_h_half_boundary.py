"""The half boundary of the staged homography sweep: where the per-cell bound's second pass runs the plan has 5
stages (0, 1a, 1b, 2, 3), a compaction behind each list stage and one recount behind the last; with the box pass
alone it keeps 4. The best key equals the unstaged key and the oracle's on the paths where slots are dropped, where
a stage is empty and where nothing may be dropped. Staging and the bound are forced on by the hooks, so small shapes
take the path. Each test prints its boundaries and the slots alive entering the stages (-s)."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import _h_cell as HC
import _h_cell_rel as HR
import _oracle
from minicv_amd import native as N, opencv, synthetic as S
from _h_stage import (LATE, NO_CANDIDATE, NO_FAIL, ON, PRUNED, SAMPLER_FAILURE, THR, THR2, evaluate, oracle_key, pack,
                      problem)

pytestmark = pytest.mark.gpu

REL_BASE = 4 ** 4    # first cell of the candidate's inliers (the 4-D grid comes first)


@contextlib.contextmanager
def second_pass(mode):
    prev = N.lib().mcvTestHCellSecondPass(mode)
    try:
        yield
    finally:
        N.lib().mcvTestHCellSecondPass(prev)


@contextlib.contextmanager
def forced():
    """Staging and the bound forced on around a call that is not _h_stage.evaluate."""
    L = N.lib()
    ps, pc = L.mcvTestHStaging(1, None), L.mcvTestHCellMode(ON, 0, 0, None)
    try:
        yield
    finally:
        L.mcvTestHStaging(ps, None)
        L.mcvTestHCellMode(pc, 0, 0, None)


@contextlib.contextmanager
def sweep_form(form):
    """mcvTestHMfma's form of the certified sweep (0 automatic, 2 the matrix cores for the list stages too)."""
    prev = N.lib().mcvTestHMfma(form, None)
    try:
        yield
    finally:
        N.lib().mcvTestHMfma(prev, None)


def stages_of(st):
    ns = st[2]
    return {"reason": st[0], "B": st[1], "stages": ns, "bounds": st[3:3 + ns + 1], "alive": st[10:10 + ns]}


def check_staged(st, n, count, stages=5):
    """The stage count (5 with the second pass, 4 without), ordered boundaries, alive never grows; -> the dict."""
    s = stages_of(st)
    assert s["stages"] == stages
    assert s["bounds"][0] == 0 and s["bounds"][-1] == n
    assert all(a <= b for a, b in zip(s["bounds"], s["bounds"][1:])), s
    assert s["alive"][0] <= count and s["alive"][1] <= count
    assert all(a >= b for a, b in zip(s["alive"][1:], s["alive"][2:])), s     # alive[0]: the slots stage 0 swept
    if s["reason"] == PRUNED:
        assert s["alive"][-1] >= 1                                              # the winner is never dropped
    else:
        assert s["alive"][2:] == [0] * (stages - 2)                             # stage 1 ran every slot to the end
    return s


def three_paths(src, dst, seed, begin, count, thr, oracle_count=True, stage0=0):
    """Staged + bound + second pass == staged + bound only == unstaged (a counts tensor) == oracle.
    -> (stages of the first, of the second, the oracle's counts)"""
    n = src.shape[0]
    pts = pack(src, dst)
    key_o, ref = oracle_key(src, dst, seed, begin, count, thr)
    key_2, st_2, cs_2, _ = evaluate(pts, n, seed, begin, count, thr, 1, ON, stage0=stage0)
    with second_pass(2):
        key_1, st_1, cs_1, _ = evaluate(pts, n, seed, begin, count, thr, 1, ON, stage0=stage0)
    key_u, st_u, _, full = evaluate(pts, n, seed, begin, count, thr, 1, ON, stage0=stage0, counts=True)
    assert st_u[0] == 5                                   # a counts tensor: the call does not stage
    assert cs_2[0] == 1 and cs_1[0] == 1                  # the bound ran
    if oracle_count:
        np.testing.assert_array_equal(full, ref)
        assert key_u == key_o
    else:
        assert key_u[1] == key_o[1]
        np.testing.assert_array_equal(full[ref >= 0], ref[ref >= 0])
    assert key_2 == key_u and key_1 == key_u
    s2, s1 = check_staged(st_2, n, count), check_staged(st_1, n, count, stages=4)
    print(f"n {n} x {count}: reason {s2['reason']}, B {s2['B']}, boundaries {s2['bounds']}, alive with the second pass "
          f"{s2['alive']}, box pass alone {s1['alive']}")
    # the box pass alone: the same plan without the half boundary; the second pass only drops more
    assert s2["bounds"][:2] + s2["bounds"][3:] == s1["bounds"] and s2["B"] == s1["B"]
    assert all(a <= b for a, b in zip(s2["alive"][1:2] + s2["alive"][3:], s1["alive"][1:]))
    return s2, s1, ref


@pytest.mark.parametrize("n,seed,share,begin,count,pruned", [(3001, 42, 0.4, 12345, 4099, True),   # 4099 = 6 * 683 + 1
                                                             (20000, 10, 0.5, 0, 4096, True),
                                                             (129, 3, 0.5, 0, 4096, False)])
def test_key_over_three_paths(gpu, n, seed, share, begin, count, pruned):
    src, dst = problem(n, seed, share)
    s2, s1, _ = three_paths(src, dst, seed, begin, count, THR)
    if pruned:
        assert s2["reason"] == PRUNED and s1["reason"] == PRUNED
        start, mid, p1 = s2["bounds"][1:4]
        assert start < mid < p1 and abs(2 * mid - (start + p1)) <= 128         # the half boundary, within a trip
        assert s2["alive"][-1] < s2["alive"][1]                                 # not vacuous: slots are dropped
    # stage 0 on a leading subset: stage 1a starts at point 0
    t2, _, _ = three_paths(src, dst, seed, begin, count, THR, stage0=256)
    assert t2["bounds"][1] == 0 and t2["alive"][0] == 256


def test_alive_counts_equal_the_host_recomputation(gpu):
    """The alive counts of the five stages against the boundaries' test recomputed on the host: a slot is alive behind a
    boundary when its count so far (the oracle's mask over the points before the boundary) + left >= B, with `left`
    from the host twins of the two bound passes. Equalities: neither side involves randomness."""
    n, seed, count = 3001, 42, 2048
    src, dst = problem(n, seed, 0.4)
    pts4 = _oracle.pack4(src, dst)
    key_o, ref = oracle_key(src, dst, seed, 0, count, THR)
    key, st, cs, _ = evaluate(pack(src, dst), n, seed, 0, count, THR, 1, ON)
    s = check_staged(st, n, count)
    assert key == key_o and s["reason"] == PRUNED
    B, bounds = s["B"], s["bounds"]
    assert all(b % 2 == 0 for b in bounds[:-1])
    have = np.nonzero(ref >= 0)[0]
    models = np.zeros((len(have), 8), np.float32)
    for k, h in enumerate(have):
        status, _, hf, _ = _oracle.h_hypothesis(pts4, seed, int(h))
        assert status >= 0
        models[k] = hf
    cnt, m = HC.masks(_oracle, pts4, models, THR2)
    np.testing.assert_array_equal(cnt, ref[have])
    # the candidate: the best count over stage 0's prefix, lowest index first; its full count is B
    prefix = m[:, :bounds[1]].sum(1)
    cand = int(np.argmax(prefix))
    assert cnt[cand] == B
    later = np.array([b // 2 for b in bounds[2:5]], np.int32)                  # the three boundaries with a `left` row
    box = HC.run(N.lib(), pts4, models[cand], models, THR2, B, device=0)
    rel = HR.run(N.lib(), pts4, models[cand], models, THR2, B, later, device=0)
    open_rel = (box["sizes"][None, REL_BASE:] * ~box["cert"][:, REL_BASE:]).sum(1)
    keep = box["ub"] >= B
    second = keep & (box["ub"] - open_rel < B)            # the slots the relative test can still drop
    alive = (keep & ~second) | (second & (rel["ub"] >= B))
    assert int(alive.sum()) == s["alive"][1] == cs[2]
    want = []
    for j, b in enumerate(bounds[2:5]):
        left = np.where(second, rel["left"][j], n - min(n, b))                  # the others: the points not processed
        alive = alive & (m[:, :b].sum(1) + left >= B)
        want.append(int(alive.sum()))
    print(f"B {B}, boundaries {bounds}, alive {s['alive']}, recomputed {want}")
    assert want == s["alive"][2:]
    assert want[0] > want[-1] >= 1                         # the boundaries drop slots, the winner stays


@pytest.mark.parametrize("stage0", [0, 256])
def test_empty_stage_hands_its_list_on(gpu, stage0):
    """B = N: the first pruning boundary falls on the prefix, so stages 1a and 1b are empty (from a subset: 1a
    alone, the half boundary sits on point 0) and must hand their lists on; every slot that ties at N is alive in
    the last stage (the inclusive test)."""
    n, count = 500, 512
    src, dst = problem(n, 41, 0.0, 0.0)
    s2, s1, ref = three_paths(src, dst, 41, 0, count, THR, stage0=stage0)
    full = int((ref == n).sum())
    assert full > 1 and s2["reason"] == PRUNED and s2["B"] == n
    b = s2["bounds"]
    assert (b[1] == b[2]) if stage0 else (b[1] == b[2] == b[3])                 # the empty stages
    for s in (s2, s1):
        assert all(a >= full for a in s["alive"][1:])
    if not stage0:
        assert s2["alive"][1] == s2["alive"][2] == s2["alive"][3]               # handed on: nothing changed, nothing lost


def check_find_homography(src, dst, thr):
    """cvFindHomography under forced staging + bound against the oracle: the count and the mask, or both fail."""
    cnt_o, H_o, mask_o, _ = _oracle.find_homography(src, dst, thr=thr, flags=N.FLAG_FIXED_ITERS)
    p = opencv.RansacParams(threshold=thr, fixed_iters=True)
    with forced():
        if cnt_o == 0:
            with pytest.raises(N.NativeError):
                opencv.findHomography(src, dst, p)
            return
        cnt, H, mask = opencv.findHomography(src, dst, p)
        st = (C.c_longlong * 16)()
        N.lib().mcvTestHStaging(-1, C.addressof(st))
        assert st[2] == 5                                  # the staged path with the half boundary ran
    assert cnt == cnt_o
    np.testing.assert_array_equal(mask, mask_o.astype(bool))


def test_late_boundary_lists_nothing(gpu):
    src, dst = problem(5000, 8, 0.9, 2e-3)
    s2, s1, _ = three_paths(src, dst, 8, 0, 4096, 1e-2)
    assert s2["reason"] == LATE and s1["reason"] == LATE
    assert s2["alive"][2:] == [0, 0, 0]
    check_find_homography(src, dst, 1e-2)


def test_sampler_failure_lists_nothing(gpu):
    """5000 collinear points and four off the line: a candidate, then a hypothesis that exhausts the sampler. The
    stage behind boundary 1 runs every slot to the end, and the host's fallback reads full counts."""
    rng = np.random.default_rng(2)
    x = np.linspace(-1, 1, 5000)
    src = np.concatenate([np.stack([x, 0.25 * x], axis=1), rng.uniform(-1, 1, (4, 2))])
    dst = np.concatenate([np.stack([x, -x], axis=1), rng.uniform(-1, 1, (4, 2))])
    key_o, ref = oracle_key(src, dst, 0, 0, 2048, 0.01)
    assert key_o[1] != NO_FAIL and (ref[:key_o[1]] >= 0).any()
    s2, s1, _ = three_paths(src, dst, 0, 0, 2048, 0.01, oracle_count=False)
    assert s2["reason"] == SAMPLER_FAILURE and s1["reason"] == SAMPLER_FAILURE
    assert s2["alive"][2:] == [0, 0, 0]
    check_find_homography(src, dst, 0.01)
    # no model at all: no candidate
    x = np.linspace(-1, 1, 30)
    src, dst = np.stack([x, 0.25 * x], axis=1), np.stack([x, -x], axis=1)
    t2, _, _ = three_paths(src, dst, 0, 0, 2048, 0.01, oracle_count=False)
    assert t2["reason"] in (NO_CANDIDATE, SAMPLER_FAILURE)
    check_find_homography(src, dst, 0.01)


def test_recount_marks_with_one_recount(gpu):
    """The point set of test_out_of_domain_models_and_non_finite_points under the forced bound: waves that leave
    the certificate's domain mark their slots, no compaction lists a marked slot, and the one recount behind the
    last stage gives them their full counts."""
    src, dst, _ = S.homography_problem(300, 25, outlier_frac=0.3)
    rng = np.random.default_rng(25)
    src[:40] = src[40:80] * (1 + 1e-7 * rng.standard_normal((40, 2)))   # near-duplicates
    src[80:90, 1] = 0.5 * src[80:90, 0] + 0.1                           # collinear run
    src[90:95] *= 1e6
    dst[95:100] *= 1e-6
    src[100, 0] = np.nan
    dst[101, 1] = np.inf
    src[102] = [1e30, -1e30]
    three_paths(src, dst, 25, 0, 4096, THR)
    keep = np.ones(300, dtype=bool)
    keep[[100, 101]] = False                                            # huge coordinates, finite extent
    three_paths(src[keep], dst[keep], 25, 0, 4096, THR)
    # coordinates of 2e7 among unit ones: some models leave the domain, the others prune (the set of
    # test_redo_slots_of_stage_0_stay_out_of_the_list)
    src, dst = problem(4300, 25, 0.3)
    src, dst = src.copy(), dst.copy()
    src[90:95] *= 2e7
    dst[95:100] *= 2e7
    three_paths(src, dst, 25, 0, 4096, THR)


def test_matrix_core_list_form(gpu):
    """kHFormMfma (mcvTestHMfma 2) runs the list stages on the matrix cores: the same five stages and lists, so the
    key and every alive count equal the default form's."""
    n, count = 4097, 4096
    src, dst = problem(n, 3)
    pts = pack(src, dst)
    key_o, _ = oracle_key(src, dst, 3, 0, count, THR)
    key_v, st_v, _, _ = evaluate(pts, n, 3, 0, count, THR, 1, ON)
    with sweep_form(2):
        key_m, st_m, _, _ = evaluate(pts, n, 3, 0, count, THR, 1, ON)
        ms = (C.c_longlong * 3)()
        N.lib().mcvTestHMfma(-1, C.addressof(ms))
    assert ms[0] >= 0 and N.lib().mcvTestHMfma(-1, None) == 0                   # the form is restored
    assert key_v == key_m == key_o
    sv, sm = check_staged(st_v, n, count), check_staged(st_m, n, count)
    print(f"default form {sv}, matrix-core list form {sm}")
    assert sv == sm and sv["reason"] == PRUNED
