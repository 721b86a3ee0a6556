"""The stage plan of the staged homography sweep on the host (mcvHostHStagePlan: the function the planner kernel
runs): the boundaries' order and trip alignment, the half boundary in the middle of stage 1's range where the
per-cell bound's second pass runs, and the plans with pruning off. No device is touched."""
from pathlib import Path

import numpy as np
import pytest

from minicv_amd import native as N

TRIP = 64                      # pairs per trip of the certified sweep (64 lanes x kCertNP = 1)
PRUNED, NO_CANDIDATE, SAMPLER_FAILURE, LATE = 0, 1, 2, 3
NONE, BOX, BOTH = 0, 1, 2      # mcvHostHStagePlan's cellBound: no bound, its box pass alone, with its second pass
SLACK_DIV, LATEST256 = 64, 192  # kHStageSlackDiv, kHStageLatest256

SIZES = [4, 5, 127, 128, 129, 255, 257, 1000, 3001, 4097, 5000, 20000, 20001, 35001, 100000, 100001]


def plan(n, B, candidate=1, failure=0, cell=BOTH, subset=0):
    out = np.full(10, -7, np.int32)
    stages = N.lib().mcvHostHStagePlan(n, candidate, failure, B, cell, subset, out.ctypes.data)
    assert stages == out[1] == (5 if cell == BOTH else 4)      # the half boundary: only with the second pass
    return {"reason": int(out[0]), "stages": stages, "pa": int(out[2]), "bounds": [int(b) for b in out[3:3 + stages + 1]],
            "rest": [int(b) for b in out[3 + stages + 1:]]}


def shares(n):
    """Candidate counts from all inliers to few: early, middle and late first boundaries."""
    return sorted({n, n - 1, (9 * n) // 10, n // 2, n // 2 + 1, n // 3, n // 4, n // 10, 4 if n >= 4 else n, 0})


def check_common(p, n):
    nPairs, b = (n + 1) // 2, p["bounds"]
    assert b[0] == 0 and b[-1] == nPairs
    assert all(x <= y for x, y in zip(b, b[1:])), b
    assert all(x % TRIP == 0 or x == nPairs for x in b[:-1]), b      # stage ranges start trip-aligned (or are empty)
    assert p["rest"] == [0] * len(p["rest"])


def test_hook_is_declared_and_bound():
    txt = (Path(__file__).resolve().parents[1] / "include" / "minicv_native.h").read_text()
    assert "MCV_API int mcvHostHStagePlan(" in txt
    assert "mcvHostHStagePlan" in N.SIGNATURES and N.lib().mcvHostHStagePlan is not None
    assert N.lib().mcvHostHStagePlan(3, 1, 0, 3, 1, 0, np.zeros(10, np.int32).ctypes.data) == -1    # N < 4
    assert N.lib().mcvHostHStagePlan(100, 1, 0, 101, 1, 0, np.zeros(10, np.int32).ctypes.data) == -1  # B > N
    assert N.lib().mcvHostHStagePlan(100, 1, 0, 50, 1, 0, None) == -1
    assert N.lib().mcvHostHStagePlan(100, 1, 0, 50, 3, 0, np.zeros(10, np.int32).ctypes.data) == -1   # cellBound > 2


@pytest.mark.parametrize("subset", [0, 1])
@pytest.mark.parametrize("cell", [NONE, BOX, BOTH])
@pytest.mark.parametrize("n", SIZES)
def test_boundaries_are_ordered_and_trip_aligned(n, cell, subset):
    for B in shares(n):
        p = plan(n, B, cell=cell, subset=subset)
        check_common(p, n)
        # stage 1 starts at the prefix, or at point 0 when stage 0 ran on a subset (only with the bound)
        assert p["bounds"][1] == (0 if cell and subset else p["pa"])
        assert p["pa"] % TRIP == 0 and 2 * p["pa"] <= n
        if n >= 2 * TRIP:
            assert p["pa"] >= TRIP


@pytest.mark.parametrize("subset", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_half_boundary_is_the_middle_of_stage_1(n, subset):
    seen = set()
    for B in shares(n):
        p, q = plan(n, B, cell=BOTH, subset=subset), plan(n, B, cell=NONE)
        r = plan(n, B, cell=BOX, subset=subset)
        assert r["reason"] == p["reason"] and r["pa"] == p["pa"]
        assert r["bounds"] == p["bounds"][:2] + p["bounds"][3:]            # the box pass alone: the same plan without it
        if p["reason"] != PRUNED:
            continue
        start, mid, p1 = p["bounds"][1:4]
        # the middle of [start, p1), rounded down to a trip: within half a trip of the exact middle, at a trip
        assert start <= mid <= p1 and (mid - start) % TRIP == 0
        assert abs(2 * mid - (start + p1)) <= TRIP
        assert mid == start + (p1 - start) // TRIP // 2 * TRIP
        # the first pruning boundary is the points a slot may miss before it falls below B, plus the slack
        want = -(-((n - B + n // SLACK_DIV + 1) // 2) // TRIP) * TRIP
        assert p1 == max(p["pa"], want)
        # the later boundaries split the rest as in the plan without the half boundary, whose own first boundary
        # differs only through its longer prefix
        trips = ((n + 1) // 2 - p1) // TRIP
        assert p["bounds"][4:] == [p1 + trips // 2 * TRIP, (n + 1) // 2]
        if q["reason"] == PRUNED and q["bounds"][2] == p1:
            assert q["bounds"][3:] == p["bounds"][4:]
        seen.add(p1 == start)
        if subset:                                                     # from point 0 stage 1 is empty only where
            assert start == 0 and (p1 > 0 or (B == n and n < SLACK_DIV))   # no point may be missed and N has no trip
    assert seen or n < 4 * TRIP                                        # some share prunes at every size with two trips


@pytest.mark.parametrize("n,B", [(500, 500), (1000, 1000), (4097, 4097), (8192, 8192)])
def test_stage_1_empty_where_the_first_boundary_is_the_prefix(n, B):
    """Nearly every point an inlier: the first boundary falls on the prefix, p1 == pa, stage 1 is empty without a
    subset, and the half boundary collapses onto it."""
    p = plan(n, B, cell=BOTH, subset=0)
    assert p["reason"] == PRUNED
    assert p["bounds"][1] == p["bounds"][2] == p["bounds"][3] == p["pa"]
    check_common(p, n)
    s = plan(n, B, cell=BOTH, subset=1)
    assert s["bounds"][1] == 0 and s["bounds"][3] == s["pa"] and s["bounds"][2] == s["pa"] // TRIP // 2 * TRIP
    # the plain stages (no bound, a longer prefix): the same collapse at large N, and no half boundary
    q = plan(20000, 19990, cell=NONE)
    assert q["reason"] == PRUNED and q["bounds"][1] == q["bounds"][2] == q["pa"] == 640


@pytest.mark.parametrize("subset", [0, 1])
@pytest.mark.parametrize("cell", [NONE, BOX, BOTH])
@pytest.mark.parametrize("n", SIZES)
def test_pruning_off_runs_stage_1_to_the_end(n, cell, subset):
    nPairs = (n + 1) // 2
    late_B = max(0, n - (nPairs * LATEST256 // 256) * 2 - TRIP * 2)    # first boundary beyond 192 / 256 of the pairs
    for kw, reason in ((dict(candidate=0, B=0), NO_CANDIDATE), (dict(candidate=0, failure=1, B=0), NO_CANDIDATE),
                       (dict(failure=1, B=n // 2), SAMPLER_FAILURE), (dict(B=min(late_B, n // 8)), LATE)):
        p = plan(n, cell=cell, subset=subset, **kw)
        assert p["reason"] == reason, (kw, p)
        check_common(p, n)
        assert p["bounds"][2:] == [nPairs] * (p["stages"] - 1)         # every later boundary is nPairs


@pytest.mark.parametrize("n", [4, 5, 127])
def test_fewer_points_than_a_trip(n):
    """No whole trip: the prefix is empty and a first boundary behind point 0 is the end, so the plan does not
    prune; with B == N and no slack the first boundary is point 0 and every stage but the last is empty."""
    for B in sorted(set(range(0, n + 1, max(1, n // 5))) | {n}):
        for subset in (0, 1):
            p = plan(n, B, subset=subset)
            assert p["pa"] == 0
            if n - B + n // SLACK_DIV == 0:
                assert p["reason"] == PRUNED and p["bounds"] == [0] * 5 + [(n + 1) // 2]
            else:
                assert p["reason"] == LATE and p["bounds"] == [0, 0] + [(n + 1) // 2] * 4


def test_headline_shape():
    """100000 correspondences, B = 50168, stage 0 on a subset: the parent's boundaries and the new one between."""
    p = plan(100000, 50168, cell=BOTH, subset=1)
    assert p["reason"] == PRUNED
    assert p["bounds"] == [0, 0, 12864, 25728, 37824, 50000]
    q = plan(100000, 50168, cell=NONE)
    assert q["bounds"] == [0, 3136, 25728, 37824, 50000]
