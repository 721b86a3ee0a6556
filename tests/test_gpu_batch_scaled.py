"""GPU parity of the batched findScaled (cvFindScaledPoseBatch, cvFindScaledPoseBatchCosts,
camera.findScaledBatch): every problem of a batch against the oracle and against its own
cvFindScaledPose call.

Bar: bit-exact. Every comparison is array_equal on values; none has a tolerance."""
import functools
import math

import numpy as np
import pytest

import _scaled_batch as B
from minicv_amd import camera as CM, native as N, synthetic as S

pytestmark = pytest.mark.gpu

# launches, synchronisations, copies, memsets of cvFindScaledPoseBatch and of the costs helper
TABLE_BATCH = (4, 1, 4, 0)
TABLE_COSTS = (3, 1, 5, 0)


def stats():
    st = np.zeros(8, np.int64)
    assert N.lib().mcvTestScaledBatchStats(st.ctypes.data) == 0
    return st


@functools.lru_cache(maxsize=None)
def mixed_device():
    return B.call("cvFindScaledPoseBatch", B.mixed())


@functools.lru_cache(maxsize=None)
def mixed_single():
    return B.single_results(B.mixed())


def test_mixed_batch_equals_oracle(gpu, oracle):
    b = B.mixed()
    k, costs, scales, ev, _ = mixed_device()
    assert k >= 0, N.last_error()
    ref = B.oracle_results(oracle, b)
    B.assert_results((costs, scales, ev), ref, "batch against the oracle")
    assert k == int(np.isfinite(ref[0]).sum())
    assert costs[0] == math.inf and costs[-1] == math.inf and ev[0] == 0 and ev[-1] == 0


def test_mixed_batch_equals_single_calls(gpu):
    k, costs, scales, ev, _ = mixed_device()
    ref = mixed_single()
    B.assert_results((costs, scales, ev), ref, "batch against cvFindScaledPose")
    assert k == int(np.isfinite(ref[0]).sum())


def test_mixed_batch_costs_equal_oracle(gpu, oracle):
    b = B.mixed()
    k, sc, co, starts = B.call_costs(b)
    assert k == int(b.sizes().sum()), N.last_error()
    for p in range(b.P):
        W, O = b.set_of(p)
        if W.shape[0] == 0:
            assert starts[p] == starts[p + 1]
            continue
        sc_ref, co_ref, _ = oracle.scaled_costs(B.cam14(b.cams[p]), W, O, b.poses[p].Rotation,
                                                b.poses[p].Translation)
        np.testing.assert_array_equal(sc[starts[p]:starts[p + 1]], sc_ref, err_msg=f"scales of problem {p}")
        np.testing.assert_array_equal(co[starts[p]:starts[p + 1]], co_ref, err_msg=f"costs of problem {p}")
    assert tuple(stats()[:4]) == TABLE_COSTS
    lists = CM.findScaledBatchCosts(b.cams, b.sets, b.poses, b.set_idx)
    for p in range(b.P):
        np.testing.assert_array_equal(lists[p][0], sc[starts[p]:starts[p + 1]])
        np.testing.assert_array_equal(lists[p][1], co[starts[p]:starts[p + 1]])


def test_set_idx_none_and_reversed(gpu):
    b = B.mixed()
    ref = mixed_device()[1:4]
    e = b.expanded()
    k, costs, scales, ev, _ = B.call("cvFindScaledPoseBatch", e)
    assert k >= 0 and e.set_idx is None and e.S == e.P, N.last_error()
    B.assert_results((costs, scales, ev), ref, "setIdx = None")
    for r in (b.reversed(), e.reversed()):
        k, costs, scales, ev, _ = B.call("cvFindScaledPoseBatch", r)
        assert k >= 0, N.last_error()
        B.assert_results((costs, scales, ev), tuple(a[::-1] for a in ref), "reversed")


def test_all_skipped_between_two_problems(gpu):
    """An all-skipped problem (test_gpu_scaled.py::test_empty_and_all_skipped: every observation at
    the translation's image, so n is tiny) between two normal ones."""
    src, pose, W, O, _ = S.scaled_problem(20, seed=9)
    dst0 = CM.transformed_view(CM.transformation(CM.scale(0.0, pose)), src)
    basis = np.eye(4)
    basis[:3, 0], basis[:3, 1], basis[:3, 2], basis[:3, 3] = dst0.right, dst0.up, -dst0.forward, dst0.location
    src_b = np.eye(4)
    src_b[:3, 0], src_b[:3, 1], src_b[:3, 2] = src.right, src.up, -src.forward
    t = np.linalg.inv(basis)[:3, :3] @ (src_b[:3, :3] @ (pose.Rotation @ pose.Translation))
    t = t / np.linalg.norm(t)
    O2 = np.ascontiguousarray(np.tile(t[:2] / t[2], (20, 1)))
    a, c = B.make_sets((70, 45), 40)
    b = B.Batch([a[0], src, c[0]], [a[1], pose, c[1]], [(a[2], a[3]), (W, O2), (c[2], c[3])], None)
    k, costs, scales, ev, _ = B.call("cvFindScaledPoseBatch", b)
    assert k == 2, N.last_error()
    assert costs[1] == math.inf and scales[1] == 0.0 and ev[1] == 0
    B.assert_results((costs, scales, ev), B.single_results(b), "all-skipped in the middle")
    alone = B.Batch([a[0], c[0]], [a[1], c[1]], [(a[2], a[3]), (c[2], c[3])], None)
    k, costs2, scales2, ev2, _ = B.call("cvFindScaledPoseBatch", alone)
    B.assert_results((costs2, scales2, ev2), (costs[[0, 2]], scales[[0, 2]], ev[[0, 2]]), "neighbours")


def test_setup_is_read_per_problem(gpu):
    """Two problems on one set that differ only in the translation's sign, two only in the focal length."""
    (src, pose, W, O), = B.make_sets((150,), 60)
    flipped = CM.CameraPose(pose.RotationIndex, pose.ScaleSign, pose.Rotation, -pose.Translation, False)
    zoomed = CM.Camera(src.location, src.forward, src.up, src.right, src.focal * 1.1)
    b = B.Batch([src, src, zoomed], [pose, flipped, pose], [(W, O)], [0, 0, 0])
    k, costs, scales, ev, _ = B.call("cvFindScaledPoseBatch", b)
    assert k >= 2, N.last_error()
    B.assert_results((costs, scales, ev), B.single_results(b), "one set, three setups")
    assert (costs[0], scales[0]) != (costs[1], scales[1]) and (costs[0], scales[0]) != (costs[2], scales[2])


def test_one_problem(gpu):
    b = B.build((137,), None, 70)
    k, costs, scales, ev, _ = B.call("cvFindScaledPoseBatch", b)
    assert k == 1, N.last_error()
    B.assert_results((costs, scales, ev), B.single_results(b), "P = 1")


def test_more_problems_than_lanes_and_launch_counts(gpu):
    """The counts of a call (DESIGN §7j's table) do not depend on P: the same after 3 and after 67
    problems, with exactly one synchronisation."""
    three = B.build((40, 40, 40), None, 300)
    k, *_ = B.call("cvFindScaledPoseBatch", three)
    assert k >= 0, N.last_error()
    st3 = stats()
    b = B.many()
    k, costs, scales, ev, _ = B.call("cvFindScaledPoseBatch", b)
    assert k >= 0 and b.P == 67, N.last_error()
    st67 = stats()
    B.assert_results((costs, scales, ev), B.single_results(b), "P = 67")
    np.testing.assert_array_equal(st3[:4], st67[:4])
    assert tuple(st67[:4]) == TABLE_BATCH and st67[1] == 1
    assert st3[4] == 3 and st67[4] == 67 and st3[5] == 3 * 2 and st67[5] == 67 * 2   # 80 candidates: 2 tiles


def test_find_scaled_batch_equals_find_scaled(gpu):
    b = B.mixed()
    got = CM.findScaledBatch(0.01, b.cams, b.sets, b.poses, b.set_idx)
    assert len(got) == b.P
    for p in range(b.P):
        cost, pose = CM.findScaled(0.01, b.cams[p], b.set_of(p), b.poses[p])
        assert got[p][0] == cost
        np.testing.assert_array_equal(got[p][1].Translation, pose.Translation)
        np.testing.assert_array_equal(got[p][1].Rotation, pose.Rotation)
        assert got[p][1].ScaleSign == pose.ScaleSign and got[p][1].RotationIndex == pose.RotationIndex
    # list-of-pairs sets and one set per problem
    e = b.expanded()
    lists = [[(W[i], O[i]) for i in range(W.shape[0])] for W, O in e.sets[:5]]
    got5 = CM.findScaledBatch(0.01, e.cams[:5], lists, e.poses[:5])
    for p in range(5):
        assert got5[p][0] == got[p][0] and got5[p][1].ScaleSign == got[p][1].ScaleSign
        np.testing.assert_array_equal(got5[p][1].Translation, got[p][1].Translation)


def test_evaluated_may_be_null(gpu):
    b = B.mixed()
    k, costs, scales, ev, _ = B.call("cvFindScaledPoseBatch", b, evaluated=False)
    ref = mixed_device()
    assert k == ref[0] and np.all(ev == B.SENT_I)
    B.assert_results((costs, scales), ref[1:3], "evaluated = None")
