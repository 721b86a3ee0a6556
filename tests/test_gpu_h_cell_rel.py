"""The second pass of the per-cell bound (candidate-relative test, per-slot `left`) on the device: bitmaps, upper
bounds and `left` figures equal the host twin's through mcvTestHCellRel, and the best key of a staged evaluate with
the new prune equals the key with the bound off, the unstaged key and the oracle's, on the paths where slots are
dropped and on those where nothing may be. Staging and the bound are forced on (mcvTestHStaging / mcvTestHCellMode
mode 1), so small shapes take the path."""
import numpy as np
import pytest

import _h_cell as HC
import _h_cell_rel as HR
import _oracle
from minicv_amd import native as N
from test_gpu_h_cell_bound import PRUNED, NO_CANDIDATE, SAMPLER_FAILURE, THR, THR2, check_keys, models_of, problem

pytestmark = pytest.mark.gpu


def check_alive(st):
    """Slots alive entering the stages in use never grow."""
    alive = st[10:10 + st[2]]
    assert all(a >= b for a, b in zip(alive, alive[1:])), alive
    return alive


@pytest.mark.parametrize("n", [4097, 8192, 20001])
def test_device_equals_host_twin(gpu, n):
    hyps = 2**12
    src, dst = problem(n, 3)
    pts4 = _oracle.pack4(src, dst)
    models = models_of(n, 3, hyps)
    cnt = _oracle.h_counts(pts4, 3, 0, hyps, THR2)
    cnt = cnt[cnt >= 0]
    best, B = models[int(np.argmax(cnt))], int(cnt.max())
    rng = np.random.default_rng(n)
    crafted = np.array([[1, 0, 0, 0, 1, 0, -4, 0], [1, 0, 0, 0, 1, 0, 0, 0], [0] * 8, [np.nan] + [0] * 7,
                        [1e30, 0, 0, 0, 1, 0, 0, 0], [1, 0, 0, 0, 1, 0, 1.2, 0.1], [1, 0, 0, 0, 1, 0, 0, np.inf]],
                       np.float32)
    near = (best[None, :] * (1 + np.exp(rng.uniform(np.log(1e-6), np.log(1e-1), (57, 1))) *
                             rng.standard_normal((57, 8)))).astype(np.float32)
    models = np.concatenate([models, crafted, near, best[None, :]])
    bounds = HR.boundaries(n)
    host = HR.run(N.lib(), pts4, best, models, THR2, B, bounds, device=0)
    dev = HR.run(N.lib(), pts4, best, models, THR2, B, bounds, device=1)
    np.testing.assert_array_equal(dev["cell"], host["cell"])
    np.testing.assert_array_equal(dev["bits"], host["bits"])
    np.testing.assert_array_equal(dev["ub"], host["ub"])
    np.testing.assert_array_equal(dev["left"], host["left"])
    assert dev["alive"] == host["alive"]
    HR.check_left(dev)
    box = HC.run(N.lib(), pts4, best, models, THR2, B, device=1)
    assert 0 < host["alive"] < box["alive"]               # the relative test drops slots the box test keeps
    # a crafted candidate too: its w = 0 line crosses the set
    host2 = HR.run(N.lib(), pts4, crafted[5], models, THR2, B, bounds, device=0)
    dev2 = HR.run(N.lib(), pts4, crafted[5], models, THR2, B, bounds, device=1)
    for k in ("cell", "bits", "ub", "left"):
        np.testing.assert_array_equal(dev2[k], host2[k])


@pytest.mark.parametrize("share", [0.0, 0.2, 0.5, 0.8, 0.95])
def test_key_over_outlier_shares(gpu, share):
    src, dst = problem(8192, 3, share)
    st, cs, ref = check_keys(src, dst, 3, 0, 2**14, THR)
    alive = check_alive(st)
    print(f"share {share}: reason {st[0]}, B {st[1]}, boundaries {st[3:8]}, alive {alive}")


@pytest.mark.parametrize("share", [0.6, 0.68])
def test_key_where_slots_skip_the_second_pass(gpu, share):
    """B below half of N with pruning on: the box pass keeps the slots whose other cells alone reach B out of the
    second pass (their `left` is the points not yet processed); the others go through it."""
    src, dst = problem(8192, 7, share)
    st, cs, ref = check_keys(src, dst, 7, 0, 2**14, THR, PRUNED)
    alive = check_alive(st)
    assert 2 * st[1] < 8192                   # the points outside the candidate's inliers alone exceed B
    print(f"share {share}: B {st[1]}, boundaries {st[3:8]}, alive {alive}")


@pytest.mark.parametrize("n", [5003, 8300])
def test_key_at_an_odd_n_and_a_partial_trip(gpu, n):
    src, dst = problem(n, 5)
    st, cs, ref = check_keys(src, dst, 5, 0, 2**12, THR, PRUNED)
    alive = check_alive(st)
    assert alive[1] < 2**12 // 2 and alive[-1] <= alive[1]
    print(f"n {n}: boundaries {st[3:8]}, alive {alive}")


def test_duplicated_winners_all_reach_the_last_stage(gpu):
    n = 4097
    src, dst = problem(n, 41, 0.0, 0.0)       # exact correspondences: many hypotheses reach count N
    src, dst = src.copy(), dst.copy()
    src[n // 2:] = src[:n - n // 2]
    dst[n // 2:] = dst[:n - n // 2]
    st, cs, ref = check_keys(src, dst, 41, 0, 1024, THR)
    alive = check_alive(st)
    full = int((ref == ref.max()).sum())
    assert full > 1 and alive[-1] >= full      # inclusive tests: every slot that ties survives every compaction


def test_sampler_failure_and_no_candidate_drop_nothing(gpu):
    x = np.linspace(-1, 1, 30)
    src = np.stack([x, 0.25 * x], axis=1)      # collinear: no sample passes the subset check
    dst = np.stack([x, -x], axis=1)
    st, cs, ref = check_keys(src, dst, 0, 0, 2048, 0.01, oracle_count=False)
    assert st[0] in (NO_CANDIDATE, SAMPLER_FAILURE)
    rng = np.random.default_rng(2)
    x = np.linspace(-1, 1, 5000)
    src2 = np.concatenate([np.stack([x, 0.25 * x], axis=1), rng.uniform(-1, 1, (4, 2))])
    dst2 = np.concatenate([np.stack([x, -x], axis=1), rng.uniform(-1, 1, (4, 2))])
    st2, cs2, ref2 = check_keys(src2, dst2, 0, 0, 2048, 0.01, SAMPLER_FAILURE, oracle_count=False)
    assert cs2[2] == int((ref2 >= 0).sum())    # pruning off: every slot with a model enters stage 1
