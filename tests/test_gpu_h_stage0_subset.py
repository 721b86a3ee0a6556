"""Stage 0 of the staged homography sweep on a leading subset of the slots (mcvTestHStage0Slots): the candidate
comes from the first S slots, stage 1 runs the bound's list from point 0, and the best key equals the unstaged key
(evaluated with a counts tensor) and the oracle's, on the paths where slots are dropped and on those where nothing
may be. Staging, the bound and S are forced, so small shapes take the path."""
import numpy as np
import pytest

import _oracle
from minicv_amd import synthetic as S
from _h_stage import (NO_CANDIDATE, NO_FAIL, ON, PRUNED, SAMPLER_FAILURE, THR, evaluate, oracle_key, pack, problem)

pytestmark = pytest.mark.gpu


def check_keys(src, dst, seed, begin, count, thr, slots, want_reason=None, oracle_count=True):
    """Staged with stage 0 on `slots` slots == unstaged with a counts tensor == oracle (oracle_count False: only the
    first failure is compared with the oracle). -> (staging stats, cell stats, oracle counts, unstaged counts)."""
    n = src.shape[0]
    pts = pack(src, dst)
    key_o, ref = oracle_key(src, dst, seed, begin, count, thr)
    key_s, st, cs, _ = evaluate(pts, n, seed, begin, count, thr, 1, ON, stage0=slots)
    key_u, st_u, _, full = evaluate(pts, n, seed, begin, count, thr, 1, ON, stage0=slots, counts=True)
    assert st_u[0] == 5                                   # a counts tensor: the call does not stage
    print(f"S {slots}: reason {st[0]}, B {st[1]}, boundaries {st[3:8]}, alive {st[10:14]}, unstaged key {key_u}")
    assert key_s == key_u
    assert key_s == key_o if oracle_count else key_s[1] == key_o[1]
    assert cs[0] == 1
    swept = slots if slots < count else count
    assert st[10] == swept                                # alive[0]: the slots stage 0 swept
    if swept < count:
        assert st[4] == 0                                 # stage 1 starts at point 0
    if want_reason is not None:
        assert st[0] == want_reason
    have = int((ref >= 0).sum())
    assert cs[2] == st[11] <= have
    if st[0] != PRUNED:
        assert cs[2] == have                              # pruning off: no slot with a model is dropped
    return st, cs, ref, full


@pytest.mark.parametrize("n,share,slots,begin,count", [(129, 0.5, 256, 0, 4096), (1000, 0.7, 256, 0, 4096),
                                                       (20000, 0.5, 256, 0, 4096), (20000, 0.5, 4096, 0, 4096),
                                                       (20000, 0.5, 256, 12345, 4099)])
def test_key_with_stage0_on_a_subset(gpu, n, share, slots, begin, count):
    src, dst = problem(n, 3, share)
    st, cs, ref, _ = check_keys(src, dst, 3, begin, count, THR, slots)
    if n == 20000:                                        # not vacuous
        assert st[0] == PRUNED and cs[2] < 0.5 * count and st[10 + st[2] - 1] >= 1


def test_ties_every_slot_that_reaches_n_survives(gpu):
    n = 1000
    src, dst = problem(n, 41, 0.0, 0.0)                   # exact correspondences: many hypotheses reach count N
    st, cs, ref, _ = check_keys(src, dst, 41, 0, 4096, THR, 256)
    full = int((ref == n).sum())
    assert ref.max() == n and full > 1
    assert st[10 + st[2] - 1] >= full                     # inclusive tests: every tie enters the last stage


def test_sampler_failure_outside_the_subset(gpu):
    x = np.linspace(-1, 1, 30)
    src = np.stack([x, 0.25 * x], axis=1)                 # the degenerate line set: samples fail the subset check
    dst = np.stack([x, -x], axis=1)
    key_o, ref = oracle_key(src, dst, 0, 0, 2048, 0.01)
    assert key_o[1] != NO_FAIL
    first = key_o[1]
    if first < 64:
        pytest.skip(f"the oracle's first sampler failure is hypothesis {first}: no room for a subset below it")
    slots = 64 if first >= 128 else 32
    while slots * 2 <= first and slots < 1024:
        slots *= 2
    assert slots <= first
    st, cs, ref, full = check_keys(src, dst, 0, 0, 2048, 0.01, slots, oracle_count=False)
    assert st[0] in (SAMPLER_FAILURE, NO_CANDIDATE)
    # every count is full: the staged counts are not readable, so compare the unstaged ones with the oracle and
    # the staged key's failure word with the oracle's (check_keys did)
    np.testing.assert_array_equal(full[ref >= 0], ref[ref >= 0])


def test_sampler_failure_beyond_the_subset_with_a_candidate(gpu):
    """5000 collinear points and four off the line: most hypotheses find a sample, the first that exhausts the
    sampler comes after slots with a model, outside a subset of 64."""
    rng = np.random.default_rng(2)
    x = np.linspace(-1, 1, 5000)
    src = np.concatenate([np.stack([x, 0.25 * x], axis=1), rng.uniform(-1, 1, (4, 2))])
    dst = np.concatenate([np.stack([x, -x], axis=1), rng.uniform(-1, 1, (4, 2))])
    key_o, ref = oracle_key(src, dst, 0, 0, 2048, 0.01)
    first = key_o[1]
    assert first != NO_FAIL and first >= 64 and (ref[:64] >= 0).any()
    st, cs, _, full = check_keys(src, dst, 0, 0, 2048, 0.01, 64, SAMPLER_FAILURE, oracle_count=False)
    np.testing.assert_array_equal(full[ref >= 0], ref[ref >= 0])


def test_no_model_in_the_subset(gpu):
    """Collinear points: no sample passes the subset check, so no slot of the subset has a model and there is no
    candidate; stage 1 runs every slot from point 0 to the end."""
    x = np.linspace(-1, 1, 40)
    src = np.stack([x, 0.25 * x], axis=1)
    dst = np.stack([x, -x], axis=1)
    key_o, ref = oracle_key(src, dst, 0, 0, 1024, 0.01)
    assert not (ref[:32] >= 0).any()
    st, cs, _, full = check_keys(src, dst, 0, 0, 1024, 0.01, 32, oracle_count=False)
    assert st[0] in (NO_CANDIDATE, SAMPLER_FAILURE)        # pruning off
    np.testing.assert_array_equal(full[ref >= 0], ref[ref >= 0])


def test_non_finite_points(gpu):
    src, dst, _ = S.homography_problem(300, 25, outlier_frac=0.3)
    rng = np.random.default_rng(25)
    src[:40] = src[40:80] * (1 + 1e-7 * rng.standard_normal((40, 2)))
    src[80:90, 1] = 0.5 * src[80:90, 0] + 0.1
    src[90:95] *= 1e6
    dst[95:100] *= 1e-6
    src[100, 0] = np.nan
    dst[101, 1] = np.inf
    src[102] = [1e30, -1e30]
    check_keys(src, dst, 25, 0, 4096, THR, 256)
    keep = np.ones(300, dtype=bool)
    keep[[100, 101]] = False
    check_keys(src[keep], dst[keep], 25, 0, 4096, THR, 256)
