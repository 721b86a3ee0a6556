"""The per-cell bound before stage 1 of the staged homography sweep, on the device: the kernels' cell table,
upper bounds and certified-cell bitmaps equal the host twin's (the same header), and the best key of a staged
evaluate is the same with the bound on, with it off and unstaged, on the paths where the bound drops slots and
on those where it must not. Staging and the bound are forced on (mcvTestHStaging / mcvTestHCellMode mode 1),
so small shapes take the path."""
import ctypes as C
import functools

import numpy as np
import pytest

import _h_cell as HC
import _oracle
from minicv_amd import native as N, opencv, synthetic as S

pytestmark = pytest.mark.gpu

THR = 5e-3
THR2 = float(np.float32(THR * THR))
NO_FAIL = 2**63 - 1
PRUNED, NO_CANDIDATE, SAMPLER_FAILURE, LATE = 0, 1, 2, 3
ON, OFF = 1, 2


@functools.lru_cache(maxsize=None)
def problem(n, seed, share=0.5, sigma=1e-3):
    src, dst, _ = S.homography_problem(n, seed, outlier_frac=share, sigma=sigma)
    return src, dst


@functools.lru_cache(maxsize=None)
def models_of(n, seed, count):
    src, dst = problem(n, seed)
    return HC.oracle_models(_oracle, _oracle.pack4(src, dst), seed, count)


def oracle_key(src, dst, seed, begin, count, thr):
    ref = _oracle.h_counts(_oracle.pack4(src, dst), seed, begin, count, float(np.float32(thr * thr)))
    fail = np.nonzero(ref == -2)[0]
    lim = fail[0] if len(fail) else count
    k0 = 0
    if (ref[:lim] >= 4).any():
        c = ref[:lim].max()
        i = int(np.nonzero(ref[:lim] == c)[0][0])
        k0 = (int(c) << 32) | (0xFFFFFFFF - (begin + i))
    return [k0, begin + int(fail[0]) if len(fail) else NO_FAIL], ref


def evaluate(pts, n, seed, begin, count, thr, staging, cell, plan=None, form=0):
    """One key-only mcvRansacEvaluate -> (key words, staging stats (16), cell stats (6), mfma stats (3))."""
    import torch
    from minicv_amd import device as D
    L = N.lib()
    own = plan is None
    if own:
        plan = D.RansacPlan(N.MODEL_HOMOGRAPHY, n, count)
    cfg = opencv.RansacParams(threshold=thr, seed=seed, fixed_iters=True, max_iters=max(count, 1)).to_c()
    key = torch.zeros(2, dtype=torch.int64, device=pts.device)
    ps, pc, pf = L.mcvTestHStaging(staging, None), L.mcvTestHCellMode(cell, 0, 0, None), L.mcvTestHMfma(form, None)
    try:
        plan.evaluate(pts, n, cfg, begin, count, key, None)
        torch.cuda.synchronize()
        st, cs, ms = (C.c_longlong * 16)(), (C.c_longlong * 6)(), (C.c_longlong * 3)()
        L.mcvTestHStaging(-1, C.addressof(st))
        L.mcvTestHCellMode(-1, 0, 0, C.addressof(cs))
        L.mcvTestHMfma(-1, C.addressof(ms))
    finally:
        L.mcvTestHStaging(ps, None)
        L.mcvTestHCellMode(pc, 0, 0, None)
        L.mcvTestHMfma(pf, None)
        if own:
            plan.close()
    return [int(v) for v in key.cpu().numpy()], [int(v) for v in st], [int(v) for v in cs], [int(v) for v in ms]


def pack(src, dst):
    import torch
    from minicv_amd import device as D
    return D.pack_points_tensor(src, dst, torch.device("cuda:0"))


def check_keys(src, dst, seed, begin, count, thr, want_reason=None, oracle_count=True):
    """Bound on == bound off == unstaged == oracle (oracle_count = False: only the first failure is compared
    with the oracle, as tests/test_gpu_h_staged.py does for chunks with a sampler failure).
    -> (staging stats, cell stats, oracle counts) of the run with the bound on."""
    n = src.shape[0]
    pts = pack(src, dst)
    key_o, ref = oracle_key(src, dst, seed, begin, count, thr)
    key_on, st, cs, _ = evaluate(pts, n, seed, begin, count, thr, 1, ON)
    key_off, st_off, cs_off, _ = evaluate(pts, n, seed, begin, count, thr, 1, OFF)
    key_un, st_un, _, _ = evaluate(pts, n, seed, begin, count, thr, 2, ON)
    assert st_un[0] == 4 and cs_off[0] == 0 and st_off[11] == count    # forced off; no bound: every slot enters stage 1
    assert cs[0] == 1 and cs[3] == HC.cells()
    assert key_on == key_off == key_un
    assert key_on == key_o if oracle_count else key_on[1] == key_o[1]
    if want_reason is not None:
        assert st[0] == want_reason
    have = int((ref >= 0).sum())
    assert cs[2] == st[11] <= have
    if st[0] != PRUNED:
        assert cs[2] == have                       # pruning off on the device: no slot with a model is dropped
    return st, cs, ref


@pytest.mark.parametrize("hyps", [2**12, 2**14])
@pytest.mark.parametrize("n", [4097, 8192, 20001])
def test_device_table_equals_host_twin(gpu, n, hyps):
    src, dst = problem(n, 3)
    pts4 = _oracle.pack4(src, dst)
    models = models_of(n, 3, hyps)
    cnt = _oracle.h_counts(pts4, 3, 0, hyps, THR2)
    cnt = cnt[cnt >= 0]
    best, B = models[int(np.argmax(cnt))], int(cnt.max())
    rng = np.random.default_rng(n)
    crafted = np.array([[1, 0, 0, 0, 1, 0, -4, 0], [1, 0, 0, 0, 1, 0, 0, 0], [0] * 8, [np.nan] + [0] * 7,
                        [1e30, 0, 0, 0, 1, 0, 0, 0]], np.float32)
    near = (best[None, :] * (1 + np.exp(rng.uniform(np.log(1e-6), np.log(1e-1), (59, 1))) *
                             rng.standard_normal((59, 8)))).astype(np.float32)
    models = np.concatenate([models, crafted, near])
    host = HC.run(N.lib(), pts4, best, models, THR2, B, device=0)
    dev = HC.run(N.lib(), pts4, best, models, THR2, B, device=1)
    np.testing.assert_array_equal(dev["cell"], host["cell"])
    np.testing.assert_array_equal(dev["sizes"], host["sizes"])
    np.testing.assert_array_equal(dev["boxes"].view(np.int32), host["boxes"].view(np.int32))
    np.testing.assert_array_equal(dev["ub"], host["ub"])
    np.testing.assert_array_equal(dev["bits"], host["bits"])
    assert dev["alive"] == host["alive"]
    assert 0 < host["alive"] < len(models) // 2        # not vacuous at 50 % outliers


@pytest.mark.parametrize("hyps", [2**12, 2**14])
@pytest.mark.parametrize("n", [4097, 8192, 20001])
def test_key_with_bound_equals_key_without(gpu, n, hyps):
    src, dst = problem(n, 3)
    st, cs, ref = check_keys(src, dst, 3, 0, hyps, THR, PRUNED)
    print(f"n {n} hyps {hyps}: non-empty cells {cs[1]}, alive after the bound {cs[2]}, entering stages {st[10:14]}")
    assert 1 <= cs[2] < hyps // 2                      # the bound drops most junk at 50 % outliers
    assert st[12] <= st[11]


@pytest.mark.parametrize("share", [0.2, 0.5, 0.8])
def test_outlier_shares(gpu, share):
    src, dst = problem(4097, 17, share)
    check_keys(src, dst, 17, 100, 4096, THR)


@pytest.mark.parametrize("n", [500, 4097])
def test_ties_keep_the_lowest_index(gpu, n):
    src, dst = problem(n, 41, 0.0, 0.0)      # exact correspondences: many hypotheses reach count N
    src, dst = src.copy(), dst.copy()
    src[n // 2:] = src[:n - n // 2]           # duplicate correspondences
    dst[n // 2:] = dst[:n - n // 2]
    st, cs, ref = check_keys(src, dst, 41, 0, 1024, THR)
    full = int((ref == ref.max()).sum())
    assert full > 1 and cs[2] >= full         # every slot that ties survives the bound


def test_sampler_failure_and_no_candidate_drop_nothing(gpu):
    x = np.linspace(-1, 1, 30)
    src = np.stack([x, 0.25 * x], axis=1)    # collinear: no sample passes the subset check
    dst = np.stack([x, -x], axis=1)
    st, cs, ref = check_keys(src, dst, 0, 0, 2048, 0.01, oracle_count=False)
    assert st[0] in (NO_CANDIDATE, SAMPLER_FAILURE)
    # 5000 collinear points and four off the line: most hypotheses find a sample, two exhaust the sampler's
    # 10000 attempts, the first of them (147) after hypotheses with a model: a candidate and a failure
    rng = np.random.default_rng(2)
    x = np.linspace(-1, 1, 5000)
    src2 = np.concatenate([np.stack([x, 0.25 * x], axis=1), rng.uniform(-1, 1, (4, 2))])
    dst2 = np.concatenate([np.stack([x, -x], axis=1), rng.uniform(-1, 1, (4, 2))])
    st2, _, ref2 = check_keys(src2, dst2, 0, 0, 2048, 0.01, SAMPLER_FAILURE, oracle_count=False)
    first = int(np.nonzero(ref2 == -2)[0][0])
    assert first > 0 and (ref2[:first] >= 0).any()


def test_late_first_boundary_drops_nothing(gpu):
    src, dst = problem(5000, 8, 0.9, 2e-3)
    check_keys(src, dst, 8, 0, 4096, 1e-2, LATE)


def test_redo_slots_of_stage_0_stay_out_of_the_list(gpu):
    """Coordinates of 2e7 among unit ones: 360 of the 4096 hypotheses leave the certificate's domain (G > 2^50),
    stage 0 marks their waves for the exact recount (matrix-core form: it counts those waves), the bound keeps
    them out of its list and the key is unchanged."""
    src, dst = problem(4300, 25, 0.3)
    src, dst = src.copy(), dst.copy()
    src[90:95] *= 2e7
    dst[95:100] *= 2e7
    n = src.shape[0]
    pts = pack(src, dst)
    key_o, ref = oracle_key(src, dst, 25, 0, 4096, THR)
    key_on, st, cs, ms = evaluate(pts, n, 25, 0, 4096, THR, 1, ON, form=2)
    key_off, _, _, _ = evaluate(pts, n, 25, 0, 4096, THR, 1, OFF, form=2)
    print("reason", st[0], "waves outside the domain", ms[2], "alive after the bound", cs[2])
    assert ms[2] >= 1
    assert key_on == key_off == key_o


def test_one_plan_many_point_sets(gpu):
    """The cell table is rebuilt per call: evaluates on one plan with different point sets give each set's key."""
    from minicv_amd import device as D
    plan = D.RansacPlan(N.MODEL_HOMOGRAPHY, 8192, 4096)
    try:
        cells = []
        for n, seed, share in ((8192, 3, 0.5), (4097, 17, 0.2), (8192, 3, 0.5), (5000, 5, 0.8), (4097, 17, 0.2)):
            src, dst = problem(n, seed, share)
            key_o, _ = oracle_key(src, dst, seed, 0, 4096, THR)
            key, st, cs, _ = evaluate(pack(src, dst), n, seed, 0, 4096, THR, 1, ON, plan=plan)
            assert key == key_o and cs[0] == 1
            cells.append((cs[1], cs[2]))
        assert cells[0] == cells[2] and cells[1] == cells[4]    # the same figures for the same points
    finally:
        plan.close()
