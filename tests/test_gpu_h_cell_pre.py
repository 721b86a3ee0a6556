"""The box test's fp32 prefilter (minicv_amd/csrc/h_cell_pre.h) in the device kernels of the per-cell bound: both
passes give the same arrays with the prefilter on, with it off and on the host twin, the device's three-way verdicts
are the host twin's, and a staged evaluate returns the same key and the same slot counts either way."""
import numpy as np
import pytest

import _h_cell as HC
import _h_cell_pre as HP
import _h_cell_rel as HR
import _oracle
from minicv_amd import native as N
from _h_stage import ON, PRUNED, THR, THR2, evaluate, models_of, oracle_key, pack, problem

pytestmark = pytest.mark.gpu


def inputs(n):
    """2048 models: the oracle's hypotheses of the problem, out-of-domain ones, and near-copies of the best."""
    hyps = 2048
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
    near = (best[None, :] * (1 + np.exp(rng.uniform(np.log(1e-6), np.log(1e-1), (2048, 1))) *
                             rng.standard_normal((2048, 8)))).astype(np.float32)
    models = np.concatenate([crafted, near[:56], best[None, :], models, near[56:]])[:2048]
    return pts4, models, best, B


@pytest.mark.parametrize("n", [4096, 20000])
def test_both_passes_equal_with_and_without_the_prefilter(gpu, n):
    L = N.lib()
    pts4, models, best, B = inputs(n)
    bounds = HR.boundaries(n)
    with HP.mode(L, 1):
        twin_b = HC.run(L, pts4, best, models, THR2, B, device=0)
        twin_r = HR.run(L, pts4, best, models, THR2, B, bounds, device=0)
        off_b = HC.run(L, pts4, best, models, THR2, B, device=1)
        dec, und = HP.stats(L)
        assert dec == 0 and und > 0
        off_r = HR.run(L, pts4, best, models, THR2, B, bounds, device=1)
    with HP.mode(L, 0):
        on_b = HC.run(L, pts4, best, models, THR2, B, device=1)
        dec_b, und_b = HP.stats(L)
        on_r = HR.run(L, pts4, best, models, THR2, B, bounds, device=1)
        dec_r, und_r = HP.stats(L)
        host_b = HC.run(L, pts4, best, models, THR2, B, device=0)
        dec_h, und_h = HP.stats(L)
    full = int((twin_b["sizes"] > 0).sum())
    assert dec_b + und_b == dec_r + und_r == dec_h + und_h == 2048 * full   # 2048 lanes: no idle ones
    assert und_b == und_r == und_h <= 0.01 * 2048 * full
    print(f"n {n}: {2048 * full} tests, undecided {und_b}")
    for out in (off_b, on_b, host_b):
        for k in ("cell", "sizes", "ub", "bits"):
            np.testing.assert_array_equal(out[k], twin_b[k])
        assert out["alive"] == twin_b["alive"]
    for out in (off_r, on_r):
        for k in ("cell", "ub", "bits", "left"):
            np.testing.assert_array_equal(out[k], twin_r[k])
        assert out["alive"] == twin_r["alive"]
    assert 0 < twin_r["alive"] < twin_b["alive"] < 2048


@pytest.mark.parametrize("n", [4096, 20000])
def test_device_verdicts_equal_the_host_twins(gpu, n):
    L = N.lib()
    pts4, models, best, B = inputs(n)
    host = HP.verdicts(L, pts4, best, models, THR2, device=0)
    dev = HP.verdicts(L, pts4, best, models, THR2, device=1)
    for k in ("cell", "sizes", "verdict"):
        np.testing.assert_array_equal(dev[k], host[k])
    np.testing.assert_array_equal(dev["boxes"].view(np.int32), host["boxes"].view(np.int32))
    with HP.mode(L, 1):
        twin = HC.run(L, pts4, best, models, THR2, B, device=0)
    HP.check_sound(dev, twin)
    assert set(np.unique(dev["verdict"])) == {HP.NOT, HP.CERT, HP.UNDECIDED}


def test_staged_key_and_slot_counts_with_and_without_the_prefilter(gpu):
    L = N.lib()
    n, hyps = 20001, 2**12
    src, dst = problem(n, 3)
    pts = pack(src, dst)
    key_o, _ = oracle_key(src, dst, 3, 0, hyps, THR)
    from minicv_amd import device as D
    plan = D.RansacPlan(N.MODEL_HOMOGRAPHY, n, hyps)       # the counters live in the plan: read them before it closes
    try:
        with HP.mode(L, 0):
            key_on, st_on, cs_on, _ = evaluate(pts, n, 3, 0, hyps, THR, 1, ON, plan=plan)
            dec, und = HP.stats(L)
        with HP.mode(L, 1):
            key_off, st_off, cs_off, _ = evaluate(pts, n, 3, 0, hyps, THR, 1, ON, plan=plan)
            dec0, und0 = HP.stats(L)
    finally:
        plan.close()
    assert key_on == key_off == key_o
    assert st_on == st_off and cs_on == cs_off and st_on[0] == PRUNED
    assert dec0 == 0 and und0 == dec + und and 0 <= und <= 0.01 * (dec + und) and dec > 0
