"""The certified fp32 prefilter of the per-cell bound's box test (minicv_amd/csrc/h_cell_pre.h) through its host
twin: a decided verdict is always the fp64 test's (mcvTestHCellBound, device = 0, prefilter off), on oracle
hypotheses, at the floats around the threshold, and outside the domain; and it decides nearly everything. CPU
only; the device kernels are compared with this twin in test_gpu_h_cell_pre.py."""
import numpy as np
import pytest

import _h_cell as HC
import _h_cell_pre as HP
from minicv_amd import synthetic as S

THR = 5e-3
THR2 = float(np.float32(THR * THR))


@pytest.fixture(scope="module")
def case(native, oracle):
    """homography_problem(4096, 11), the models of hypotheses 0..1023 and the one with the best oracle count."""
    src, dst, _ = S.homography_problem(4096, 11)
    pts4 = oracle.pack4(src, dst)
    models = HC.oracle_models(oracle, pts4, 11, 1024)
    cnt = oracle.h_counts(pts4, 11, 0, 1024, THR2)
    cnt = cnt[cnt >= 0]
    assert len(cnt) == len(models)
    k = int(np.argmax(cnt))
    return pts4, models, models[k], int(cnt[k])


def fp64_twin(L, pts4, cand, models, B, G=4, Gs=12, thr2=THR2):
    with HP.mode(L, 1):
        out = HC.run(L, pts4, cand, models, thr2, B, G, Gs)
        dec, und = HP.stats(L)
    assert dec == 0 and und > 0            # the prefilter is off: everything went to fp64
    return out


def with_prefilter(L, pts4, cand, models, B, G=4, Gs=12, thr2=THR2):
    with HP.mode(L, 0):
        out = HC.run(L, pts4, cand, models, thr2, B, G, Gs)
        st = HP.stats(L)
    return out, st


def same(a, b):
    for k in ("cell", "sizes", "ub", "bits"):
        np.testing.assert_array_equal(a[k], b[k])
    assert a["alive"] == b["alive"]


@pytest.mark.parametrize("G,Gs", [(4, 12), (6, 24), (1, 1)])
def test_soundness_and_no_giving_up(native, case, G, Gs):
    L = native.lib()
    pts4, models, best, B = case
    twin = fp64_twin(L, pts4, best, models, B, G, Gs)
    v = HP.verdicts(L, pts4, best, models, THR2, G, Gs)
    full = HP.check_sound(v, twin)
    pre, (dec, und) = with_prefilter(L, pts4, best, models, B, G, Gs)
    same(pre, twin)
    tests = len(models) * int(full.sum())
    assert dec + und == tests
    assert und == int((v["verdict"][:, full] == HP.UNDECIDED).sum())
    ver = v["verdict"][:, full]
    print(f"grid ({G}, {Gs}): {tests} tests, certified {(ver == 1).mean():.4f}, not {(ver == 0).mean():.4f}, "
          f"undecided {und} ({und / tests:.2e})")
    if (G, Gs) == (4, 12):
        assert und <= 0.01 * tests         # a prefilter that hands everything to fp64 fails here
        assert (ver == HP.CERT).any() and (ver == HP.NOT).any()


def f2i(f):
    """Monotone float32 -> int64 (the ordered-integer encoding)."""
    i = np.asarray(f, np.float32).view(np.int32).astype(np.int64)
    return np.where(i >= 0, i, -(i & 0x7fffffff))


def i2f(i):
    i = np.asarray(i, np.int64)
    return np.where(i >= 0, i, (-i) | 0x80000000).astype(np.uint32).view(np.float32)


def test_floats_around_the_threshold(native, case):
    """64 (model, cell, side) triples: h2 (right / left side) or h5 (above / below) moves until the fp64 test flips
    to certified, bisected to the neighbouring floats where that side's form crosses beta; then the 9 consecutive
    floats around the crossing, and steps of 2^8 and 2^14 ulps beside them."""
    L = native.lib()
    pts4, models, best, B = case
    twin = fp64_twin(L, pts4, best, models, B)
    v = HP.verdicts(L, pts4, best, models, THR2)
    open_ = (v["verdict"] == HP.NOT) & ~twin["cert"] & (twin["sizes"] > 0)[None, :]
    rng = np.random.default_rng(64)
    ks, cs = np.nonzero(open_)
    pick = rng.permutation(len(ks))[:160]
    trip = [(int(ks[p]), int(cs[p]), j % 4) for j, p in enumerate(pick)]   # side: h2 up, h2 down, h5 up, h5 down
    coef = np.array([2 if t[2] < 2 else 5 for t in trip])
    sign = np.array([1.0 if t[2] % 2 == 0 else -1.0 for t in trip])
    base = models[[t[0] for t in trip]].copy()
    cell = np.array([t[1] for t in trip])
    rows = np.arange(len(trip))

    def certified(vals):
        m = base.copy()
        m[rows, coef] = vals
        return fp64_twin(L, pts4, best, m, B)["cert"][rows, cell]

    start = base[rows, coef]
    far = (start + sign * 8.0).astype(np.float32)
    ok = ~certified(start) & certified(far)
    assert ok.sum() >= 64
    keep = np.nonzero(ok)[0][:64]
    base, cell, coef, rows = base[keep], cell[keep], coef[keep], np.arange(64)
    lo, hi = f2i(start[keep]), f2i(far[keep])          # not certified at lo, certified at hi
    up = hi > lo
    for _ in range(34):
        mid = (lo + hi) // 2
        c = certified(i2f(mid))
        hi = np.where(c, mid, hi)
        lo = np.where(c, lo, mid)
    assert (np.abs(hi - lo) == 1).all()
    seen = set()
    steps = list(range(-5, 4)) + [-2**14, -2**8, 2**8, 2**14]   # lo and hi are steps -1 and 0
    for st in steps:
        m = base.copy()
        m[rows, coef] = i2f(hi + np.where(up, st, -st))
        tw = fp64_twin(L, pts4, best, m, B)
        vv = HP.verdicts(L, pts4, best, m, THR2)
        HP.check_sound(vv, tw)
        pre, _ = with_prefilter(L, pts4, best, m, B)
        same(pre, tw)
        if st in (-1, 0):
            np.testing.assert_array_equal(tw["cert"][rows, cell], st == 0)
        seen |= set(vv["verdict"][rows, cell].tolist())
    assert seen == {HP.NOT, HP.CERT, HP.UNDECIDED}     # both sides of the band and the band itself were visited


def domain_sets(oracle):
    """Point sets at and beyond the bound's domain: a NaN, an infinite and a 1e30 coordinate, the set of the staged
    sweep's out-of-domain test, and its finite part (huge coordinates, finite extents)."""
    src, dst, _ = S.homography_problem(300, 25, outlier_frac=0.3)
    rng = np.random.default_rng(25)
    src[:40] = src[40:80] * (1 + 1e-7 * rng.standard_normal((40, 2)))
    src[80:90, 1] = 0.5 * src[80:90, 0] + 0.1
    src[90:95] *= 1e6
    dst[95:100] *= 1e-6
    fin = (src.copy(), dst.copy())
    src[100, 0] = np.nan
    dst[101, 1] = np.inf
    src[102] = [1e30, -1e30]
    out = {"staged_test": oracle.pack4(src, dst), "finite_huge": oracle.pack4(*fin)}
    for name, (row, col, val) in {"nan": (7, 0, np.nan), "inf": (8, 3, np.inf), "1e30": (9, 1, 1e30)}.items():
        s2, d2, _ = S.homography_problem(500, 14, outlier_frac=0.5)
        p = oracle.pack4(s2, d2)
        p[row, col] = val
        out[name] = p
    return out


@pytest.mark.parametrize("name", ["staged_test", "finite_huge", "nan", "inf", "1e30"])
def test_out_of_domain_never_certifies(native, oracle, name):
    L = native.lib()
    pts4 = domain_sets(oracle)[name]
    rng = np.random.default_rng(3)
    models = np.concatenate([HP.crafted_models(rng, S.H_TRUE), HC.oracle_models(oracle, pts4, 25, 200).reshape(-1, 8)])
    cand = (S.H_TRUE / S.H_TRUE[2, 2]).ravel()[:8].astype(np.float32)
    twin = fp64_twin(L, pts4, cand, models, 3)
    v = HP.verdicts(L, pts4, cand, models, THR2)
    HP.check_sound(v, twin)
    pre, _ = with_prefilter(L, pts4, cand, models, 3)
    same(pre, twin)
    if name in ("staged_test", "nan", "inf"):
        assert not (v["verdict"] == HP.CERT).any() and not twin["cert"].any()


def test_sign_change_of_w_and_empty_cells(native, case):
    L = native.lib()
    pts4, models, best, B = case
    m = np.concatenate([HP.crafted_models(np.random.default_rng(7), S.H_TRUE),
                        np.array([[1, 0, 0, 0, 1, 0, -4, 0]], np.float32)])
    twin = fp64_twin(L, pts4, best, m, B)
    v = HP.verdicts(L, pts4, best, m, THR2)
    full = HP.check_sound(v, twin)
    assert (~full).any()                                   # the 4-D grid has empty cells
    b = twin["boxes"]
    crossing = full & (b[:, 0] <= 0.25) & (b[:, 1] >= 0.25)   # w = 1 - 4 x changes sign inside these cells
    assert crossing.any() and not (v["verdict"][-1, crossing] == HP.CERT).any()
    assert (v["verdict"][-1, crossing] == HP.NOT).any()       # and the prefilter itself says so
    pre, _ = with_prefilter(L, pts4, best, m, B)
    same(pre, twin)
