"""The certified homography sweep's bf16 matrix-core form (mcv_h_verify_mfma).

Counts equal the oracle's op-by-op counts and the VALU form's (mcvTestHomographySweep modes 5 / 4) over
the tile edges (32 points, 32 hypotheses per wave), crafted models and point sets; the undecided-row and
event-overflow paths are reached on purpose (points on a model's threshold circle); the W, U, V the form
computes lie within the bound its certificate uses; the staged sweep under the forced
matrix-core form returns the unstaged key.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from minicv_amd import native as N
from minicv_amd import opencv, synthetic as S

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
# the certificate's constant for one matrix-core dot, in u * sum |terms| (kMfmaDotC, h_cert.h), and its
# absolute term for pieces and sums the matrix core may flush below 2^-126
DOT_C = 8.5
THR2 = float(np.float32(5e-3 ** 2))
VALU, MFMA = 4, 5


def sweep(pts, models, thr2, mode):
    pts = np.ascontiguousarray(pts, np.float32)
    models = np.ascontiguousarray(models, np.float32)
    counts = np.zeros(len(models), np.int32)
    ok = N.lib().mcvTestHomographySweep(pts.ctypes.data, pts.shape[0], models.ctypes.data, len(models), float(thr2),
                                        mode, counts.ctypes.data)
    assert ok == 1, N.last_error()
    return counts


def stats3():
    """(undecided rows logged, waves overflowed, waves outside the bound's domain) of the last sweep."""
    st = (C.c_longlong * 3)()
    N.lib().mcvTestHMfma(-1, C.addressof(st))
    return int(st[0]), int(st[1]), int(st[2])


def stats():
    return stats3()[:2]


def oracle_counts(oracle, pts, models, thr2):
    pts = np.ascontiguousarray(pts, np.float32)
    return np.array([oracle.h_count(pts, np.ascontiguousarray(m, np.float32), float(thr2)) for m in models], np.int32)


def sampled_models(oracle, pts, seed, count):
    """The oracle's fp32 models of the first `count` hypotheses with a model."""
    ms = []
    hyp = 0
    while len(ms) < count and hyp < 8 * count + 64:
        st, _, hf, _ = oracle.h_hypothesis(np.ascontiguousarray(pts, np.float32), seed, hyp)
        if st == 1:
            ms.append(np.asarray(hf, np.float32)[:8])
        hyp += 1
    return ms


def problem(n, seed, scale=1.0):
    src, dst, _ = S.homography_problem(max(n, 8), seed, outlier_frac=0.4)
    return (np.c_[src, dst][:n] * scale).astype(np.float32)


def out_of_domain_models():
    """One out-of-domain row sends its whole wave of 32 to the exact recount: these get a wave of their own."""
    return [np.array([1, 0, 0, 0, 1, 0, 3e37, 3e37], np.float32),        # outside the bound's domain
            np.array([2.0 ** 110, 0, 0, 0, 1, 0, 0, 0], np.float32)]     # a coefficient above 2^100


def crafted_models(rng):
    """In-domain models with extreme coefficients: they must go through the matrix-core certificate."""
    ms = [np.array([1.02, -0.09, -0.16, 0.08, 1.04, -0.07, 0.40, 0.13], np.float32)]
    ms.append(np.array([2.0 ** 40, -2.0 ** 38, 2.0 ** 39, 2.0 ** 37, 2.0 ** 40, 1.0, 0.25, -0.5], np.float32))
    ms.append(np.array([1e-39, 2e-40, -1e-41, 3e-42, 1e-39, 1e-45, 1e-40, -1e-44], np.float32))   # denormal
    ms.append(np.array([1.0, 1e-42, 0.0, -1e-43, 1.0, 0.0, 2.0 ** -140, 0.0], np.float32))
    ms.append(np.zeros(8, np.float32))                                   # the zero model of a failed slot
    ms.append(np.array([1, 0, 0, 0, 1, 0, -1, 0], np.float32))           # w = 0 at x = 1
    for _ in range(8):
        ms.append((rng.normal(size=8) * rng.choice([1e-3, 1, 10], size=8)).astype(np.float32))
    return ms


@pytest.fixture(scope="module")
def reference(gpu, oracle):
    """One point set of 4099 correspondences and 100 models, the oracle's counts of every prefix length
    shared by the shape cases below. Models 0..31 (the first wave): the crafted in-domain ones and sampled
    ones; 32, 33: the out-of-domain ones; the rest sampled."""
    rng = np.random.default_rng(7)
    pts = problem(4099, 11)
    pts[[7, 50, 3000], 0] = 1.0   # w = 0 for the crafted model with h6 = -1
    sampled = sampled_models(oracle, pts, 11, 100)
    crafted = crafted_models(rng)
    models = crafted + sampled[:32 - len(crafted)] + out_of_domain_models() + sampled[32 - len(crafted):]
    models = np.stack(models[:100])
    ref = {n: oracle_counts(oracle, pts[:n], models, THR2) for n in (1, 31, 32, 33, 95, 4099)}
    return pts, models, ref


@pytest.mark.parametrize("n", [1, 31, 32, 33, 95, 4099])
def test_counts_equal_oracle_over_tile_edges(reference, n):
    pts, models, ref = reference
    for h in (1, 31, 32, 33, 100):
        got = sweep(pts[:n], models[:h], THR2, MFMA)
        np.testing.assert_array_equal(got, ref[n][:h], err_msg=f"N={n} hyps={h}")
        np.testing.assert_array_equal(sweep(pts[:n], models[:h], THR2, VALU), ref[n][:h])


@pytest.mark.parametrize("n", [95, 4099])
def test_extreme_coefficients_take_the_matrix_core_certificate(reference, n):
    """The wave of the crafted models (coefficients up to 2^40 and down to denormal, the zero model, w = 0 on
    the point set) is neither out of domain nor overflowed, so its counts are the certificate's and the
    logged rows' recount; the out-of-domain pair in a wave of its own takes the exact recount."""
    pts, models, ref = reference
    got = sweep(pts[:n], models[:32], THR2, MFMA)
    und, ovf, ood = stats3()
    print("crafted wave: undecided rows", und, "overflowed", ovf, "out of domain", ood)
    assert ovf == 0 and ood == 0
    np.testing.assert_array_equal(got, ref[n][:32])
    got = sweep(pts[:n], models[32:34], THR2, MFMA)
    assert stats3()[2] == 1
    np.testing.assert_array_equal(got, ref[n][32:34])


def test_failed_slot_is_left_untouched(gpu, oracle):
    """A negative count (no model, no sample) marks a slot the sweep must not write: run through the plan,
    whose generate writes the statuses (a degenerate point set: every sample is collinear)."""
    import torch
    from minicv_amd import device as D
    dev = torch.device("cuda:0")
    x = np.linspace(-1, 1, 64)
    src = np.stack([x, 0.25 * x], axis=1)
    dst = np.stack([x, -x], axis=1)
    ref = oracle.h_counts(oracle.pack4(src, dst), 0, 0, 256, float(np.float32(1e-4)))
    assert (ref < 0).any()
    pts = D.pack_points_tensor(src, dst, dev)
    plan = D.RansacPlan(N.MODEL_HOMOGRAPHY, 64, 256)
    cfg = opencv.RansacParams(threshold=0.01, seed=0, fixed_iters=True, max_iters=256).to_c()
    key = torch.zeros(2, dtype=torch.int64, device=dev)
    counts = torch.zeros(256, dtype=torch.int32, device=dev)
    prev = N.lib().mcvTestHMfma(2, None)
    try:
        plan.evaluate(pts, 64, cfg, 0, 256, key, counts)
        torch.cuda.synchronize()
    finally:
        N.lib().mcvTestHMfma(prev, None)
        plan.close()
    np.testing.assert_array_equal(counts.cpu().numpy(), ref)


POINT_SETS = ["unit", "pixel", "tiny", "nan", "equal"]


@pytest.mark.parametrize("kind", POINT_SETS)
def test_point_sets(gpu, oracle, kind):
    n = 777
    scale = {"pixel": 4000.0, "tiny": 1e-6}.get(kind, 1.0)
    pts = problem(n, 21, scale)
    thr2 = float(np.float32(THR2 * scale * scale))
    if kind == "nan":
        pts[5, 0] = np.nan
    if kind == "equal":
        pts[:] = pts[3]
    rng = np.random.default_rng(3)
    models = sampled_models(oracle, problem(n, 21, scale), 21, 40)
    base = np.array([1.02, -0.09, -0.16 * scale, 0.08, 1.04, -0.07 * scale, 0.40 / scale, 0.13 / scale], np.float32)
    models += [base] + [(base * (1 + 1e-3 * rng.normal(size=8))).astype(np.float32) for _ in range(23)]
    models = np.stack(models)
    ref = oracle_counts(oracle, pts, models, thr2)
    assert kind in ("nan", "equal") or ref.max() > n // 3   # the cases are not vacuous
    np.testing.assert_array_equal(sweep(pts, models, thr2, MFMA), ref)
    np.testing.assert_array_equal(sweep(pts, models, thr2, VALU), ref)


def threshold_points(n, rng, h, thr, ulps=3):
    """Correspondences whose error against model h sits within a few ulps of thr^2: x' = proj(x) + thr e."""
    src = rng.uniform(-1, 1, size=(n, 2))
    w = h[6] * src[:, 0] + h[7] * src[:, 1] + 1.0
    px = (h[0] * src[:, 0] + h[1] * src[:, 1] + h[2]) / w
    py = (h[3] * src[:, 0] + h[4] * src[:, 1] + h[5]) / w
    ang = rng.uniform(0, 2 * np.pi, size=n)
    r = thr * (1.0 + ulps * 2.0 ** -23 * rng.integers(-2, 3, size=n))
    return np.c_[src, px + r * np.cos(ang), py + r * np.sin(ang)].astype(np.float32)


def test_undecided_rows_are_logged_and_recounted(gpu, oracle):
    rng = np.random.default_rng(5)
    h = np.array([1.02, -0.09, -0.16, 0.08, 1.04, -0.07, 0.40, 0.13], np.float64)
    pts = problem(333, 31)
    pts[40:72] = threshold_points(32, rng, h, 5e-3)
    models = np.stack([h.astype(np.float32)] + sampled_models(oracle, pts, 31, 40))
    ref = oracle_counts(oracle, pts, models, THR2)
    got = sweep(pts, models, THR2, MFMA)
    und, ovf = stats()
    print("undecided rows", und, "overflowed waves", ovf)
    assert und >= 1 and ovf == 0
    np.testing.assert_array_equal(got, ref)
    # the decided neighbours of the cut: both sides occur among the threshold points
    inl = oracle.h_count(pts[40:72].copy(), models[0], THR2)
    assert 0 < inl < 32


def test_event_overflow_takes_the_exact_recount(gpu, oracle):
    """More undecided rows in one wave than its event list holds (1024): every tile of 32 threshold points
    logs a row for the model on the circle and for its near copies."""
    rng = np.random.default_rng(6)
    h = np.array([1.02, -0.09, -0.16, 0.08, 1.04, -0.07, 0.40, 0.13], np.float64)
    n = 32 * 48
    pts = threshold_points(n, rng, h, 5e-3)
    models = np.stack([(h * (1 + 1e-9 * k)).astype(np.float32) for k in range(32)] +
                      sampled_models(oracle, problem(200, 32), 32, 8))
    ref = oracle_counts(oracle, pts, models, THR2)
    got = sweep(pts, models, THR2, MFMA)
    und, ovf = stats()
    print("undecided rows", und, "overflowed waves", ovf)
    assert ovf >= 1 and und > 1024
    np.testing.assert_array_equal(got, ref)


def bf16_split(v):
    """The kernel's split: three bf16 pieces, each rounded to nearest even, as float64 values."""
    v = np.asarray(v, np.float32)
    out = []
    r = v.copy()
    for _ in range(3):
        b = r.view(np.uint32).astype(np.uint64)
        p = (((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)
        out.append(p.astype(np.float64))
        r = (r - p).astype(np.float32)
    return out


def operand_sets():
    rng = np.random.default_rng(9)
    sets = {}
    m = rng.normal(size=(64, 8)).astype(np.float32)
    p = rng.uniform(-1, 1, size=(257, 4)).astype(np.float32)
    sets["random"] = (m, p)
    sets["mixed exponents"] = ((m * np.exp2(rng.integers(-30, 30, size=m.shape))).astype(np.float32),
                               (p * np.exp2(rng.integers(-20, 20, size=p.shape))).astype(np.float32))
    mc = m.copy()
    pc = p.copy()
    mc[:, 2] = -(mc[:, 0] * pc[0, 0] + mc[:, 1] * pc[0, 1])   # U cancels at point 0, nearly at its copies
    mc[:, 5] = -(mc[:, 3] * pc[0, 0] + mc[:, 4] * pc[0, 1])
    pc[1:64] = pc[0] * (1 + 2.0 ** -20 * rng.integers(-8, 9, size=(63, 4)))
    sets["cancellation"] = (mc, pc.astype(np.float32))
    md = m.copy()
    md[:, 0] *= 2.0 ** 30
    md[:, 4] *= 2.0 ** 30
    md[:, 6] *= 2.0 ** 20
    sets["one dominant term"] = (md, p)
    sets["denormal pieces"] = ((m * 2.0 ** -120).astype(np.float32), (p * 2.0 ** -10).astype(np.float32))
    return sets


@pytest.mark.parametrize("name", list(operand_sets()))
def test_mfma_dot_within_the_certificate_bound(gpu, name):
    """|W, U, V of the matrix-core form - the exact value| <= DOT_C u sum |h| |x| + the flush term: the
    arithmetic assumption of the certificate (split: 2.01 u; accumulation: the rest)."""
    m, p = operand_sets()[name]
    out = np.zeros((len(m), len(p), 3), np.float32)
    ok = N.lib().mcvTestHMfmaWuv(p.ctypes.data, len(p), m.ctypes.data, len(m), out.ctypes.data)
    assert ok == 1, N.last_error()
    md, x, y = m.astype(np.float64), p[:, 0].astype(np.float64), p[:, 1].astype(np.float64)
    worst = 0.0
    for f, (a, b, c) in enumerate([(6, 7, None), (0, 1, 2), (3, 4, 5)]):
        cst = np.ones(len(m)) if c is None else md[:, c]
        exact = md[:, a, None] * x[None, :] + md[:, b, None] * y[None, :] + cst[:, None]
        mag = np.abs(md[:, a, None] * x[None, :]) + np.abs(md[:, b, None] * y[None, :]) + np.abs(cst)[:, None]
        flush = 2.0 ** -122 * (np.abs(md[:, a]) + np.abs(md[:, b]))[:, None] + \
            2.0 ** -122 * (np.abs(x) + np.abs(y) + 1.0)[None, :]
        err = np.abs(out[:, :, f].astype(np.float64) - exact)
        ratio = np.max((err - flush).clip(min=0) / (U * mag + 1e-300))
        worst = max(worst, float(ratio))
        assert np.all(err <= DOT_C * U * mag + flush), (name, f, ratio)
    print(f"{name}: worst |dot - exact| = {worst:.3f} u sum|terms|")


@pytest.mark.parametrize("n", [4099, 8192])
def test_staged_parity_under_the_matrix_core_form(gpu, oracle, n):
    import torch
    from minicv_amd import device as D
    dev = torch.device("cuda:0")
    src, dst, _ = S.homography_problem(n, 12)
    pts = D.pack_points_tensor(src, dst, dev)
    cfg = opencv.RansacParams(threshold=5e-3, seed=12, fixed_iters=True, max_iters=4096).to_c()
    keys = {}
    L = N.lib()
    for label, staging, form, with_counts in (("staged mfma", 1, 2, False), ("staged mixed", 1, 3, False),
                                              ("unstaged mfma", 2, 2, True), ("unstaged valu", 2, 1, True)):
        plan = D.RansacPlan(N.MODEL_HOMOGRAPHY, n, 4096)
        key = torch.zeros(2, dtype=torch.int64, device=dev)
        counts = torch.zeros(4096, dtype=torch.int32, device=dev) if with_counts else None
        ps, pf = L.mcvTestHStaging(staging, None), L.mcvTestHMfma(form, None)
        try:
            plan.evaluate(pts, n, cfg, 0, 4096, key, counts)
            torch.cuda.synchronize()
            st = (C.c_longlong * 16)()
            L.mcvTestHStaging(-1, C.addressof(st))
        finally:
            L.mcvTestHStaging(ps, None)
            L.mcvTestHMfma(pf, None)
        keys[label] = ([int(v) for v in key.cpu().numpy()], counts.cpu().numpy() if with_counts else None, int(st[0]))
        plan.close()
    ref = oracle.h_counts(oracle.pack4(src, dst), 12, 0, 4096, THR2)
    np.testing.assert_array_equal(keys["unstaged mfma"][1], ref)
    np.testing.assert_array_equal(keys["unstaged valu"][1], ref)
    assert keys["staged mfma"][2] == 0 and keys["staged mixed"][2] == 0   # the stages pruned
    assert keys["staged mfma"][0] == keys["staged mixed"][0] == keys["unstaged mfma"][0] == keys["unstaged valu"][0]
