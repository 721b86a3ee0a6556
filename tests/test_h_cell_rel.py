"""The second pass of the per-cell bound (minicv_amd/csrc/h_cell_bound.h: the candidate-relative test on the cells
of the candidate's inliers, united with the box test) and the per-slot `left` figures of the later compactions,
through the host twin (mcvTestHCellRel, device = 0): a certified (model, cell) never holds an inlier of the
reference's op-by-op error, count(p) + left(p) never undercuts a model's count, `left` is what the cell ids and
the bitmaps say, and the relative test prunes what the issue's model says it does. CPU only; the device kernels
are compared with this twin in test_gpu_h_cell_rel.py."""
import numpy as np
import pytest

import _h_cell as HC
import _h_cell_rel as HR
from minicv_amd import synthetic as S

THR = 5e-3
THR2 = float(np.float32(THR * THR))
G, GS = 4, 12
REL = G ** 4            # first cell of the candidate's inliers


def perturbed(best, rng):
    """Copies of the candidate at relative perturbations 1e-6 .. 1e-1: the dangerous models are the near ones."""
    out = []
    for rel in (1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1):
        for _ in range(8):
            out.append(best * (1 + rel * rng.standard_normal(8)))
    return np.array(out, np.float32)


def crafted_models(rng, H):
    """Models whose vanishing line w = 0 crosses the point set [-1, 1]^2, grazes it, or lies far outside; huge and
    tiny coefficients; affine, zero and non-finite ones (the recipe of test_h_cell_bound.py)."""
    out = []
    base = (H / H[2, 2]).ravel()[:8]
    for _ in range(60):
        h = base * (1 + 0.05 * rng.standard_normal(8))
        a = rng.uniform(0, 2 * np.pi)
        r = rng.choice([0.5, 1.0, 1.2, 1.4, 1.5, 2.0, 5.0, 40.0])
        h[6], h[7] = r * np.cos(a), r * np.sin(a)
        out.append(h)
    for s in (1e-20, 1e-6, 1e6, 1e20, 1e35):
        out.append(base * s)
        h = base.copy()
        h[6:] *= s
        out.append(h)
    out.append(np.zeros(8))
    out.append(np.array([1, 0, 0, 0, 1, 0, 0, 0], float))
    out.append(np.array([1, 0, 0, 0, 1, 0, -1, 0], float))
    out.append(np.array([np.nan, 0, 0, 0, 1, 0, 0, 0], float))
    out.append(np.array([1, 0, 0, 0, 1, 0, np.inf, 0], float))
    return np.array(out, np.float32)


@pytest.mark.parametrize("share", [0.0, 0.2, 0.5, 0.8, 0.95])
def test_soundness_on_oracle_hypotheses(native, oracle, share):
    src, dst, _ = S.homography_problem(4096, 11, outlier_frac=share)
    pts4 = oracle.pack4(src, dst)
    models = HC.oracle_models(oracle, pts4, 11, 2000)
    cnt = oracle.h_counts(pts4, 11, 0, 2000, THR2)
    cnt = cnt[cnt >= 0]
    k = int(np.argmax(cnt))
    best, B = models[k], int(cnt.max())
    models = np.concatenate([models, perturbed(best, np.random.default_rng(5))])
    out = HR.run(native.lib(), pts4, best, models, THR2, B, HR.boundaries(4096))
    full, _ = HR.check_sound(oracle, pts4, models, THR2, out)
    HR.check_left(out)
    # the candidate itself: none of its own inlier cells is certified, and it is never dropped
    assert full[k] == B and out["ub"][k] >= B
    assert not out["cert"][k, REL:].any()
    assert out["alive"] == int((out["ub"] >= B).sum())
    box = HC.run(native.lib(), pts4, best, models, THR2, B)
    assert (out["cert"] | ~box["cert"]).all()            # the union holds every cell the box test certifies
    np.testing.assert_array_equal(out["cert"][:, :REL], box["cert"][:, :REL])
    print(f"share {share}: pruned {(out['ub'] < B).mean():.3f} (box only {(box['ub'] < B).mean():.3f}) of "
          f"{len(models)} models, B {B}")


def test_vanishing_lines_of_models_and_candidates(native, oracle):
    """Models and candidates whose w = 0 line crosses or grazes the set: sound whichever of them is the candidate."""
    rng = np.random.default_rng(7)
    src, dst, _ = S.homography_problem(4096, 12, outlier_frac=0.5)
    pts4 = oracle.pack4(src, dst)
    models = crafted_models(rng, S.H_TRUE)
    true = (S.H_TRUE / S.H_TRUE[2, 2]).ravel()[:8].astype(np.float32)
    cands = [true] + [models[i] for i in (0, 1, 2, 3, 7, 11, 60, 61, 62, 63, 70, 72, 73, 74)]
    certified = 0
    for cand in cands:
        out = HR.run(native.lib(), pts4, cand, np.concatenate([models, true[None, :]]), THR2, 100, HR.boundaries(4096))
        HR.check_sound(oracle, pts4, np.concatenate([models, true[None, :]]), THR2, out)
        HR.check_left(out)
        certified += int(out["cert"][:, REL:].sum())
    assert certified > 0
    # a cell the zero line of the candidate's w crosses is never certified by the relative test: with the
    # candidate w_c = 1 - 4 x (it keeps the points it maps near their destinations, if any) and a far model
    cand = np.array([1, 0, 0, 0, 1, 0, -4, 0], np.float32)
    far = np.array([[1, 0, 50, 0, 1, 50, 0, 0]], np.float32)
    o2 = HR.run(native.lib(), pts4, cand, far, THR2, 100, HR.boundaries(4096))
    b = HC.run(native.lib(), pts4, cand, far, THR2, 100)
    crossing = (b["sizes"] > 0) & (b["boxes"][:, 0] <= 0.25) & (b["boxes"][:, 1] >= 0.25)
    crossing[:REL] = False
    np.testing.assert_array_equal(o2["cert"][0, crossing], b["cert"][0, crossing])


def test_offsets_within_ulps_of_the_relative_flip(native, oracle):
    """One cell of candidate inliers, as wide as a cell of the 12 x 12 grid gets, its destinations across the
    candidate's whole inlier band (so the destination box is far too wide for the box test), and a model that is the
    candidate shifted by f in x': bisect f to the float at which the cell flips to certified, then step the model's
    h2 by +-2 ulp around it. The flip sits at 2 kappa, the double of the box test's margin: between 2 thr and
    1.1 x 2 thr."""
    L = native.lib()
    rng = np.random.default_rng(9)
    c = ((S.H_TRUE / S.H_TRUE[2, 2]).ravel()[:8] * (1 + 1e-3 * rng.standard_normal(8))).astype(np.float32)
    cd = c.astype(np.float64)
    ps = np.stack([rng.uniform(0.17, 0.33, 60), rng.uniform(0.17, 0.33, 60)], 1).astype(np.float32)   # inside bin (7, 7)
    w = cd[6] * ps[:, 0] + cd[7] * ps[:, 1] + 1
    proj = np.stack([(cd[0] * ps[:, 0] + cd[1] * ps[:, 1] + cd[2]) / w, (cd[3] * ps[:, 0] + cd[4] * ps[:, 1] + cd[5]) / w], 1)
    d = proj.copy()
    d[:, 0] += np.tile([0.98 * THR, -0.98 * THR, 0.0], 20)     # still the candidate's inliers
    anchors = np.array([[-1, -1, -1.5, -1.5], [1, 1, 1.5, 1.5], [-1, 1, 1.5, -1.5], [1, -1, -1.5, 1.5]], np.float32)
    pts4 = np.concatenate([np.concatenate([ps, d.astype(np.float32)], 1), anchors]).astype(np.float32)
    n = len(pts4)

    def model(f, ulps=0):
        h = cd.copy()
        h[0] += f * cd[6]
        h[1] += f * cd[7]
        h[2] += f
        h = h.astype(np.float32)
        for _ in range(abs(ulps)):
            h[2] = np.nextafter(h[2], np.float32(np.inf if ulps > 0 else -np.inf))
        return h

    def state(h):
        out = HR.run(L, pts4, c, h[None, :], THR2, 1, [0, (n + 1) // 2])
        cell = out["cell"][0]
        assert cell >= REL and (out["cell"][:60] == cell).all()      # one cell of the candidate's inliers
        HR.check_sound(oracle, pts4, h[None, :], THR2, out)
        assert not HC.run(L, pts4, c, h[None, :], THR2, 1)["cert"][0, cell]   # never the box test's doing
        return bool(out["cert"][0, cell])

    lo, hi = THR, 4 * THR
    assert not state(model(lo)) and state(model(hi))
    for _ in range(50):
        mid = 0.5 * (lo + hi)
        if state(model(mid)):
            hi = mid
        else:
            lo = mid
    print(f"flip at {hi / THR:.4f} thr")
    assert 2 * THR < hi < 1.1 * 2 * THR
    seen = set()
    for f in (lo, hi):
        for ulps in (-2, -1, 0, 1, 2):
            seen.add(state(model(f, ulps)))
    assert seen == {False, True}


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("col", [0, 3])
def test_non_finite_coordinate_certifies_nothing(native, oracle, bad, col):
    src, dst, _ = S.homography_problem(500, 14, outlier_frac=0.5)
    pts4 = oracle.pack4(src, dst)
    pts4[123, col] = bad
    models = HC.oracle_models(oracle, pts4, 14, 100)
    out = HR.run(native.lib(), pts4, models[0], models, THR2, 10, HR.boundaries(500))
    assert out["cell"].min() >= 0 and out["cell"].max() < HC.cells()
    assert not out["cert"].any() and (out["ub"] == 500).all() and out["alive"] == len(models)
    HR.check_left(out)


@pytest.mark.parametrize("thr2,inside", [(2.0 ** -100, True), (2.0 ** 20, True), (2.0 ** -101, False),
                                         (2.0 ** 21, False)])
def test_threshold_at_the_ends_of_the_domain(native, oracle, thr2, inside):
    scale = 1e-12 if thr2 < 1 else 1e5
    src, dst, _ = S.homography_problem(1000, 15, outlier_frac=0.5, sigma=0.0)
    unit = oracle.pack4(src, dst)
    pts4 = (unit.astype(np.float64) * scale).astype(np.float32)
    models = HC.oracle_models(oracle, unit, 15, 300).astype(np.float64)
    models *= np.array([1, 1, scale, 1, 1, scale, 1 / scale, 1 / scale])
    models = models.astype(np.float32)
    cnt, _ = HC.masks(oracle, pts4, models, thr2)
    out = HR.run(native.lib(), pts4, models[int(np.argmax(cnt))], models, thr2, int(cnt.max()), HR.boundaries(1000))
    HR.check_sound(oracle, pts4, models, thr2, out)
    HR.check_left(out)
    if not inside:
        assert not out["cert"].any()


def restated_shares(pts4, cell, cand, models, B, thr):
    """The bound restated in exact arithmetic (float64, no beta) on the twin's own partition. Box test: w keeps its
    sign at the four source corners and their images lie beyond the destination box by more than 1.02 thr on one
    side. Relative test (cells of the candidate's inliers): with D = u w_c - u_c w (x) or v w_c - v_c w (y) and
    P = w w_c, the centre-radius lower bound of +-s s_c D - 2 x 1.02 thr |P| over the source box is positive.
    -> (share of models with UB < B under the box test alone, under the union)."""
    p = pts4.astype(np.float64)
    used = np.unique(cell)
    lo = np.array([p[cell == c].min(0) for c in used])
    hi = np.array([p[cell == c].max(0) for c in used])
    size = np.array([(cell == c).sum() for c in used])
    inl = used >= REL
    cx = np.stack([lo[:, 0], hi[:, 0], lo[:, 0], hi[:, 0]], 1)
    cy = np.stack([lo[:, 1], lo[:, 1], hi[:, 1], hi[:, 1]], 1)
    xc, yc = 0.5 * (lo[:, 0] + hi[:, 0]), 0.5 * (lo[:, 1] + hi[:, 1])
    rx, ry = 0.5 * (hi[:, 0] - lo[:, 0]), 0.5 * (hi[:, 1] - lo[:, 1])
    k = 2 * 1.02 * thr
    c = cand.astype(np.float64)
    wc_corner = c[6] * cx + c[7] * cy + 1
    sc_ok = (wc_corner > 0).all(1) | (wc_corner < 0).all(1)
    sc = np.sign(wc_corner[:, 0])

    def quad(a, b):     # coefficients xx, xy, yy, x, y, 1 of (a0 x + a1 y + a2)(b0 x + b1 y + b2)
        return np.array([a[0] * b[0], a[0] * b[1] + a[1] * b[0], a[1] * b[1], a[0] * b[2] + a[2] * b[0],
                         a[1] * b[2] + a[2] * b[1], a[2] * b[2]])

    def low(q):         # centre-radius lower bound of the quadratic q per cell
        val = q[0] * xc * xc + q[1] * xc * yc + q[2] * yc * yc + q[3] * xc + q[4] * yc + q[5]
        gx, gy = 2 * q[0] * xc + q[1] * yc + q[3], q[1] * xc + 2 * q[2] * yc + q[4]
        return val - abs(gx) * rx - abs(gy) * ry - (abs(q[0]) * rx * rx + abs(q[1]) * rx * ry + abs(q[2]) * ry * ry)

    Wc = np.array([c[6], c[7], 1.0])
    box_pruned = union_pruned = 0
    for h in models.astype(np.float64):
        w = h[6] * cx + h[7] * cy + 1
        px = (h[0] * cx + h[1] * cy + h[2]) / w
        py = (h[3] * cx + h[4] * cy + h[5]) / w
        same = (w > 0).all(1) | (w < 0).all(1)
        m = 1.02 * thr
        out = ((px > hi[:, 2:3] + m).all(1) | (px < lo[:, 2:3] - m).all(1) |
               (py > hi[:, 3:4] + m).all(1) | (py < lo[:, 3:4] - m).all(1))
        box = same & out
        W = np.array([h[6], h[7], 1.0])
        t = np.sign(w[:, 0]) * sc
        P = quad(W, Wc)
        rel = np.zeros(len(used), bool)
        for a, b in ((h[0:3], c[0:3]), (h[3:6], c[3:6])):
            D = quad(a, Wc) - quad(b, W)
            for sg in (1.0, -1.0):
                # +-t D - k t P with t per cell: both signs of t, picked per cell
                lp = low(sg * D - k * P)
                lm = low(-sg * D + k * P)
                rel |= np.where(t > 0, lp, lm) > 0
        rel &= inl & same & sc_ok
        box_pruned += size[~box].sum() < B
        union_pruned += size[~(box | rel)].sum() < B
    return box_pruned / len(models), union_pruned / len(models)


def test_effectiveness_on_the_cfg3_shape(native, oracle):
    src, dst, _ = S.homography_problem(8192, 3)
    pts4 = oracle.pack4(src, dst)
    models = HC.oracle_models(oracle, pts4, 3, 4096)
    cnt = oracle.h_counts(pts4, 3, 0, 4096, THR2)
    cnt = cnt[cnt >= 0]
    best, B = models[int(np.argmax(cnt))], int(cnt.max())
    out = HR.run(native.lib(), pts4, best, models, THR2, B, HR.boundaries(8192))
    box = HC.run(native.lib(), pts4, best, models, THR2, B)
    share, share_box = float((out["ub"] < B).mean()), float((box["ub"] < B).mean())
    ref_box, ref = restated_shares(pts4, out["cell"], best, models, B, THR)
    print(f"pruned share {share:.4f} (box only {share_box:.4f}); restated {ref:.4f} (box only {ref_box:.4f}); B {B}")
    assert ref - ref_box >= 0.05
    assert share - share_box >= 0.5 * (ref - ref_box)
    assert (out["ub"] >= cnt).all()
