"""Independent numpy restatement of the affine family (cv::estimateAffine2D, 3-point samples, and
cv::estimateAffinePartial2D, 2-point samples): the closed forms in np.float64 scalars,
the error in np.float32 operation by operation, the subset check, the sequential RANSAC loop, LMedS and
its sigma / mask step. The Philox samples come from mcvHostHypothesis' sampleIdx, the CV samples from a
Python restatement of cv::RNG (as tests/test_cv_sampler.py) plus the subset check. Nothing here calls the
code under test for a model, an error, a count or a median.
"""
from __future__ import annotations

import functools

import numpy as np

import _oracle as O
from minicv_amd import native as N

FLT_EPSILON = float(np.float32(1.19209290e-07))
NAN_KEY = 0xFFFFFFFF
f64 = np.float64
f32 = np.float32


def model_points(model: int) -> int:
    return 3 if model == N.MODEL_AFFINE else 2


# ---- subset check --------------------------------------------------------------------------------
def have_collinear(px, py) -> bool:
    """haveCollinearPoints: the last point against the lines through earlier pairs; float differences
    promoted to double, FLT_EPSILON test."""
    px = np.asarray(px, dtype=f32)
    py = np.asarray(py, dtype=f32)
    i = len(px) - 1
    for j in range(i):
        dx1, dy1 = f64(f32(px[j] - px[i])), f64(f32(py[j] - py[i]))
        for k in range(j):
            dx2, dy2 = f64(f32(px[k] - px[i])), f64(f32(py[k] - py[i]))
            if abs(dx2 * dy1 - dy2 * dx1) <= f64(FLT_EPSILON) * (abs(dx1) + abs(dy1) + abs(dx2) + abs(dy2)):
                return True
    return False


def check_subset(pts4, idx) -> bool:
    p = pts4[np.asarray(idx)]
    return not have_collinear(p[:, 0], p[:, 1]) and not have_collinear(p[:, 2], p[:, 3])


# ---- closed forms --------------------------------------------------------------------------------
def solve_affine(p):
    """p: 3 x {x, y, X, Y} float32 -> the 6 doubles of the 2x3 matrix (sums left to right)."""
    (x1, y1, X1, Y1), (x2, y2, X2, Y2), (x3, y3, X3, Y3) = [[f64(v) for v in r] for r in p]
    with np.errstate(all="ignore"):
        d = f64(1) / (x1 * (y2 - y3) + x2 * (y3 - y1) + x3 * (y1 - y2))
        out = []
        for a1, a2, a3 in ((X1, X2, X3), (Y1, Y2, Y3)):
            out.append(d * (a1 * (y2 - y3) + a2 * (y3 - y1) + a3 * (y1 - y2)))
            out.append(d * (a1 * (x3 - x2) + a2 * (x1 - x3) + a3 * (x2 - x1)))
            out.append(d * (a1 * (x2 * y3 - x3 * y2) + a2 * (x3 * y1 - x1 * y3) + a3 * (x1 * y2 - x2 * y1)))
    return np.array(out, dtype=f64)


def solve_similarity(p):
    (x1, y1, X1, Y1), (x2, y2, X2, Y2) = [[f64(v) for v in r] for r in p]
    with np.errstate(all="ignore"):
        dx, dy, dX, dY = x1 - x2, y1 - y2, X1 - X2, Y1 - Y2
        d = f64(1) / (dx * dx + dy * dy)
        S0 = d * (dX * dx + dY * dy)
        S1 = d * (dY * dx - dX * dy)
        S2 = d * (dY * (x1 * y2 - x2 * y1) - (X1 * y2 - X2 * y1) * dy - (X1 * x2 - X2 * x1) * dx)
        S3 = d * (-dX * (x1 * y2 - x2 * y1) - (Y1 * x2 - Y2 * x1) * dx - (Y1 * y2 - Y2 * y1) * dy)
    return np.array([S0, -S1, S2, S1, S0, S3], dtype=f64)


def solve(model, pts4, idx):
    """-> (status 1 / -1, A (6 doubles), Af (6 floats))."""
    p = pts4[np.asarray(idx)]
    A = solve_affine(p) if model == N.MODEL_AFFINE else solve_similarity(p)
    with np.errstate(all="ignore"):
        Af = A.astype(f32)
    ok = bool(np.isfinite(A).all() and np.isfinite(Af).all())
    return (1 if ok else -1), A, Af


# ---- error ---------------------------------------------------------------------------------------
def fma32(a, b, c):
    """float32 fma(a, b, c), exactly: the product is exact in float64, the sum is rounded to odd in
    float64 (TwoSum), and 53 >= 2 * 24 + 2 bits make the final rounding to float32 the correct one."""
    a, b, c = (np.asarray(v, dtype=f32).astype(f64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & np.isfinite(e) & (e != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(f32)


def errors(pts4, Af, fused: bool = False):
    """computeError over all points, float32: op by op (default) or the fused definition."""
    Af = np.asarray(Af, dtype=f32)
    x, y, X, Y = (np.ascontiguousarray(pts4[:, k], dtype=f32) for k in range(4))
    with np.errstate(all="ignore"):
        if fused:
            a = fma32(Af[0], x, fma32(Af[1], y, Af[2])) - X
            b = fma32(Af[3], x, fma32(Af[4], y, Af[5])) - Y
            return fma32(a, a, b * b)
        a = ((Af[0] * x + Af[1] * y) + Af[2]) - X
        b = ((Af[3] * x + Af[4] * y) + Af[5]) - Y
        return a * a + b * b


def count(pts4, Af, thr2, fused=False, want_mask=False):
    with np.errstate(all="ignore"):
        m = errors(pts4, Af, fused) <= f32(thr2)
    return (int(m.sum()), m.astype(np.uint8)) if want_mask else int(m.sum())


def keys(err):
    k = np.ascontiguousarray(err, dtype=f32).view(np.uint32).copy()
    k[np.isnan(err)] = NAN_KEY
    return k


def rank_value(pts4, Af, rank, fused=False):
    """The error of rank `rank` (0-based, ascending over the uint32 view, every NaN last)."""
    k = np.sort(keys(errors(pts4, Af, fused)))[rank]
    return f32(np.nan) if k == NAN_KEY else np.array([k], dtype=np.uint32).view(f32)[0]


def key_of(v) -> int:
    v = f32(v)
    return NAN_KEY if np.isnan(v) else int(np.array([v], dtype=f32).view(np.uint32)[0])


def same_bits(a, b) -> bool:
    return key_of(a) == key_of(b)


# ---- samples -------------------------------------------------------------------------------------
class CvRngPy:
    """cv::RNG: state = (uint64)(unsigned)state * 4164903690 + (unsigned)(state >> 32)."""

    def __init__(self, state: int = 0xFFFFFFFFFFFFFFFF):
        self.s = state & 0xFFFFFFFFFFFFFFFF

    def next(self) -> int:
        self.s = ((self.s & 0xFFFFFFFF) * 4164903690 + (self.s >> 32)) & 0xFFFFFFFFFFFFFFFF
        return self.s & 0xFFFFFFFF

    def uniform(self, a: int, b: int) -> int:
        return a if a == b else (self.next() % (b - a)) + a


def cv_subsets(model, pts4, n, rows, max_attempts=10000):
    """getSubset's stream with the family's checkSubset -> (accepted rows, int32[rows, m]); rows from the
    first failure on are -1."""
    m = model_points(model)
    rng = CvRngPy()
    out = np.full((rows, m), -1, dtype=np.int32)
    for h in range(rows):
        ok = False
        for _ in range(max_attempts):
            idx = []
            for i in range(m):
                while True:
                    v = rng.uniform(0, n)
                    if v not in idx:
                        break
                idx.append(v)
            if m == 2 or check_subset(pts4, idx):
                ok = True
                break
        if not ok:
            return h, out
        out[h] = idx
    return rows, out


def host_hypothesis(model, pts4, seed, hyp):
    """The product's host twin -> (status, A6, Af6, sample)."""
    A = np.zeros(9)
    Af = np.zeros(9, dtype=f32)
    idx = np.full(3, -1, dtype=np.int32)
    st = N.lib().mcvHostHypothesis(model, pts4.ctypes.data, pts4.shape[0], seed, hyp, A.ctypes.data, Af.ctypes.data,
                                   idx.ctypes.data)
    return st, A[:6].copy(), Af[:6].copy(), idx[:model_points(model)].copy()


class Samples:
    """Hypothesis h's sample: Philox (through the host twin's sampleIdx) or the Python CV stream."""

    def __init__(self, model, pts4, seed=0, cv=False, rows=0):
        self.model, self.pts4, self.seed, self.cv = model, pts4, seed, cv
        if cv:
            self.accepted, self.table = cv_subsets(model, pts4, pts4.shape[0], rows)

    def get(self, h):
        """-> index list, or None when the sampler gave up (status -2)."""
        if self.cv:
            return None if h >= self.accepted else self.table[h].tolist()
        st, _, _, idx = host_hypothesis(self.model, self.pts4, self.seed, h)
        return None if st == -2 else idx.tolist()


def hypothesis(model, pts4, samples: Samples, h):
    """-> (status, A, Af, idx): -2 no sample, -1 no model, 1."""
    idx = samples.get(h)
    if idx is None:
        return -2, None, None, None
    st, A, Af = solve(model, pts4, idx)
    return st, A, Af, idx


# ---- RANSAC / LMedS ------------------------------------------------------------------------------
def ransac_ref(model, pts4, thr, conf, max_iters, seed=0, cv=False, fixed=False, fused=False):
    """RANSACPointSetRegistrator::run restated -> None (no model) or dict(hyp, A, Af, idx, count, mask)."""
    n = pts4.shape[0]
    m = model_points(model)
    thr2 = float(f32(thr * thr))
    niters = max(max_iters, 1)
    samples = Samples(model, pts4, seed, cv, niters)
    best, best_count = None, 0
    it = 0
    while it < niters:
        st, A, Af, idx = hypothesis(model, pts4, samples, it)
        if st == -2:
            break
        if st == 1:
            c = count(pts4, Af, thr2, fused)
            if c > max(best_count, m - 1):
                best_count = c
                best = dict(hyp=it, A=A, Af=Af, idx=idx)
                if not fixed:
                    niters = O.load().orc_update_num_iters(conf, (n - c) / n, m, niters)
        it += 1
    if best is None:
        return None
    c, mask = count(pts4, best["Af"], thr2, fused, want_mask=True)
    best.update(count=c, mask=mask, thr2=thr2)
    return best


def lmeds_ref(model, pts4, conf, max_iters, seed=0, cv=False, fixed=False, fused=False):
    """LMeDSPointSetRegistrator::run restated -> None (the call fails) or dict(hyp, A, Af, med, sigma, count, mask)."""
    n = pts4.shape[0]
    m = model_points(model)
    niters = max_iters if fixed else O.load().orc_update_num_iters(conf, 0.45, m, max_iters)
    samples = Samples(model, pts4, seed, cv, niters)
    best = None
    for h in range(niters):
        st, A, Af, idx = hypothesis(model, pts4, samples, h)
        if st == -2:
            if h == 0:
                return None
            break
        if st != 1:
            continue
        med = rank_value(pts4, Af, n // 2, fused)
        if best is None or key_of(med) < key_of(best["med"]):
            best = dict(hyp=h, A=A, Af=Af, idx=idx, med=med)
    if best is None or np.isnan(best["med"]):
        return None
    sigma = max(2.5 * 1.4826 * (1 + 5.0 / (n - m)) * float(np.sqrt(f64(best["med"]))), 0.001)
    thr2 = float(f32(sigma * sigma))
    c, mask = count(pts4, best["Af"], thr2, fused, want_mask=True)
    if c < m:
        return None
    best.update(sigma=sigma, thr2=thr2, count=c, mask=mask)
    return best


# ---- refine --------------------------------------------------------------------------------------
def lstsq_model(model, pts4, mask):
    """The exact optimum of the refine's cost (linear least squares in the parameters) on the masked points."""
    p = pts4[np.asarray(mask, dtype=bool)].astype(f64)
    x, y, X, Y = p[:, 0], p[:, 1], p[:, 2], p[:, 3]
    one, zero = np.ones_like(x), np.zeros_like(x)
    if model == N.MODEL_AFFINE:
        M = np.concatenate([np.stack([x, y, one, zero, zero, zero], 1), np.stack([zero, zero, zero, x, y, one], 1)])
        h = np.linalg.lstsq(M, np.concatenate([X, Y]), rcond=None)[0]
        return h
    M = np.concatenate([np.stack([x, -y, one, zero], 1), np.stack([y, x, zero, one], 1)])
    a, b, tx, ty = np.linalg.lstsq(M, np.concatenate([X, Y]), rcond=None)[0]
    return np.array([a, -b, tx, b, a, ty])


def cost(pts4, mask, A6):
    p = pts4[np.asarray(mask, dtype=bool)].astype(f64)
    rx = A6[0] * p[:, 0] + A6[1] * p[:, 1] + A6[2] - p[:, 2]
    ry = A6[3] * p[:, 0] + A6[4] * p[:, 1] + A6[5] - p[:, 3]
    return float(np.sum(rx * rx + ry * ry))


def rel(a, b) -> float:
    """Relative Frobenius deviation of a from b."""
    a, b = np.asarray(a, dtype=f64).ravel(), np.asarray(b, dtype=f64).ravel()
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def host_refine(model, pts4, mask, A6):
    A = np.array(A6, dtype=f64).copy()
    mk = np.ascontiguousarray(mask, dtype=np.uint8)
    used = N.lib().mcvHostAffineRefine(model, pts4.ctypes.data, pts4.shape[0], mk.ctypes.data, A.ctypes.data)
    assert used == int(mk.astype(bool).sum()), N.last_error()
    return A


# The largest relative deviation of mcvHostAffineRefine from numpy.linalg.lstsq over test_affine.py's seeds,
# measured on the CPU, and the tests' bound: 10x that (other seeds, libm builds).
LSTSQ_DEV_MEASURED = 7.97e-14
LSTSQ_BOUND = 10 * LSTSQ_DEV_MEASURED


# ---- shared cases --------------------------------------------------------------------------------
SIZES = (2, 3, 4, 63, 64, 65, 257, 1000, 4099)
MODELS = (N.MODEL_AFFINE, N.MODEL_SIMILARITY)


def scene(model, n, seed, outlier_frac=0.3):
    from minicv_amd import synthetic as S
    src, dst, inl, A = S.affine_problem(n, seed, outlier_frac=outlier_frac, similarity=model == N.MODEL_SIMILARITY)
    return O.pack4(src, dst), inl, A


def subnormal_set(n, rng):
    """Points whose residuals under the identity lie between 1e-23 and 1e-20: a * a is subnormal in float32
    (from its last few bits at 1e-23 up to 1e-40)."""
    p = np.empty((n, 4), dtype=f32)
    p[:, :2] = rng.uniform(-1e-18, 1e-18, (n, 2)).astype(f32)
    r = 10.0 ** rng.uniform(-23, -20, (n, 2)) * rng.choice([-1.0, 1.0], (n, 2))
    p[:, 2:] = (p[:, :2].astype(f64) + r).astype(f32)
    return np.ascontiguousarray(p)


IDENTITY = np.array([1, 0, 0, 0, 1, 0], dtype=f32)


@functools.lru_cache(maxsize=None)
def rank_cases():
    """-> list of (label, errKind, pts4, models [k, 6] f32, ranks, expected [len(ranks), k]); computed once."""
    out = []
    for n in SIZES:
        rng = np.random.default_rng(3000 + n)
        ranks = sorted({0, n // 2, n - 1})
        pts, _, A = scene(N.MODEL_AFFINE, n, 50 + n)
        near = (A.ravel() + rng.normal(0, 1e-3, 6)).astype(f32)
        nan_model = np.array([np.nan, 0, 0, 0, 1, 0], dtype=f32)
        models = np.ascontiguousarray(np.stack([near, rng.normal(0, 1, 6).astype(f32), nan_model, IDENTITY]))
        equal = np.ascontiguousarray(np.tile(pts[:1], (n, 1)))
        nanpts = pts.copy()
        # odd n: the median is a NaN; even n: it is the last finite error
        nanpts[: (n // 2 + 1 if n % 2 else n // 2 - 1), 2] = np.nan
        for tag, p in (("spread", pts), ("equal", equal), ("nan", np.ascontiguousarray(nanpts)),
                       ("subnormal", subnormal_set(n, rng))):
            for fused in (0, 1):
                out.append([f"{tag}-n{n}-fused{fused}", fused, p, models, ranks])
    for c in out:
        _, fused, p, models, ranks = c
        exp = np.empty((len(ranks), models.shape[0]), dtype=f32)
        for i, r in enumerate(ranks):
            for j in range(models.shape[0]):
                exp[i, j] = rank_value(p, models[j], r, bool(fused))
        c.append(exp)
    return [tuple(c) for c in out]


def run_rank_hook(fn, model, kind, pts4, models, rank):
    vals = np.full(models.shape[0], -1.0, dtype=f32)
    ok = fn(model, pts4.ctypes.data, pts4.shape[0], models.ctypes.data, models.shape[0], kind, rank, vals.ctypes.data)
    assert ok == 1, N.last_error()
    return vals
