"""GPU tests of the batched matcher (cvMatchFeaturesBatch / cvMatchAndFindModelBatch, match_batch.hip):
the raw knn-2 of every directed problem against the references, ties and tile edges, isolation of a
problem from the images stored around its train image, the export against the loop of single calls bit for
bit, launches and synchronisations that do not depend on the batch, and the fused call against
matchFeaturesBatch + findModelBatch."""
import ctypes as C
import functools

import numpy as np
import pytest

import _matcher_cases as MC
from _l2u8_ref import assert_same, match_l2_u8
from minicv_amd import native as N
from minicv_amd import opencv, synthetic as S

pytestmark = pytest.mark.gpu

INT_MAX = np.iinfo(np.int32).max
SIZES = [0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257]


# ---- helpers ---------------------------------------------------------------------------------------
def knn_batch(rows, directed, norm):
    """mcvTestMatchBatchKnn on a list of uint8 [n_i][dim] images -> per directed problem (idx, dist, idx2, dist2)."""
    dim = rows[0].shape[1]
    counts = np.array([r.shape[0] for r in rows], dtype=np.int32)
    cat = np.ascontiguousarray(np.concatenate(rows, axis=0))
    dp = np.ascontiguousarray(np.asarray(directed, dtype=np.int32).reshape(-1, 2))
    n = int(sum(counts[i] for i in dp[:, 0]))
    dt = np.int32 if norm == N.NORM_HAMMING else np.float32
    idx, idx2 = np.full(max(n, 1), -9, np.int32), np.full(max(n, 1), -9, np.int32)
    d1, d2 = np.zeros(max(n, 1), dt), np.zeros(max(n, 1), dt)
    got = N.lib().mcvTestMatchBatchKnn(cat.ctypes.data, counts.ctypes.data, len(rows), dim, dp.ctypes.data, len(dp), norm,
                                       idx.ctypes.data, d1.ctypes.data, idx2.ctypes.data, d2.ctypes.data)
    assert got == n, N.last_error()
    out, o = [], 0
    for i, _ in dp:
        c = int(counts[i])
        out.append((idx[o:o + c], d1[o:o + c], idx2[o:o + c], d2[o:o + c]))
        o += c
    return out


def reference(oracle, q, t, norm):
    if norm == N.NORM_HAMMING:
        return oracle.match_hamming(q, t)
    return match_l2_u8(q, t)


def same(got, ref, norm):
    if norm == N.NORM_HAMMING:
        for g, r in zip(got, ref):
            np.testing.assert_array_equal(g, r)
    else:
        assert_same(got, ref)


def stats():
    st = np.zeros(8, dtype=np.int64)
    assert N.lib().mcvTestMatchBatchStats(st.ctypes.data) == 1
    return {"launches": int(st[0]), "syncs": int(st[1]), "problems": int(st[2]), "workgroups": int(st[3]),
            "copies": int(st[4])}


# ---- 1. raw knn-2 against the references -----------------------------------------------------------
@pytest.mark.parametrize("norm,dim", [(N.NORM_HAMMING, 32), (N.NORM_HAMMING, 64), (N.NORM_HAMMING, 61),
                                      (N.NORM_HAMMING, 1), (N.NORM_L2, 128), (N.NORM_L2, 61)])
def test_raw_knn_against_reference(gpu, oracle, norm, dim):
    rng = np.random.default_rng(7 * dim + norm)
    # few distinct values per byte at L2: exact ties happen between different rows
    rows = [rng.integers(0, 256 if norm == N.NORM_HAMMING else 4, size=(n, dim), dtype=np.uint8) for n in SIZES]
    n = len(SIZES)
    directed = [(i, j) for i in range(n) for j in range(n)]      # both orders and (i, i)
    got = knn_batch(rows, directed, norm)
    assert stats()["problems"] == len(directed)
    for (i, j), g in zip(directed, got):
        ref = reference(oracle, rows[i], rows[j], norm)
        if SIZES[j] == 0:
            assert (g[0] == -1).all() and (g[2] == -1).all()
        if SIZES[j] < 2 and SIZES[i] > 0:
            assert (g[2] == -1).all()
            assert (g[3] == INT_MAX).all() if norm == N.NORM_HAMMING else np.isinf(g[3]).all()
        same(g, ref, norm)


# ---- 2. ties and edges, Hamming --------------------------------------------------------------------
@pytest.mark.parametrize("nbytes", [32, 64, 61])
def test_hamming_plants_and_saturation(gpu, nbytes):
    rng = np.random.default_rng(nbytes)
    t = rng.integers(0, 256, size=(300, nbytes), dtype=np.uint8)
    q, idx, dist, idx2, dist2 = MC.hamming_plants(t, 70)
    tsat = np.full((300, nbytes), 255, np.uint8)
    qsat = np.where((np.arange(70) % 2 == 0)[:, None], 0, 255).astype(np.uint8) * np.ones((1, nbytes), np.uint8)
    filler = rng.integers(0, 256, size=(45, nbytes), dtype=np.uint8)
    rows = [filler, q, t, qsat, tsat, filler]
    got = knn_batch(rows, [(1, 2), (3, 4), (0, 5)], N.NORM_HAMMING)
    same(got[0], (idx, dist, idx2, dist2), N.NORM_HAMMING)
    sat = np.where(np.arange(70) % 2 == 0, 8 * nbytes, 0).astype(np.int32)
    same(got[1], (np.zeros(70, np.int32), sat, np.ones(70, np.int32), sat), N.NORM_HAMMING)


# ---- 3. ties and edges, byte SIFT ------------------------------------------------------------------
@pytest.mark.parametrize("dim", [128, 61])
@pytest.mark.parametrize("nt", [65, 257])
def test_l2u8_duplicate_rows(gpu, dim, nt):
    rng = np.random.default_rng(dim + nt)
    ta = rng.integers(0, 256, size=(nt, dim), dtype=np.uint8)
    tb = ta.copy()
    r = rng.integers(0, 256, size=dim, dtype=np.uint8)
    ta[[0, 31, 32, nt - 1]] = r
    tb[[32, nt - 1]] = r
    q = rng.integers(0, 256, size=(40, dim), dtype=np.uint8)
    q[::3] = r
    got = knn_batch([q, ta, tb], [(0, 1), (0, 2)], N.NORM_L2)
    for g, t, first, second in ((got[0], ta, 0, 31), (got[1], tb, 32, nt - 1)):
        assert (g[0][::3] == first).all() and (g[2][::3] == second).all()
        assert (g[1][::3] == 0).all() and (g[3][::3] == 0).all()
        assert_same(g, match_l2_u8(q, t))


# ---- 4. isolation ----------------------------------------------------------------------------------
@pytest.mark.parametrize("norm,dim", [(N.NORM_HAMMING, 32), (N.NORM_HAMMING, 61), (N.NORM_L2, 128), (N.NORM_L2, 61)])
@pytest.mark.parametrize("nt", [33, 65])
def test_problem_is_isolated_from_its_neighbours(gpu, oracle, norm, dim, nt):
    """Exact copies of a query sit in the first and last rows of the images stored right before and right
    after the train image: a tile that read past the train image's ends would find them at distance 0."""
    rng = np.random.default_rng(dim + nt)
    q = rng.integers(0, 256, size=(50, dim), dtype=np.uint8)
    t = rng.integers(0, 256, size=(nt, dim), dtype=np.uint8)
    before = rng.integers(0, 256, size=(40, dim), dtype=np.uint8)
    after = rng.integers(0, 256, size=(40, dim), dtype=np.uint8)
    before[0], before[-1], after[0], after[-1] = q[3], q[7], q[3], q[49]
    rows = [q, before, t, after]
    got = knn_batch(rows, [(0, 1), (0, 2), (0, 3), (2, 2)], norm)
    ref = reference(oracle, q, t, norm)
    assert ref[1][3] > 0 and ref[1][7] > 0 and ref[1][49] > 0      # no copy inside the train image itself
    same(got[1], ref, norm)
    same(got[0], reference(oracle, q, before, norm), norm)
    assert got[0][1][3] == 0 and got[2][1][49] == 0               # the neighbours do hold the copies


# ---- 5. the export equals the loop ------------------------------------------------------------------
# features of image a -> survivors of (a, b) at ratio 0.8 with cross-check, b = feature_pair_problem's partner
SURVIVORS = {31: 16, 32: 15, 33: 14, 63: 31, 64: 31, 65: 28, 127: 56, 128: 58, 129: 59, 255: 120, 256: 115,
             257: 116, 300: 130, 513: 222}


def partner(n):
    return n + 3 if n in (32, 33) else n - 7


@functools.lru_cache(maxsize=None)
def planted_images(sizes, kind):
    """For each n: the two images of feature_pair_problem(n, partner(n), seed=100 + n) -> (points, descriptors)."""
    out = []
    for n in sizes:
        pa, da, pb, db, _ = S.feature_pair_problem(n, partner(n), seed=100 + n, kind=kind)
        out += [(pa, da), (pb, db)]
    for p, d in out:
        p.setflags(write=False)
        d.setflags(write=False)
    return tuple(out)


def expected_pairs(oracle, da, db, ratio, cross, maxd):
    idx, d1, idx2, d2 = oracle.match_hamming(da, db)
    d1f = d1.astype(np.float32)
    d2f = np.where(d2 == INT_MAX, np.float32(np.inf), d2.astype(np.float32))
    keep = idx >= 0
    if ratio > 0:
        keep &= d1f < np.float32(ratio) * d2f
    if maxd > 0:
        keep &= d1f <= np.float32(maxd)
    if cross:
        back = oracle.match_hamming(db, da)[0]
        keep &= back[np.maximum(idx, 0)] == np.arange(len(idx))
    q = np.nonzero(keep)[0]
    return np.stack([q, idx[q]], axis=1).astype(np.int32), d1f[q]


EXPORT_SIZES = (33, 65, 129, 257)
EXPORT_PAIRS = [(0, 1), (1, 0), (2, 3), (3, 2), (4, 5), (5, 4), (6, 7), (7, 6)]


def test_survivor_table_in_numpy(gpu, oracle):
    for k, n in enumerate(EXPORT_SIZES):
        imgs = planted_images(EXPORT_SIZES, "hamming")
        ep, _ = expected_pairs(oracle, imgs[2 * k][1], imgs[2 * k + 1][1], 0.8, True, 0)
        assert len(ep) == SURVIVORS[n]


@pytest.mark.parametrize("norm", [N.NORM_HAMMING, N.NORM_L2])
@pytest.mark.parametrize("ratio", [0.8, 0.0, 0.75])
@pytest.mark.parametrize("cross", [True, False])
@pytest.mark.parametrize("maxd", [0.0, 60.0])
def test_export_equals_the_loop(gpu, oracle, norm, ratio, cross, maxd):
    imgs = planted_images(EXPORT_SIZES, "hamming" if norm == N.NORM_HAMMING else "sift_u8")
    feats = [opencv.Features(p, d) for p, d in imgs]
    got = opencv.matchFeaturesBatch(feats, EXPORT_PAIRS, ratio=ratio, cross_check=cross, max_distance=maxd, norm=norm)
    assert len(got) == len(EXPORT_PAIRS)
    for (i, j), (pairs, dist) in zip(EXPORT_PAIRS, got):
        lp, ld = opencv.matchFeatures(feats[i], feats[j], ratio=ratio, cross_check=cross, max_distance=maxd, norm=norm)
        assert len(pairs) >= 8
        np.testing.assert_array_equal(pairs, lp)
        np.testing.assert_array_equal(dist.view(np.uint32), ld.view(np.uint32))
        if norm == N.NORM_HAMMING:
            ep, ed = expected_pairs(oracle, imgs[i][1], imgs[j][1], ratio, cross, maxd)
            np.testing.assert_array_equal(pairs, ep)
            np.testing.assert_array_equal(dist, ed)


@pytest.mark.parametrize("norm", [N.NORM_AUTO, N.NORM_L2])
def test_offsets_are_the_cumulative_counts(gpu, norm):
    imgs = planted_images(EXPORT_SIZES, "hamming" if norm == N.NORM_AUTO else "sift_u8")
    feats = [opencv.Features(p, d) for p, d in imgs]
    ip = np.array(EXPORT_PAIRS, dtype=np.int32)
    structs = (N.DetectorResult * len(feats))(*[f.struct for f in feats])
    cap = sum(imgs[i][0].shape[0] for i, _ in EXPORT_PAIRS)
    pairs = np.zeros((cap, 2), np.int32)
    offsets = np.full(len(ip) + 1, -7, np.int32)
    total = N.lib().cvMatchFeaturesBatch(C.addressof(structs), len(feats), ip.ctypes.data, len(ip), None, norm,
                                         pairs.ctypes.data, None, cap, offsets.ctypes.data)     # NULL cfg and dist
    assert total > 0, N.last_error()
    counts = [len(opencv.matchFeatures(feats[i], feats[j], norm=norm)[0]) for i, j in EXPORT_PAIRS]
    assert offsets.tolist() == [0] + np.cumsum(counts).tolist() and total == offsets[-1]
    for p in range(len(ip)):
        assert (np.diff(pairs[offsets[p]:offsets[p + 1], 0]) > 0).all()


# ---- 6. launches and synchronisations do not depend on the batch -------------------------------------
@pytest.mark.parametrize("norm,dim", [(N.NORM_HAMMING, 32), (N.NORM_HAMMING, 61), (N.NORM_L2, 128)])
def test_launches_do_not_depend_on_the_batch(gpu, norm, dim):
    rng = np.random.default_rng(dim)
    feats = [opencv.Features(rng.uniform(0, 100, (n, 2)), rng.integers(0, 256, size=(n, dim), dtype=np.uint8))
             for n in (40, 70, 100, 130, 64, 65, 200, 33, 90, 257, 128, 50)]
    batches = {
        "B = 2": [(0, 1), (2, 3)],
        "B = 40": [(i % 12, (5 * i + 1) % 12) for i in range(40)],
        "every image in one pair": [(2 * k, 2 * k + 1) for k in range(6)],
        "one image in 20 pairs": [(3, k % 12) for k in range(10)] + [(k % 12, 3) for k in range(10)],
    }
    seen = {}
    for cross in (False, True):
        for name, pairs in batches.items():
            out = opencv.matchFeaturesBatch(feats, pairs, ratio=0.0, cross_check=cross, norm=norm)
            assert sum(len(p) for p, _ in out) > 0
            st = stats()
            assert st["problems"] == (2 if cross else 1) * len(pairs)
            seen[(cross, name)] = (st["launches"], st["syncs"], st["copies"])
    assert len(set(seen.values())) == 1, seen
    launches, syncs, copies = next(iter(seen.values()))
    assert launches == (5 if (norm, dim) == (N.NORM_HAMMING, 32) else 6) and syncs == 2 and copies == 5


# ---- 7. errors on the device path ------------------------------------------------------------------
def test_device_path_edges(gpu):
    imgs = planted_images(EXPORT_SIZES, "hamming")
    feats = [opencv.Features(p, d) for p, d in imgs]
    empty = opencv.Features(np.zeros((0, 2)), np.zeros((0, 32), np.uint8))
    feats2 = feats[:2] + [empty]
    ip = np.array([[0, 1], [0, 2], [2, 1], [1, 0], [2, 2]], dtype=np.int32)
    structs = (N.DetectorResult * 3)(*[f.struct for f in feats2])
    cap = 33 + 33 + 0 + 36 + 0
    pairs = np.zeros((cap, 2), np.int32)
    dist = np.zeros(cap, np.float32)
    offsets = np.full(6, -7, np.int32)
    call = lambda B, mx: N.lib().cvMatchFeaturesBatch(C.addressof(structs), 3, ip.ctypes.data, B, None, N.NORM_AUTO,
                                                      pairs.ctypes.data, dist.ctypes.data, mx, offsets.ctypes.data)
    total = call(5, cap)
    assert total > 0, N.last_error()
    a, b = (len(opencv.matchFeatures(feats[i], feats[j])[0]) for i, j in ((0, 1), (1, 0)))
    assert offsets.tolist() == [0, a, a, a, a + b, a + b] and total == a + b   # empty images: empty slices
    assert call(5, total) == total
    assert call(5, total - 1) == -1 and "maxPairs" in N.last_error()
    assert call(0, 0) == 0 and offsets[0] == 0
    out = opencv.matchFeaturesBatch(feats2, [(2, 0), (0, 2)], cross_check=True)
    assert [len(p) for p, _ in out] == [0, 0]


# ---- 8. fused ---------------------------------------------------------------------------------------
FUSED_SIZES = (129, 257, 300, 513)


@pytest.mark.parametrize("model", [N.MODEL_HOMOGRAPHY, N.MODEL_FUNDAMENTAL, N.MODEL_AFFINE, N.MODEL_SIMILARITY])
def test_fused_equals_match_then_find_model_batch(gpu, model):
    imgs = list(planted_images(FUSED_SIZES, "hamming"))
    rng = np.random.default_rng(2)
    # two images of 2 features; the train image's rows are equal, so d1 == d2 and the ratio test leaves nothing
    imgs += [(rng.uniform(0, 100, (2, 2)), rng.integers(0, 256, size=(2, 32), dtype=np.uint8)),
             (rng.uniform(0, 100, (2, 2)), np.full((2, 32), 0x5A, np.uint8))]
    feats = [opencv.Features(p, d) for p, d in imgs]
    pairs = [(8, 9), (0, 1), (2, 3), (4, 5), (7, 6)]          # pair 0: the two images of 2 features
    params = opencv.RansacParams(threshold=3.0, max_iters=500, seed=11, confidence=0.99)
    fused = opencv.matchAndFindModelBatch(feats, pairs, model=model, ratio=0.8, cross_check=True, params=params)
    err = N.last_error()
    matches = opencv.matchFeaturesBatch(feats, pairs, ratio=0.8, cross_check=True)
    srcs = [imgs[i][0][m[:, 0]].astype(np.float32).astype(np.float64) for (i, _), (m, _) in zip(pairs, matches)]
    dsts = [imgs[j][0][m[:, 1]].astype(np.float32).astype(np.float64) for (_, j), (m, _) in zip(pairs, matches)]
    ref = opencv.findModelBatch(model, srcs, dsts, params)
    for p, ((cnt, M, pr, mask), (m, _), (rc, rM, rmask)) in enumerate(zip(fused, matches, ref)):
        np.testing.assert_array_equal(pr, m)
        assert cnt == rc
        np.testing.assert_array_equal(mask, rmask)
        np.testing.assert_array_equal(M.view(np.uint64), rM.view(np.uint64))
        if p == 0:
            assert cnt == 0 and len(pr) == 0 and not M.any() and not mask.any()
        else:
            assert len(pr) >= 8       # at least the largest sample size
            if model == N.MODEL_HOMOGRAPHY:
                assert cnt >= 8
                sc, sH, smask = opencv.findHomography(srcs[p], dsts[p], params)
                assert cnt == sc
                np.testing.assert_array_equal(mask, smask)
                np.testing.assert_array_equal(M.view(np.uint64), sH.view(np.uint64))
    assert "problem 0" in err and "cvFindModelBatch" in err
