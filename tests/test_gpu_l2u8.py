"""GPU tests of the exact uint8 L2 matcher on the int8 matrix cores (match_l2u8.hip; needs an MI355X).

Every result is an exact integer computation, so every comparison is array_equal: indices, second
places and the fp32 distances bit for bit, against the oracle's L2 matcher on the bytes as float32
and / or the int64 numpy restatement (tests/_l2u8_ref.py; test_l2u8.py ties the two together). There
is no re-rank and no exact scan behind the GEMM form: a wrong operand map, a wrong K padding or a
wrong tie-break shows up as a mismatch here."""
import ctypes as C

import numpy as np
import pytest

from minicv_amd import native as N, opencv, synthetic as S

import _l2u8_ref as R

pytestmark = pytest.mark.gpu


def check(oracle, q, t, use_oracle=True):
    got = opencv.matchL2U8(q, t)
    R.assert_same(got, R.match_l2_u8(q, t))
    if use_oracle:
        R.assert_same(got, oracle.match_l2(q.astype(np.float32), t.astype(np.float32)))
    return got


# one lane / one row, train tile edges 31 / 32 / 33 (and the two-chain tile's 64), query block edges
# 127 / 129, every kind of K padding (dim 1, 17, 31, 33, 129 and the exact 32 / 64 / 128 / 256 / 512),
# more than one train chunk (4099 and 3000 rows)
@pytest.mark.parametrize("nq,nt,dim", [(1, 1, 128), (1, 2, 128), (33, 31, 128), (32, 32, 32), (127, 33, 31),
                                       (129, 4099, 128), (200, 777, 33), (100, 300, 1), (64, 200, 17),
                                       (300, 500, 64), (64, 200, 129), (64, 200, 256), (50, 100, 512),
                                       (2000, 3000, 128)])
def test_l2u8_shapes(gpu, oracle, nq, nt, dim):
    q, t = R.random_u8(nq, nt, dim, seed=nq + 3 * nt + 7 * dim)
    check(oracle, q, t)
    qs, ts, _ = S.sift_u8_problem(nq, nt, dim=dim, seed=nq + nt + dim)
    check(oracle, qs, ts)


@pytest.mark.parametrize("nq,nt,dim", [(65, 63, 128), (65, 64, 128), (65, 65, 128), (130, 257, 256)])
def test_l2u8_two_chain_tile_edges(gpu, oracle, nq, nt, dim):
    """The 64-row tile of the two-chain form: train counts around it."""
    q, t = R.random_u8(nq, nt, dim, seed=nt)
    check(oracle, q, t)


@pytest.mark.parametrize("dim", [128, 512])
def test_l2u8_extremes(gpu, oracle, dim):
    """Rows of all 0 and all 255: d^2 = dim * 255^2 (the largest distance; at dim 512 the accumulator's
    and the norms' 2^23 in the shifted domain, where 0 -> -128) and 0, with ties among them."""
    rng = np.random.default_rng(dim)
    t = rng.integers(0, 256, size=(300, dim), dtype=np.uint8)
    t[:20] = 0
    t[20:40] = 255
    t[40:50] = 128
    t[50:60] = 127
    q = np.concatenate([np.zeros((10, dim), np.uint8), np.full((10, dim), 255, np.uint8),
                        np.full((5, dim), 128, np.uint8), rng.integers(0, 256, size=(40, dim), dtype=np.uint8)])
    idx, d, idx2, d2 = check(oracle, q, t)
    assert (idx[:10] == 0).all() and (idx2[:10] == 1).all() and (d[:10] == 0).all()
    assert (idx[10:20] == 20).all() and (idx2[10:20] == 21).all()
    # every query at the maximum distance from every train row
    far = check(oracle, np.zeros((40, dim), np.uint8), np.full((5, dim), 255, np.uint8))
    assert (far[0] == 0).all() and (far[2] == 1).all()
    assert (far[1] == np.float32(np.sqrt(float(dim * 255 * 255)))).all() and (far[3] == far[1]).all()
    near = check(oracle, np.full((40, dim), 255, np.uint8), np.full((3, dim), 255, np.uint8))
    assert (near[1] == 0).all() and (near[0] == 0).all() and (near[2] == 1).all()


def test_l2u8_ties_duplicated_train_rows(gpu, oracle):
    """Duplicated train rows at known indices: idx is the lowest, idx2 the next duplicate — across lanes
    halves (rows 4 apart), tiles and train chunks."""
    rng = np.random.default_rng(1)
    base = rng.integers(0, 256, size=(700, 128), dtype=np.uint8)
    t = np.concatenate([base, base, base])
    q = base[rng.integers(0, 700, size=400)]
    idx, d, idx2, d2 = check(oracle, q, t)
    assert (d == 0).all() and (d2 == 0).all()
    assert (idx < 700).all() and (idx2 == idx + 700).all()
    # duplicates next to each other and 4 / 32 / 64 rows apart
    t2 = rng.integers(0, 256, size=(200, 128), dtype=np.uint8)
    for a, b in ((10, 11), (20, 24), (30, 62), (70, 134), (3, 199)):
        t2[b] = t2[a]
    q2 = t2[[10, 20, 30, 70, 3]]
    idx, d, idx2, d2 = check(oracle, q2, t2)
    np.testing.assert_array_equal(idx, [10, 20, 30, 70, 3])
    np.testing.assert_array_equal(idx2, [11, 24, 62, 134, 199])


@pytest.mark.parametrize("nq,nt,dim", [(200, 2000, 8), (150, 333, 8), (150, 333, 17), (300, 1000, 128)])
def test_l2u8_ties_two_valued(gpu, oracle, nq, nt, dim):
    """Values in {0, 1}: d^2 takes at most dim + 1 values. At dim 8 there are 256 distinct rows, so with
    2000 train rows every query has several exact copies (all tie at 0) and with 333 most queries tie
    for the two places; at dim 17 / 128 a good share still does. The lowest indices win."""
    q, t = R.random_u8(nq, nt, dim, seed=5, high=2)
    idx, d, idx2, d2 = check(oracle, q, t)
    tied = (d == d2).mean()                       # a property of the inputs (the reference says the same)
    assert tied > 0.5 if dim == 8 else tied > 0.1
    assert (idx < idx2)[d == d2].all()


def test_l2u8_few_train_rows(gpu, oracle):
    q, t = R.random_u8(70, 1, 128, seed=2)
    idx, d, idx2, d2 = check(oracle, q, t)
    assert (idx == 0).all() and (idx2 == -1).all() and np.isinf(d2).all()
    # no train row: every place empty, index -1 / distance +inf (what mcv_l2_refine writes for nt == 0)
    got = opencv.matchL2U8(q, np.zeros((0, 128), np.uint8))
    R.assert_same(got, R.match_l2_u8(q, np.zeros((0, 128), np.uint8)))
    assert (got[0] == -1).all() and np.isinf(got[1]).all() and (got[2] == -1).all() and np.isinf(got[3]).all()
    assert len(opencv.matchL2U8(np.zeros((0, 128), np.uint8), t)[0]) == 0


@pytest.fixture(scope="module")
def sift_medium():
    return S.sift_u8_problem(4000, 6000, seed=12)


def test_l2u8_equals_float_path_and_oracle(gpu, oracle, sift_medium):
    """sift_u8_problem(4000, 6000): the int8 kernel == the shipped float path on the widened bytes ==
    the oracle, with planted neighbours found and exact ties present."""
    q, t, planted = sift_medium
    got = check(oracle, q, t)
    R.assert_same(got, opencv.matchL2(q.astype(np.float32), t.astype(np.float32)))
    ok = planted >= 0
    assert np.mean((t[got[0][ok]] == t[planted[ok]]).all(axis=1)) > 0.99
    assert (got[1] == got[3]).any()


def test_l2u8_large_equals_float_path(gpu):
    """20000 x 33000 x 128: many query blocks and train chunks; against the float GPU path (the oracle
    would take too long), which test_gpu_matchers.py ties to the oracle."""
    q, t, _ = S.sift_u8_problem(20000, 33000, seed=13)
    got = opencv.matchL2U8(q, t)
    R.assert_same(got, opencv.matchL2(q.astype(np.float32), t.astype(np.float32)))
    pick = np.r_[0:64, 19936:20000, np.random.default_rng(0).choice(20000, 400, replace=False)]
    R.assert_same([g[pick] for g in got], R.match_l2_u8(q[pick], t))


def test_l2u8_back_to_back_on_two_streams(gpu):
    """The device entry point is asynchronous on the caller's stream and shares one workspace per
    thread and device: two calls on two streams with different inputs, issued back to back, each read
    only after its own stream's sync."""
    import torch
    from minicv_amd import device as D
    dev = torch.device("cuda:0")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    qa, ta, _ = S.sift_u8_problem(3000, 5000, seed=51)
    qb, tb, _ = S.sift_u8_problem(2000, 7000, seed=52)
    bufs = {}
    for name, (q, t) in {"a": (qa, ta), "b": (qb, tb)}.items():
        qd, td = torch.from_numpy(q).to(dev), torch.from_numpy(t).to(dev)
        bufs[name] = (qd, td, torch.empty(len(q), dtype=torch.int32, device=dev),
                      torch.empty(len(q), dtype=torch.float32, device=dev),
                      torch.empty(len(q), dtype=torch.int32, device=dev),
                      torch.empty(len(q), dtype=torch.float32, device=dev))
    torch.cuda.synchronize()
    for k in range(3):
        for name, s in (("a", s1), ("b", s2)):
            qd, td, idx, dist, idx2, dist2 = bufs[name]
            D.match_l2_u8(qd, td, idx, dist, idx2, dist2, stream=s)
    for name, s, (q, t) in (("a", s1, (qa, ta)), ("b", s2, (qb, tb))):
        s.synchronize()
        R.assert_same([x.cpu().numpy() for x in bufs[name][2:]], R.match_l2_u8(q, t))
    torch.cuda.synchronize()


def test_l2u8_sharded_equals_one(gpu, sift_medium):
    """cvMatchL2U8Multi with deviceCount 3 (every block on the one visible GPU, or spread over several)
    equals deviceCount 1 bit for bit; fewer queries than devices too."""
    q, t, _ = sift_medium
    one = opencv.matchL2U8(q[:1001], t)
    R.assert_same(opencv.matchL2U8(q[:1001], t, deviceCount=3), one)
    R.assert_same(one, R.match_l2_u8(q[:1001], t))
    R.assert_same(opencv.matchL2U8(q[:2], t, deviceCount=5), [o[:2] for o in one])
    with pytest.raises(N.NativeError, match="deviceCount"):
        opencv.matchL2U8(q[:10], t, deviceCount=17)


# ---- pipeline: cvMatchFeaturesNorm / cvMatchAndFindModelNorm ---------------------------------------

@pytest.fixture(scope="module")
def pair_u8():
    return S.feature_pair_problem(3000, 3500, seed=31, kind="sift_u8", match_frac=0.6)


@pytest.mark.parametrize("ratio,cross,maxd", [(0.8, False, 0.0), (0.0, False, 0.0), (0.75, True, 0.0),
                                              (0.0, True, 60.0), (0.9, False, 40.0)])
def test_match_features_u8_l2_equals_float(gpu, pair_u8, ratio, cross, maxd):
    pa, da, pb, db, planted = pair_u8
    A8, B8 = opencv.Features(pa, da), opencv.Features(pb, db)
    Af, Bf = opencv.Features(pa, da.astype(np.float32)), opencv.Features(pb, db.astype(np.float32))
    p8, d8 = opencv.matchFeatures(A8, B8, ratio=ratio, cross_check=cross, max_distance=maxd, norm=N.NORM_L2)
    pf, df = opencv.matchFeatures(Af, Bf, ratio=ratio, cross_check=cross, max_distance=maxd)
    np.testing.assert_array_equal(p8, pf)
    np.testing.assert_array_equal(d8.view(np.uint32), df.view(np.uint32))
    pl, dl = opencv.matchFeatures(Af, Bf, ratio=ratio, cross_check=cross, max_distance=maxd, norm=N.NORM_L2)
    np.testing.assert_array_equal(pl, pf)
    assert len(p8) > 100
    # the stated filters on the reference matcher's output
    idx, d1, idx2, d2 = R.match_l2_u8(da, db)
    keep = idx >= 0
    if ratio > 0:
        keep &= d1 < np.float32(ratio) * d2
    if maxd > 0:
        keep &= d1 <= np.float32(maxd)
    if cross:
        keep &= R.match_l2_u8(db, da)[0][np.maximum(idx, 0)] == np.arange(len(idx))
    qs = np.nonzero(keep)[0]
    np.testing.assert_array_equal(p8, np.stack([qs, idx[qs]], axis=1).astype(np.int32))
    np.testing.assert_array_equal(d8, d1[qs])


@pytest.mark.parametrize("model", [N.MODEL_HOMOGRAPHY, N.MODEL_FUNDAMENTAL])
def test_match_and_find_model_u8_l2_equals_float(gpu, pair_u8, model):
    pa, da, pb, db, planted = pair_u8
    A8, B8 = opencv.Features(pa, da), opencv.Features(pb, db)
    Af, Bf = opencv.Features(pa, da.astype(np.float32)), opencv.Features(pb, db.astype(np.float32))
    p = opencv.RansacParams(threshold=3.0, confidence=0.99, max_iters=1000, seed=7)
    c8, M8, pr8, m8 = opencv.matchAndFindModel(A8, B8, model=model, ratio=0.8, cross_check=True, params=p,
                                               norm=N.NORM_L2)
    cf, Mf, prf, mf = opencv.matchAndFindModel(Af, Bf, model=model, ratio=0.8, cross_check=True, params=p)
    assert c8 == cf
    np.testing.assert_array_equal(M8, Mf)
    np.testing.assert_array_equal(pr8, prf)
    np.testing.assert_array_equal(m8, mf)
    if model == N.MODEL_HOMOGRAPHY:
        err = np.linalg.norm(S.project(M8, pa) - S.project(S.H_PIX, pa), axis=1)
        assert np.median(err) < 0.5


def _old_match_features(A, B, ratio, cross, maxd):
    """The cvMatchFeatures export itself (no norm argument)."""
    n = A.struct.PointCount
    pairs = np.zeros((max(n, 1), 2), dtype=np.int32)
    dist = np.zeros(max(n, 1), dtype=np.float32)
    cfg = N.MatchConfig(float(ratio), int(cross), float(maxd), N.MODEL_HOMOGRAPHY)
    k = N.lib().cvMatchFeatures(C.addressof(A.struct), C.addressof(B.struct), C.addressof(cfg), pairs.ctypes.data,
                                dist.ctypes.data, max(n, 1))
    N.check(k >= 0, "cvMatchFeatures")
    return pairs[:k].copy(), dist[:k].copy()


def test_auto_and_hamming_on_bytes_unchanged(gpu, oracle):
    """norm AUTO and HAMMING on uint8 rows are cvMatchFeatures' Hamming matching, pair for pair; AUTO on
    byte SIFT rows is still Hamming (not L2): the caller has to ask for L2."""
    pa, da, pb, db, _ = S.feature_pair_problem(1500, 1800, seed=33)
    A, B = opencv.Features(pa, da), opencv.Features(pb, db)
    old = _old_match_features(A, B, 0.8, True, 0.0)
    for norm in (N.NORM_AUTO, N.NORM_HAMMING):
        got = opencv.matchFeatures(A, B, ratio=0.8, cross_check=True, norm=norm)
        np.testing.assert_array_equal(got[0], old[0])
        np.testing.assert_array_equal(got[1], old[1])
    idx, d1, idx2, d2 = oracle.match_hamming(da, db)
    assert np.array_equal(old[1], d1[old[0][:, 0]].astype(np.float32))
    ds, dbs, _ = S.sift_u8_problem(400, 500, dim=64, seed=34)      # 64 bytes: the Hamming matcher's widest row
    rng = np.random.default_rng(34)
    ps, pbs = rng.uniform(0, 640, size=(400, 2)), rng.uniform(0, 640, size=(500, 2))
    As, Bs = opencv.Features(ps, ds), opencv.Features(pbs, dbs)
    auto = opencv.matchFeatures(As, Bs, ratio=0.0, norm=N.NORM_AUTO)
    np.testing.assert_array_equal(auto[1], oracle.match_hamming(ds, dbs)[1].astype(np.float32))
    l2 = opencv.matchFeatures(As, Bs, ratio=0.0, norm=N.NORM_L2)
    np.testing.assert_array_equal(l2[1], R.match_l2_u8(ds, dbs)[1])
    with pytest.raises(N.NativeError, match="MCV_NORM_HAMMING needs uint8"):
        opencv.matchFeatures(opencv.Features(ps, ds.astype(np.float32)), opencv.Features(pbs, dbs.astype(np.float32)),
                             norm=N.NORM_HAMMING)
