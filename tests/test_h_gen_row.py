"""The homography generate's certified one-row pass 2 (mcv_h_gen_r, jacobi_eig.h eig9_replay_row_rev, hyp_homography.h
h_model_f_cert): the reverse replay of one row of V nominates the fp32 model, a rigorous bound decides where that
model is the exact path's bit for bit, every other lane runs the exact pass 2. Every test compares against the exact
path: the same call with the pass switched off, or the host twin's exact solve.

Measured with the host twin over hypotheses [0, 65536) of the cfg3 problem (N = 100000, seed 3), as the last test
prints: bound err 8.9e-14 .. 1.4e-13, measured |y_rev - v_fwd|_inf at most 1.1e-15, largest ratio 0.0094; 65443 lanes
decided, 93 undecided (share 0.0014 against the cap 1 / 64)."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from minicv_amd import native as N, opencv, synthetic as S

SEED = 3
THR = 5e-3


def pack4(src, dst):
    return np.ascontiguousarray(np.concatenate([src, dst], axis=1).astype(np.float32))


def generate(pts4, seed, begin, count, row, table=None):
    """The split generate alone on the device -> (models (count, 8) f32, statuses (count,), (decided, undecided))."""
    models = np.zeros((count, 8), np.float32)
    status = np.zeros(count, np.int32)
    st = (C.c_longlong * 2)()
    tab = None if table is None else np.ascontiguousarray(table, np.int32)
    ok = N.lib().mcvTestHGenerate(pts4.ctypes.data, pts4.shape[0], seed, None if tab is None else tab.ctypes.data,
                                  begin, count, row, models.ctypes.data, status.ctypes.data, st)
    assert ok == 1, N.last_error()
    return models, status, (int(st[0]), int(st[1]))


def host_row(pts4, seed, begin, count, table=None, huge=False):
    """The host twin -> dict of the one-row pass's and the exact solve's per-hypothesis results."""
    out = {"row": np.zeros((count, 8), np.float32), "fwd": np.zeros((count, 8), np.float32),
           "status": np.zeros(count, np.int32), "decided": np.zeros(count, np.int32), "err": np.zeros(count),
           "dev": np.zeros(count)}
    tab = None if table is None else np.ascontiguousarray(table, np.int32)
    ok = N.lib().mcvHostHGenRow(pts4.ctypes.data, pts4.shape[0], seed, None if tab is None else tab.ctypes.data, begin,
                                count, int(huge), out["row"].ctypes.data, out["fwd"].ctypes.data,
                                out["status"].ctypes.data, out["decided"].ctypes.data, out["err"].ctypes.data,
                                out["dev"].ctypes.data)
    assert ok == 1, N.last_error()
    return out


def same_bytes(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


@contextlib.contextmanager
def row_mode(m):
    prev = N.lib().mcvTestHGenRow(int(m), None)
    assert 0 <= prev <= 3
    try:
        yield
    finally:
        N.lib().mcvTestHGenRow(prev, None)


def row_stats():
    st = (C.c_longlong * 2)()
    assert N.lib().mcvTestHGenRow(-1, st) >= 0
    return int(st[0]), int(st[1])


def hard_samples():
    """-> (pts4, table): quadruples that are hard for the certificate, one table row each."""
    rng = np.random.default_rng(11)
    H = S.H_TRUE
    quads = []

    def mapped(src, Hm=H):
        q = np.c_[src, np.ones(len(src))] @ Hm.T
        return q[:, :2] / q[:, 2:3]

    for _ in range(64):   # near-collinear: the third point 1e-6 .. 1e-3 off the line through the first two
        a, b, d = rng.uniform(-1, 1, (3, 2))
        t = rng.uniform(0.2, 0.8)
        n = np.array([-(b - a)[1], (b - a)[0]])
        c = a + t * (b - a) + rng.choice([1e-6, 1e-5, 1e-4, 1e-3]) * n
        src = np.stack([a, b, c, d])
        quads.append(np.c_[src, mapped(src)])
    for scale in (1e4, 1e-4):
        for _ in range(48):
            src = rng.uniform(-1, 1, (4, 2))
            quads.append(np.c_[src, mapped(src)] * scale)
    for _ in range(16):   # one point twice: a rank-deficient system with a model of some kind
        src = rng.uniform(-1, 1, (4, 2))
        src[1] = src[0]
        quads.append(np.c_[src, mapped(src)])
    for _ in range(16):   # one point four times: the normalisation's scales vanish, status NoModel
        src = np.repeat(rng.uniform(-1, 1, (1, 2)), 4, axis=0)
        quads.append(np.c_[src, mapped(src)])
    Hz = np.array([[1, 0, 0.3], [0, 1, -0.2], [1.0, 0.5, 0.0]])   # H22 = 0: R[8] of the solve is rounding noise
    for _ in range(64):
        src = rng.uniform(0.5, 1.5, (4, 2))
        quads.append(np.c_[src, mapped(src, Hz)])
    pts4 = np.ascontiguousarray(np.concatenate(quads).astype(np.float32))
    table = np.arange(len(pts4), dtype=np.int32).reshape(-1, 4)
    return pts4, table


@pytest.fixture(scope="module")
def torch_dev(gpu):
    import torch
    return torch, torch.device("cuda:0")


def evaluate_key(torch_dev, src, dst, count, mode):
    torch, dev = torch_dev
    from minicv_amd import device as D
    pts = D.pack_points_tensor(src, dst, dev)
    plan = D.RansacPlan(N.MODEL_HOMOGRAPHY, src.shape[0], count)
    cfg = opencv.RansacParams(threshold=THR, seed=SEED, fused_error=False).to_c()
    key = torch.zeros(2, dtype=torch.int64, device=dev)
    with row_mode(mode):
        plan.evaluate(pts, src.shape[0], cfg, 0, count, key)
        torch.cuda.synchronize()
        st = row_stats()
    out = [int(v) for v in key.cpu().numpy()]
    plan.close()
    return out, st


@pytest.mark.gpu
@pytest.mark.parametrize("n", [512, 4])
def test_bit_identity(torch_dev, n):
    """8192 hypotheses of a cfg3-shaped problem: fp32 models, statuses and the evaluate's key with the one-row pass
    are the exact pass 2's bytes."""
    src, dst, _ = S.homography_problem(n, SEED, outlier_frac=0.5 if n > 4 else 0.0)   # the one quadruple must pass
    pts4 = pack4(src, dst)
    m0, s0, _ = generate(pts4, SEED, 0, 8192, 0)
    m1, s1, (dec, und) = generate(pts4, SEED, 0, 8192, 1)
    print(f"N={n}: decided {dec}, undecided {und}")
    assert same_bytes(m1, m0) and same_bytes(s1, s0)
    # lanes pass 1 handed on: all with a model, none without a sample
    assert int((s0 == 0).sum()) <= dec + und <= int((s0 != -2).sum()) and 0 < dec <= int((s0 == 0).sum())
    k2, st2 = evaluate_key(torch_dev, src, dst, 8192, 2)
    k1, st1 = evaluate_key(torch_dev, src, dst, 8192, 1)
    assert k1 == k2 and st2 == (0, 0) and st1 == (dec, und)


@pytest.mark.gpu
def test_hard_samples(torch_dev):
    """Near-collinear, scaled by 1e4 / 1e-4, duplicated points, H22 near 0: the same bytes, and the fallback ran."""
    pts4, table = hard_samples()
    k = len(table)
    m0, s0, _ = generate(pts4, SEED, 0, k, 0, table)
    m1, s1, (dec, und) = generate(pts4, SEED, 0, k, 1, table)
    print(f"hard samples: {k} quadruples, decided {dec}, undecided {und}, NoModel {(s0 == -1).sum()}")
    assert same_bytes(m1, m0) and same_bytes(s1, s0)
    assert und > 0 and (s0 == -1).any() and (s0 == 0).any()
    tw = host_row(pts4, SEED, 0, k, table)
    assert int(tw["decided"].sum()) == dec
    d = tw["decided"] == 1
    assert same_bytes(tw["row"][d], m0[d]) and (s0[d] == 0).all()


@pytest.mark.gpu
def test_forced_fallback(torch_dev):
    """The bound times 2^40: no lane is decided, every model comes from the exact pass, the same bytes."""
    src, dst, _ = S.homography_problem(512, SEED)
    pts4 = pack4(src, dst)
    m0, s0, _ = generate(pts4, SEED, 100, 4099, 0)
    m2, s2, (dec, und) = generate(pts4, SEED, 100, 4099, 2)
    assert dec == 0 and int((s0 == 0).sum()) <= und <= int((s0 != -2).sum())
    assert same_bytes(m2, m0) and same_bytes(s2, s0)
    k2, _ = evaluate_key(torch_dev, src, dst, 4099, 2)
    k3, st3 = evaluate_key(torch_dev, src, dst, 4099, 3)
    assert k3 == k2 and st3[0] == 0 and st3[1] > 0


@pytest.mark.gpu
def test_log_overflow(torch_dev):
    """A log of 100 rows: the lanes that overflow it still end with the exact models (the one-pass kernel's)."""
    src, dst, _ = S.homography_problem(512, SEED)
    pts4 = pack4(src, dst)
    m0, s0, _ = generate(pts4, SEED, 0, 4096, 0)
    for cap in (100, 138):
        prev = N.lib().mcvTestEigLogCap(cap)
        try:
            m1, s1, (dec, und) = generate(pts4, SEED, 0, 4096, 1)
        finally:
            N.lib().mcvTestEigLogCap(prev)
        print(f"cap {cap}: decided {dec}, undecided {und}")
        assert same_bytes(m1, m0) and same_bytes(s1, s0)
        assert int((s0 == 0).sum()) <= dec + und <= int((s0 != -2).sum()) and und > 100


@pytest.mark.gpu
@pytest.mark.parametrize("refine", [False, True])
@pytest.mark.parametrize("rewrite", [False, True])
def test_finalize(torch_dev, refine, rewrite):
    """finalize after a certified evaluate: H, the mask and the count are the exact path's; with the points rewritten
    in place between evaluate and finalize, the re-solve path's."""
    torch, dev = torch_dev
    from minicv_amd import device as D
    n, count = 1500, 4096
    src, dst, _ = S.homography_problem(n, SEED)
    src2, dst2, _ = S.homography_problem(n, SEED + 1)
    cfg = opencv.RansacParams(threshold=THR, seed=SEED, fused_error=False, refine=refine).to_c()
    got = []
    for mode in (2, 1):
        pts = D.pack_points_tensor(src, dst, dev)
        plan = D.RansacPlan(N.MODEL_HOMOGRAPHY, n, count)
        key = torch.zeros(2, dtype=torch.int64, device=dev)
        mask = torch.zeros(n, dtype=torch.uint8, device=dev)
        with row_mode(mode):
            plan.evaluate(pts, n, cfg, 0, count, key)
            torch.cuda.synchronize()
            st = row_stats()
            _, hyp = D.unpack_key(int(key[0].item()))
            if rewrite:
                pts.copy_(D.pack_points_tensor(src2, dst2, dev))
            fc, M = plan.finalize(pts, n, cfg, hyp, mask)
        assert (st[0] > 0) == (mode == 1)
        got.append((hyp, fc, M.copy(), mask.cpu().numpy().copy()))
        plan.close()
    (h2, c2, M2, k2), (h1, c1, M1, k1) = got
    assert h1 == h2 and c1 == c2 and same_bytes(M1, M2) and np.array_equal(k1, k2)


def test_host_twin_cfg3():
    """65536 cfg3 hypotheses at N = 100000 on the host twin: every decided lane has the forward solve's model bits,
    the bound holds on every lane, the reverse row is the forward row to about 1e-13, and the undecided share stays
    at or below 1 / 64."""
    src, dst, _ = S.homography_problem(100000, SEED)
    pts4 = pack4(src, dst)
    k = 65536
    tw = host_row(pts4, SEED, 0, k)
    d = tw["decided"] == 1
    has = tw["status"] == 1
    ran = tw["err"] > 0
    ratio = float((tw["dev"][ran] / tw["err"][ran]).max())
    und = int((has & ~d).sum())
    print(f"decided {int(d.sum())}, undecided {und} (share {und / max(1, int(has.sum())):.5f}), err "
          f"{tw['err'][ran].min():.3e} .. {tw['err'][ran].max():.3e}, max dev {tw['dev'].max():.3e}, max dev / err "
          f"{ratio:.4f}")
    assert (tw["dev"] <= tw["err"]).all()
    assert tw["dev"].max() < 1e-13
    assert has[d].all() and same_bytes(tw["row"][d], tw["fwd"][d])
    assert und * 64 <= int(has.sum())
    # the 2^40 switch leaves nothing decided
    assert host_row(pts4, SEED, 0, 256, huge=True)["decided"].sum() == 0
