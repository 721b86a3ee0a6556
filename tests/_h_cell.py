"""Shared helpers of the per-cell bound's tests (test_h_cell_bound.py, test_gpu_h_cell_bound.py): the hook
mcvTestHCellBound (device kernels or host twin), oracle hypotheses and masks, and the soundness check."""
import ctypes as C

import numpy as np


def cells(G=4, Gs=12):
    return G ** 4 + Gs * Gs


def run(L, pts4, cand, models, thr2, B, G=4, Gs=12, device=0):
    """-> dict: cell (N,), boxes (cells, 8), sizes (cells,), ub (K,), cert (K, cells) bool, alive."""
    pts4 = np.ascontiguousarray(pts4, np.float32)
    models = np.ascontiguousarray(models, np.float32).reshape(-1, 8)
    cand = np.ascontiguousarray(cand, np.float32)
    n, k, nc = pts4.shape[0], models.shape[0], cells(G, Gs)
    words = (nc + 31) // 32
    cell = np.full(n, -1, np.int32)
    boxes = np.zeros((nc, 8), np.float32)
    sizes = np.zeros(nc, np.int32)
    ub = np.zeros(k, np.int32)
    bits = np.zeros((k, words), np.uint32)
    alive = C.c_int(-1)
    ok = L.mcvTestHCellBound(pts4.ctypes.data, n, cand.ctypes.data, models.ctypes.data, k, np.float32(thr2), int(B),
                             G, Gs, int(device), cell.ctypes.data, boxes.ctypes.data, sizes.ctypes.data,
                             ub.ctypes.data, bits.ctypes.data, C.addressof(alive))
    assert ok == 1
    cert = ((bits[:, np.arange(nc) >> 5] >> (np.arange(nc) & 31).astype(np.uint32)) & 1).astype(bool)
    return {"cell": cell, "boxes": boxes, "sizes": sizes, "ub": ub, "cert": cert, "bits": bits,
            "alive": int(alive.value)}


def oracle_models(oracle, pts4, seed, count):
    """The fp32 models of the oracle's hypotheses [0, count) that have one: (K, 8) float32."""
    out = []
    for h in range(count):
        st, _, hf, _ = oracle.h_hypothesis(pts4, seed, h)
        if st >= 0:
            out.append(hf.copy())
    return np.array(out, np.float32).reshape(-1, 8)


def masks(oracle, pts4, models, thr2):
    """-> counts (K,), inlier masks (K, N) bool of the oracle's op-by-op error."""
    cnt = np.zeros(len(models), np.int64)
    m = np.zeros((len(models), pts4.shape[0]), bool)
    for k, hf in enumerate(models):
        c, mk = oracle.h_count(pts4, hf, np.float32(thr2), want_mask=True)
        cnt[k], m[k] = c, mk.astype(bool)
    return cnt, m


def check_table(pts4, out, G=4, Gs=12):
    """The cell table is the partition's: ids in range, sizes and boxes from the points themselves."""
    nc = cells(G, Gs)
    cell = out["cell"]
    assert cell.min() >= 0 and cell.max() < nc
    np.testing.assert_array_equal(np.bincount(cell, minlength=nc), out["sizes"])
    for c in np.nonzero(out["sizes"])[0]:
        p = pts4[cell == c]
        if np.isfinite(p).all():
            want = np.stack([p.min(0), p.max(0)], 1).ravel()   # xmin xmax ymin ymax x'min ...
            np.testing.assert_array_equal(out["boxes"][c], want)


def check_sound(oracle, pts4, models, thr2, out):
    """Every certified (model, cell) holds no inlier of the oracle's mask; UB >= the oracle's count.
    -> (counts, masks)"""
    cnt, m = masks(oracle, pts4, models, thr2)
    cert_at_point = out["cert"][:, out["cell"]]            # (K, N): the point's cell is certified for the model
    bad = cert_at_point & m
    assert not bad.any(), f"{int(bad.sum())} inliers inside certified cells (models {np.nonzero(bad.any(1))[0][:5]})"
    assert (out["cert"][:, out["sizes"] == 0] == 0).all()   # empty cells are never marked
    want_ub = (out["sizes"][None, :] * ~out["cert"]).sum(1)
    np.testing.assert_array_equal(out["ub"], want_ub)
    assert (out["ub"] >= cnt).all()
    return cnt, m
