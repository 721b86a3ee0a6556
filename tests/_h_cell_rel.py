"""Shared helpers of the tests of the per-cell bound's second pass (test_h_cell_rel.py, test_gpu_h_cell_rel.py):
the hook mcvTestHCellRel (device kernels or host twin), the brute-force `left` and the soundness check."""
import ctypes as C

import numpy as np

import _h_cell as HC


def run(L, pts4, cand, models, thr2, B, bounds, G=4, Gs=12, device=0):
    """-> dict: cell (N,), ub (K,), cert (K, cells) bool of the union test, bits, left (len(bounds), K), alive."""
    pts4 = np.ascontiguousarray(pts4, np.float32)
    models = np.ascontiguousarray(models, np.float32).reshape(-1, 8)
    cand = np.ascontiguousarray(cand, np.float32)
    bounds = np.ascontiguousarray(bounds, np.int32)
    n, k, nc, nb = pts4.shape[0], models.shape[0], HC.cells(G, Gs), len(bounds)
    words = (nc + 31) // 32
    cell = np.full(n, -1, np.int32)
    ub = np.zeros(k, np.int32)
    bits = np.zeros((k, words), np.uint32)
    left = np.full((nb, k), -1, np.int32)
    alive = C.c_int(-1)
    ok = L.mcvTestHCellRel(pts4.ctypes.data, n, cand.ctypes.data, models.ctypes.data, k, np.float32(thr2), int(B), G, Gs,
                           bounds.ctypes.data, nb, int(device), cell.ctypes.data, ub.ctypes.data, bits.ctypes.data,
                           left.ctypes.data, C.addressof(alive))
    assert ok == 1
    cert = ((bits[:, np.arange(nc) >> 5] >> (np.arange(nc) & 31).astype(np.uint32)) & 1).astype(bool)
    return {"cell": cell, "ub": ub, "cert": cert, "bits": bits, "left": left, "alive": int(alive.value),
            "sizes": np.bincount(cell, minlength=nc).astype(np.int32), "limits": np.minimum(2 * bounds.astype(np.int64), n)}


def boundaries(n):
    """Four boundaries in pairs: the start, two inside (one of them odd in points' terms), the end."""
    return np.array([0, n // 16, n // 3 // 2, (n + 1) // 2], np.int32)


def brute_left(out):
    """left from the cell ids and the bitmaps: the points at or after each limit whose cell is not certified."""
    open_at_point = ~out["cert"][:, out["cell"]]                     # (K, N)
    return np.stack([open_at_point[:, lim:].sum(1) for lim in out["limits"]]).astype(np.int32)


def check_left(out):
    np.testing.assert_array_equal(out["left"], brute_left(out))
    order = np.argsort(out["limits"], kind="stable")
    assert (np.diff(out["left"][order], axis=0) <= 0).all()          # non-increasing over the boundaries
    n = len(out["cell"])
    for j, lim in enumerate(out["limits"]):
        if lim == 0:
            np.testing.assert_array_equal(out["left"][j], out["ub"])
        if lim == n:
            assert (out["left"][j] == 0).all()


def check_sound(oracle, pts4, models, thr2, out):
    """No inlier of the oracle's op-by-op mask inside a certified cell; UB >= count; count(p) + left(p) >= count
    at every boundary. -> (counts, masks)"""
    cnt, m = HC.masks(oracle, pts4, models, thr2)
    bad = out["cert"][:, out["cell"]] & m
    assert not bad.any(), f"{int(bad.sum())} inliers inside certified cells (models {np.nonzero(bad.any(1))[0][:5]})"
    assert (out["cert"][:, out["sizes"] == 0] == 0).all()
    np.testing.assert_array_equal(out["ub"], (out["sizes"][None, :] * ~out["cert"]).sum(1))
    assert (out["ub"] >= cnt).all()
    for j, lim in enumerate(out["limits"]):
        assert (m[:, :lim].sum(1) + out["left"][j] >= cnt).all()
    return cnt, m
