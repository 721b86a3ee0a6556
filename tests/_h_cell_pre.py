"""Shared helpers of the box test's fp32 prefilter tests (test_h_cell_pre.py, test_gpu_h_cell_pre.py): the hooks
mcvTestHCellPre (switch, counters) and mcvTestHCellPreVerdicts (three-way verdicts, device kernel or host twin)."""
import contextlib
import ctypes as C

import numpy as np

import _h_cell as HC

NOT, CERT, UNDECIDED = 0, 1, 2


@contextlib.contextmanager
def mode(L, m):
    """The prefilter's switch for the block: 0 on, 1 off (fp64 alone)."""
    prev = L.mcvTestHCellPre(int(m), None)
    assert prev in (0, 1)
    try:
        yield
    finally:
        L.mcvTestHCellPre(prev, None)


def stats(L):
    """-> (decided, undecided) of the calling thread's last bound pass or hook call."""
    st = (C.c_longlong * 2)()
    assert L.mcvTestHCellPre(-1, st) >= 0
    return int(st[0]), int(st[1])


def verdicts(L, pts4, cand, models, thr2, G=4, Gs=12, device=0):
    """-> dict: cell (N,), boxes (cells, 8), sizes (cells,), verdict (K, cells) uint8."""
    pts4 = np.ascontiguousarray(pts4, np.float32)
    models = np.ascontiguousarray(models, np.float32).reshape(-1, 8)
    cand = np.ascontiguousarray(cand, np.float32)
    n, k, nc = pts4.shape[0], models.shape[0], HC.cells(G, Gs)
    cell = np.full(n, -1, np.int32)
    boxes = np.zeros((nc, 8), np.float32)
    sizes = np.zeros(nc, np.int32)
    out = np.full((k, nc), 255, np.uint8)
    ok = L.mcvTestHCellPreVerdicts(pts4.ctypes.data, n, cand.ctypes.data, models.ctypes.data, k, np.float32(thr2), 0,
                                   G, Gs, int(device), cell.ctypes.data, boxes.ctypes.data, sizes.ctypes.data,
                                   out.ctypes.data)
    assert ok == 1
    assert out.max() <= UNDECIDED
    return {"cell": cell, "boxes": boxes, "sizes": sizes, "verdict": out}


def check_sound(v, twin):
    """Every decided verdict is the fp64 twin's bit; nothing is certified in an empty cell. -> the non-empty mask."""
    full = twin["sizes"] > 0
    np.testing.assert_array_equal(v["sizes"], twin["sizes"])
    ver, cert = v["verdict"], twin["cert"]
    assert not (ver[:, ~full] == CERT).any()
    bad = (ver != UNDECIDED) & (ver.astype(bool) != cert) & full[None, :]
    assert not bad.any(), f"{int(bad.sum())} decided verdicts differ from fp64 (first {np.argwhere(bad)[:5].tolist()})"
    assert not ((ver == CERT) & ~cert).any()
    return full


def crafted_models(rng, H):
    """Models whose vanishing line w = 0 crosses the point set [-1, 1]^2, grazes it or lies far outside; affine
    ones; huge, tiny and non-finite coefficients."""
    out = []
    base = (H / H[2, 2]).ravel()[:8]
    for _ in range(60):
        h = base * (1 + 0.05 * rng.standard_normal(8))
        a = rng.uniform(0, 2 * np.pi)
        r = rng.choice([0.5, 1.0, 1.2, 1.4, 1.5, 2.0, 5.0, 40.0])   # 1 / distance of the line from the origin
        h[6], h[7] = r * np.cos(a), r * np.sin(a)
        out.append(h)
    for s in (1e-20, 1e-6, 1e6, 1e20, 1e35):
        out.append(base * s)
        h = base.copy()
        h[6:] *= s
        out.append(h)
    out += [np.zeros(8), np.array([1, 0, 0, 0, 1, 0, 0, 0], float), np.array([1, 0, 0, 0, 1, 0, -1, 0], float),
            np.array([np.nan, 0, 0, 0, 1, 0, 0, 0], float), np.array([1, 0, 0, 0, 1, 0, np.inf, 0], float)]
    return np.array(out, np.float32)
