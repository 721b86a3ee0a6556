"""Pass 1 of the homography generate (mcv_h_gen_aw, jacobi_eig.h eig9_rotations_lane): the lane-slice rotation loop
keeps its trackers as byte offsets, carries the pivot's address through the pivot tree and rescans on magnitudes.
Its pivot sequence, and with it every model and status, must stay the generic loop's, which the host twin still runs:
every test compares the device's bytes with the host twin's exact solve.

Lattice quadruples are the inputs on which a tie-break or a tracker can go wrong: with small integer coordinates the
LtL holds many elements of equal magnitude, so the pivot tree and the rescans meet genuine ties."""
import ctypes as C

import numpy as np
import pytest

from minicv_amd import native as N, synthetic as S

SEED = 3
LATTICE_ROWS = 4096
# the eight symmetries of the square lattice
SYMMETRIES = np.array([[[1, 0], [0, 1]], [[0, -1], [1, 0]], [[-1, 0], [0, -1]], [[0, 1], [-1, 0]],
                       [[1, 0], [0, -1]], [[-1, 0], [0, 1]], [[0, 1], [1, 0]], [[0, -1], [-1, 0]]], np.int64)
# block edges of pass 1 (64 lanes per block; 56 before): one lane, a block short of, at and past full, two blocks
# and one lane, many blocks
EDGE_COUNTS = [1, 55, 56, 57, 63, 64, 65, 2 * 64 + 1, 8192]


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


def host_exact(pts4, seed, begin, count, table=None):
    """The host twin's exact solve -> (models (count, 8) f32, zero without a model; h_hypothesis's statuses)."""
    row, fwd = np.zeros((count, 8), np.float32), np.zeros((count, 8), np.float32)
    status, decided = np.zeros(count, np.int32), np.zeros(count, np.int32)
    err, dev = np.zeros(count), np.zeros(count)
    tab = None if table is None else np.ascontiguousarray(table, np.int32)
    ok = N.lib().mcvHostHGenRow(pts4.ctypes.data, pts4.shape[0], seed, None if tab is None else tab.ctypes.data, begin,
                                count, 0, row.ctypes.data, fwd.ctypes.data, status.ctypes.data, decided.ctypes.data,
                                err.ctypes.data, dev.ctypes.data)
    assert ok == 1, N.last_error()
    return fwd, status


def same_bytes(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def lattice_quadruples():
    """-> (pts4, table): LATTICE_ROWS quadruples, four source points with integer coordinates in [-3, 3] (distinct, no
    three on a line), the destination their image under a lattice symmetry, an integer scale 1..3 and an integer
    translation in [-3, 3]."""
    rng = np.random.default_rng(20240611)
    quads = np.zeros((0, 4, 2), np.int64)
    while len(quads) < LATTICE_ROWS:
        q = rng.integers(-3, 4, (4 * LATTICE_ROWS, 4, 2))
        ok = np.ones(len(q), bool)
        for a, b, c in ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)):
            u, v = q[:, b] - q[:, a], q[:, c] - q[:, a]
            ok &= (u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]) != 0   # also drops coincident points
        quads = np.concatenate([quads, q[ok]])
    src = quads[:LATTICE_ROWS]
    sym = SYMMETRIES[rng.integers(0, 8, LATTICE_ROWS)]
    scale = rng.integers(1, 4, LATTICE_ROWS)
    shift = rng.integers(-3, 4, (LATTICE_ROWS, 1, 2))
    dst = np.einsum("qij,qpj->qpi", sym, src) * scale[:, None, None] + shift
    pts4 = np.ascontiguousarray(np.concatenate([src, dst], axis=2).reshape(-1, 4).astype(np.float32))
    table = np.arange(len(pts4), dtype=np.int32).reshape(-1, 4)
    return pts4, table


def device_status(host_status):
    """The generate's status word for the host twin's: 0 with a model, the failure code otherwise."""
    return np.where(host_status == 1, 0, host_status).astype(np.int32)


@pytest.fixture(scope="module")
def lattice(gpu):
    pts4, table = lattice_quadruples()
    return pts4, table, host_exact(pts4, SEED, 0, len(table), table)


@pytest.fixture(scope="module")
def stream(gpu):
    src, dst, _ = S.homography_problem(512, SEED)
    pts4 = pack4(src, dst)
    return pts4, host_exact(pts4, SEED, 0, max(EDGE_COUNTS))


@pytest.mark.gpu
@pytest.mark.parametrize("row", [0, 1])
def test_lattice_ties(lattice, row):
    """4096 lattice quadruples: models and statuses are the host twin's bytes, with the exact and the one-row pass 2."""
    pts4, table, (fwd, status) = lattice
    has = status == 1
    print(f"lattice: {int(has.sum())} of {len(table)} quadruples with a model")
    assert has.sum() * 10 >= 9 * len(table)   # otherwise the test would compare failures
    m, s, _ = generate(pts4, SEED, 0, len(table), row, table)
    assert same_bytes(s, device_status(status))
    assert same_bytes(m, fwd)


@pytest.mark.gpu
@pytest.mark.parametrize("count", EDGE_COUNTS)
def test_block_edges(stream, count):
    """The seeded sample stream at N = 512 with the last block of pass 1 full, one lane short and one lane over."""
    pts4, (fwd, status) = stream
    for row in (0, 1):
        m, s, _ = generate(pts4, SEED, 0, count, row)
        assert same_bytes(s, device_status(status[:count]))
        assert same_bytes(m, fwd[:count])


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [100, 0])
def test_overflow_with_ties(lattice, cap):
    """The lattice set with a log of 100 rows and of none: the lanes handed to the one-pass kernel end with the same
    bytes as with the full log."""
    pts4, table, (fwd, status) = lattice
    m0, s0, _ = generate(pts4, SEED, 0, len(table), 1, table)
    prev = N.lib().mcvTestEigLogCap(cap)
    try:
        m1, s1, (dec, und) = generate(pts4, SEED, 0, len(table), 1, table)
    finally:
        N.lib().mcvTestEigLogCap(prev)
    print(f"cap {cap}: decided {dec}, undecided {und}")
    assert same_bytes(m1, m0) and same_bytes(s1, s0)
    assert same_bytes(m1, fwd) and same_bytes(s1, device_status(status))
