"""Inputs of the matcher branch tests (test_matcher_cases.py checks them on the CPU, with the oracle
and numpy only; test_gpu_matcher_branches.py runs the kernels on them), and the predicates that are
computed from the reference alone.

Every builder is deterministic and cached: the CPU test and the GPU test of one case see the same
arrays (read-only), and the oracle's answer for a case is computed once per process."""
import functools

import numpy as np

from minicv_amd import synthetic as S

NBASE = 64            # distinct rows of a triples train set (nt = 3 NBASE = 192)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---- Hamming ---------------------------------------------------------------------------------------

def steps2(nq, nt):
    """The quantity launch_match_hamming compares with 8192 to choose one or two query tiles per wave.
    Restated here only to show that the inputs were sized for the branch; the GPU tests assert
    mcvHammingLastQueryTiles(), which is the proof."""
    return -(-nq // 256) * -(-nt // 32)


# name -> (nq, nt, bytes per descriptor)
HAMMING = {
    "H1": (70, 262177, 64),       # one query block over ~340 segments, last tile of 1 row
    "H2": (2305, 26250, 64),      # 10 query blocks, the last holding 1 query; nt % 32 == 10
    "H3": (2305, 26250, 61),      # H2 through the repack
    "H4": (40, 2100001, 64),      # more than 128 tiles per range at 2 blocks per CU: the range cap binds
    "H5": (40, (1 << 22) - 1, 32),   # nt at the key's index-field limit
}
HAMMING_ALIGN = [(300, 1000, 32), (300, 1000, 64)]   # H7: one query tile per wave, both widths


def flip_bits(row, bits):
    r = row.copy()
    for b in bits:
        r[b // 8] ^= np.uint8(1 << (b % 8))
    return r


@functools.lru_cache(maxsize=None)
def hamming_case(name):
    nq, nt, nbytes = HAMMING[name]
    q, t, _ = S.hamming_problem(nq, nt, nbytes=nbytes, seed=sum(map(ord, name)) + nq + nt)
    if name == "H5":
        # neighbours at the last two rows and at row 0: r at nt - 1, r with one bit flipped at nt - 2,
        # r with two other bits flipped at 0; the first three queries are those rows
        r = t[nt - 1].copy()
        t[nt - 2] = flip_bits(r, [7])
        t[0] = flip_bits(r, [100, 201])
        q[0], q[1], q[2] = r, t[nt - 2], t[0]
    else:
        # the last query's only near neighbour is the last train row (3 bits away): a row past nt that
        # the last tile failed to mask would repeat it and take the second place
        q[nq - 1] = flip_bits(t[nt - 1], [0, 9 * nbytes // 2, 8 * nbytes - 1])
    return _frozen(q, t)


def hamming_plants(t, nq):
    """Copies of chosen rows at chosen indices of t (in place): the first tile, the second tile, a
    middle tile, the first row of the last partial tile and the last rows, plus all-zero and all-one
    rows. The planted rows come back as queries (repeated cyclically up to nq), so by construction
    dist == 0, idx is the lowest copy and idx2 the next one (dist2 == 0). One more row sits at the last
    index alone, its only neighbour a copy with one bit flipped in a middle tile: idx = nt - 1 at
    distance 0 and idx2 that copy at distance 1 (a row past nt that the last tile failed to mask would
    repeat row nt - 1 and take the second place).
    -> q, idx, dist, idx2, dist2 (the expected answers)."""
    nt, nbytes = t.shape
    assert nt >= 256
    last = (nt - 1) // 32 * 32            # first row of the last (partial) tile
    mid = nt // 2 // 32 * 32 + 3
    assert last + 1 < nt - 2
    rng = np.random.default_rng(nt)
    row = lambda: rng.integers(0, 256, nbytes, dtype=np.uint8)
    groups = [
        (row(), [5, mid, nt - 3]),            # first tile, a middle one, the last
        (row(), [37, 38]),                    # neighbours in one tile
        (row(), [41, 45]),                    # 4 apart: the two lane halves
        (row(), [last, last + 1]),            # the last (partial) tile
        (row(), [31, 32]),                    # across a tile edge
        (row(), [mid + 1, nt - 2]),           # a middle tile and the last
        (np.zeros(nbytes, np.uint8), [1, nt // 3]),
        (np.full(nbytes, 255, np.uint8), [2, 2 * nt // 3]),
    ]
    alone = row()
    used = [i for _, rows in groups for i in rows] + [nt - 1, mid + 2]
    assert len(set(used)) == len(used) and max(used) < nt
    for r, rows in groups:
        t[rows] = r
    t[nt - 1] = alone
    t[mid + 2] = flip_bits(alone, [3])
    groups.append((alone, [nt - 1, mid + 2]))
    k = np.arange(nq) % len(groups)
    q = np.stack([groups[i][0] for i in k])
    idx = np.array([groups[i][1][0] for i in k], np.int32)
    idx2 = np.array([groups[i][1][1] for i in k], np.int32)
    dist = np.zeros(nq, np.int32)
    dist2 = (k == len(groups) - 1).astype(np.int32)
    return q, idx, dist, idx2, dist2


@functools.lru_cache(maxsize=None)
def hamming_plants_case():
    """H6: hamming_plants on a random train set of H2's shape, and the saturated pair: every train row
    all ones, the queries alternately all zeros (distance 8 * bytes from every row) and all ones
    (distance 0 from every row), so every place is a tie that the lowest indices 0 and 1 win."""
    nq, nt, nbytes = HAMMING["H2"]
    t = np.random.default_rng(6).integers(0, 256, size=(nt, nbytes), dtype=np.uint8)
    q, idx, dist, idx2, dist2 = hamming_plants(t, nq)
    tsat = np.full((nt, nbytes), 255, np.uint8)
    qsat = np.where((np.arange(nq) % 2 == 0)[:, None], np.uint8(0), np.uint8(255)) * np.ones((1, nbytes), np.uint8)
    return _frozen(q, t, idx, dist, idx2, dist2, qsat.astype(np.uint8), tsat)


# ---- float L2 --------------------------------------------------------------------------------------

def triples(base, nq, noise, rng):
    """Train set = three bit-identical copies of base, each query = a base row plus noise: every query
    has d1 == d2 == d3 exactly, which no sound certificate can separate (approx3 - tol <= d3^2 = e2), so
    every query must be queued for the exact scan; the lowest-index rule gives idx2 == idx + len(base)."""
    base = np.ascontiguousarray(base, dtype=np.float32)
    t = np.concatenate([base, base, base])
    pick = rng.integers(0, len(base), size=nq)
    q = (base[pick].astype(np.float64) + rng.normal(scale=noise, size=(nq, base.shape[1]))).astype(np.float32)
    return q, t


def near_tie_clusters(dim, offset, scale, nbase=200, nq=700, copies=6, seed=29):
    """test_l2_exact_scan_filter_near_threshold's construction for any dim: `copies` perturbed copies
    (1e-3) of each base row (values up to offset + 255, all times scale), queries = base rows + 2e-3.
    Every fifth base row carries exact triples instead: its copies 0-2 are one bit-identical row and
    its copies 3-5 another, so whatever order the two land in, the three nearest rows of a query drawn
    from it contain an exact tie for the second place (d2 == d3) and the query must be queued whatever
    the GEMM form rounds to. Query k is drawn from base row k % nbase: exactly one fifth of the
    queries (nq a multiple of nbase / 2)."""
    assert copies == 6
    rng = np.random.default_rng(seed + dim)
    base = S.sift_like(nbase, dim, rng).astype(np.float64) + offset
    pert = [rng.normal(scale=1e-3, size=base.shape) for _ in range(copies)]
    tri = np.arange(nbase) % 5 == 0
    for c in (1, 2):
        pert[c][tri] = pert[0][tri]
    for c in (4, 5):
        pert[c][tri] = pert[3][tri]
    t = (np.concatenate([base + p for p in pert]) * scale).astype(np.float32)
    pick = np.arange(nq) % nbase
    q = ((base[pick] + rng.normal(scale=2e-3, size=(nq, dim))) * scale).astype(np.float32)
    return q, t


def exact_d2(q, t):
    """[nq][nt] squared distances as the oracle defines them: fp64 differences of the fp32 values,
    squared and added in dimension order (no fused multiply-add), so bit for bit the oracle's sums."""
    q64, t64 = np.asarray(q, np.float32).astype(np.float64), np.asarray(t, np.float32).astype(np.float64)
    tT = np.ascontiguousarray(t64.T)
    d = np.zeros((q64.shape[0], t64.shape[0]))
    e = np.empty_like(d)
    for k in range(q64.shape[1]):
        np.subtract(q64[:, k, None], tT[k][None, :], out=e)
        np.multiply(e, e, out=e)
        d += e
    return d


def smallest3(q, t, block=128):
    """The three smallest exact d^2 per query, ascending ([nq][3]); nt >= 3."""
    out = np.empty((len(q), 3))
    for b in range(0, len(q), block):
        d = exact_d2(q[b:b + block], t)
        out[b:b + block] = np.sort(np.partition(d, 2, axis=1)[:, :3], axis=1)
    return out


def must_queue(q, t):
    """Lower bound of the exact-scan queue, from the reference alone: the queries whose exact third-
    smallest d^2 is <= d2^2 (1 + 1e-12). A query that mcv_l2_refine certifies has every row other than
    its two candidates strictly above e2 (1 + 1e-12) >= d2^2 (1 + 1e-12) (a sound certificate: every
    such row's exact d^2 >= approx3 - tol), so its third-smallest d^2 is above that too; a query counted
    here can therefore not be certified."""
    s = smallest3(q, t)
    return int(np.count_nonzero(s[:, 2] <= s[:, 1] * (1.0 + 1e-12)))


def f32_norm_inf_share(t):
    """Share of the rows whose fp32 squared norm (fp32 running sum in dimension order) is +inf."""
    t = np.asarray(t, np.float32)
    acc = np.zeros(len(t), np.float32)
    with np.errstate(over="ignore"):
        for k in range(t.shape[1]):
            acc = acc + t[:, k] * t[:, k]
    return float(np.isinf(acc).mean())


# Triples cases: id -> (nq, dim, scale, dom, chunks). dom = what mcvL2LastGemmForm() must return (16
# needs dim <= 128 and max |x| < 2^15); chunks = 1 where the case is sized for the scan's T == 1 branch,
# None where the test computes T from the queue length.
TRIPLES = {
    "L1-32": (8500, 32, 1.0, 16, 1), "L1-61": (8500, 61, 1.0, 16, 1), "L1-128": (8500, 128, 1.0, 16, 1),
    "L2-17": (4300, 17, 1e4, 32, 1), "L2-32": (4300, 32, 1e4, 32, 1), "L2-64": (4300, 64, 1e4, 32, 1),
    "L3-129": (4300, 129, 1.0, 32, 1), "L3-200": (4300, 200, 1.0, 32, 1), "L3-256": (4300, 256, 1.0, 32, 1),
    "L4-40x32": (40, 32, 1.0, 16, None), "L4-40x200": (40, 200, 1.0, 32, None),
    "L4-2100x32": (2100, 32, 1.0, 16, None), "L4-6000x32": (6000, 32, 1.0, 16, None),
}


@functools.lru_cache(maxsize=None)
def triples_case(name):
    nq, dim, scale, _, _ = TRIPLES[name]
    rng = np.random.default_rng(1000 + nq + dim)
    base = (S.sift_like(NBASE, dim, rng).astype(np.float64) * scale).astype(np.float32)
    return _frozen(*triples(base, nq, 0.3 * scale, rng))


# L8: triples of normal * 3e18 (50 distinct rows, nt = 150). id -> (nq, dim)
OVERFLOW = {"L8-32": (200, 32), "L8-200": (200, 200)}
OVERFLOW_NBASE = 50


@functools.lru_cache(maxsize=None)
def overflow_case(name):
    nq, dim = OVERFLOW[name]
    rng = np.random.default_rng(80 + dim)
    base = (rng.normal(size=(OVERFLOW_NBASE, dim)) * 3e18).astype(np.float32)
    return _frozen(*triples(base, nq, 3e16, rng))


# Cluster cases: id -> (dim, offset, scale, dom)
CLUSTERS = {f"L5-{dim}-{off}": (dim, float(off), 1.0, 16 if dim <= 128 else 32)
            for dim in (17, 32, 61, 64, 200, 256) for off in (0, 1000)}
CLUSTERS.update({f"L6-{dim}": (dim, 0.0, 1e4, 32) for dim in (17, 61, 64)})
CLUSTERS.update({f"L9-{dim}": (dim, 0.0, 1.0, 16) for dim in (128, 64)})


@functools.lru_cache(maxsize=None)
def clusters_case(name):
    dim, offset, scale, _ = CLUSTERS[name]
    return _frozen(*near_tie_clusters(dim, offset, scale))


def order_sensitive(dim, nq=64, nt=100):
    """Rows whose exact order depends on the oracle's summation order (dimension 0 first). Every query
    is the zero vector. Row 0 = (2^14, d, d, ..., d) with d = 2^-13: after 2^28 each d^2 = 2^-26 is a
    quarter of an ulp and is lost, so its d^2 is 2^28 exactly. Row 1 = (2^14, 0, ..., 0, 2^-11): d^2 =
    2^28 + 2^-22 (4 ulps). In dimension order row 0 is nearer; summed from the last dimension the
    (dim - 1) 2^-26 of row 0 add up first (15 ulps at dim 61 and more) and row 1 is nearer. Every other
    row is (20000, noise): d^2 >= 4e8, far beyond any certificate's tolerance of the two (below 1e4
    at these magnitudes), so the two candidates' exact sums alone decide the answer.
    -> q, t; the exact answer is idx 0, idx2 1."""
    rng = np.random.default_rng(dim)
    t = np.zeros((nt, dim), np.float32)
    t[:, 0] = 20000.0
    t[2:, 1:] = rng.normal(scale=0.5, size=(nt - 2, dim - 1))
    t[0, 0] = t[1, 0] = 2.0 ** 14
    t[0, 1:] = 2.0 ** -13
    t[1, 1:] = 0.0
    t[1, dim - 1] = 2.0 ** -11
    return np.zeros((nq, dim), np.float32), t


ORDER = {"O-128": (128, 1), "O-64": (64, 1), "O-61": (61, 0)}    # id -> (dim, device view offset in floats)


@functools.lru_cache(maxsize=None)
def order_case(name):
    return _frozen(*order_sensitive(ORDER[name][0]))


PLAIN = {"L7-200": (300, 4099, 200), "L7-129": (257, 1000, 129)}


@functools.lru_cache(maxsize=None)
def plain_case(name):
    nq, nt, dim = PLAIN[name]
    q, t, _ = S.l2_problem(nq, nt, dim=dim, seed=nq + nt + dim)
    return _frozen(q, t)


# ---- shared oracle answers --------------------------------------------------------------------------

_answers = {}


def oracle_answer(oracle, kind, name, q, t):
    """The oracle's four outputs for a case, computed once per process and left unchanged."""
    key = (kind, name)
    if key not in _answers:
        out = oracle.match_hamming(q, t) if kind == "hamming" else oracle.match_l2(q, t)
        _answers[key] = _frozen(*out)
    return _answers[key]
