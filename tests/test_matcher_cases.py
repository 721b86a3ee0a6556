"""CPU checks of the matcher branch-test inputs (tests/_matcher_cases.py): with the oracle and numpy
only, every case does what test_gpu_matcher_branches.py relies on — the Hamming launch quantity is
on the intended side of its threshold, the triples cases force every query into the exact scan, the
cluster cases a fifth of them, the values sit on the intended side of the f16 domain bound, the
overflow cases overflow the share of fp32 norms they are meant to, and the tie rule's answer is the one
the GPU tests assert."""
import numpy as np
import pytest

import _matcher_cases as MC


# ---- Hamming ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,expect", [("H1", 8194), ("H2", 8210), ("H3", 8210), ("H4", 65626), ("H5", 131072)])
def test_hamming_cases_take_two_query_tiles(name, expect):
    nq, nt, nbytes = MC.HAMMING[name]
    assert MC.steps2(nq, nt) == expect and expect > 8192
    assert nt < (1 << 22)


def test_hamming_case_shapes():
    nq, nt, nbytes = MC.HAMMING["H1"]
    assert nt % 32 == 1 and nq < 256            # a last tile of one row; one query block
    nq, nt, nbytes = MC.HAMMING["H2"]
    assert nt % 32 == 10 and nq % 256 == 1      # the last query block holds one query
    assert MC.HAMMING["H3"][2] % 4 != 0         # the repack
    nq, nt, nbytes = MC.HAMMING["H4"]
    # ranges of at most 128 tiles: more of them than two blocks per CU at any CU count up to 256
    assert -(-nt // 32) / 128 > 2 * 256 and nbytes == 64
    assert MC.HAMMING["H5"][1] == (1 << 22) - 1
    for nq, nt, nbytes in MC.HAMMING_ALIGN:
        assert MC.steps2(nq, nt) <= 8192


def test_hamming_h5_neighbours_at_the_last_rows(oracle):
    q, t = MC.hamming_case("H5")
    nt = len(t)
    idx, dist, idx2, dist2 = MC.oracle_answer(oracle, "hamming", "H5", q, t)
    assert (idx[0], dist[0], idx2[0], dist2[0]) == (nt - 1, 0, nt - 2, 1)
    assert (idx[1], dist[1], idx2[1], dist2[1]) == (nt - 2, 0, nt - 1, 1)
    assert (idx[2], dist[2], idx2[2], dist2[2]) == (0, 0, nt - 1, 2)
    assert idx.max() == (1 << 22) - 2


def test_hamming_plants_answer_by_construction(oracle):
    q, t, idx, dist, idx2, dist2, qsat, tsat = MC.hamming_plants_case()
    nbytes = t.shape[1]
    for r, e in zip(oracle.match_hamming(q, t), (idx, dist, idx2, dist2)):
        np.testing.assert_array_equal(r, e)
    assert (dist == 0).all() and set(np.unique(dist2)) == {0, 1}
    # planted rows in the first tile, a middle one, the last partial tile and the last row (as the best)
    nt = len(t)
    assert idx.min() < 32 and idx.max() == nt - 1 and (idx2 >= (nt - 1) // 32 * 32).any()
    assert (q == 0).all(axis=1).any() and (q == 255).all(axis=1).any()
    r = oracle.match_hamming(qsat, tsat)
    assert (r[0] == 0).all() and (r[2] == 1).all()
    np.testing.assert_array_equal(r[1], np.where(np.arange(len(qsat)) % 2 == 0, 8 * nbytes, 0))
    np.testing.assert_array_equal(r[3], r[1])


@pytest.mark.parametrize("name", ["H1", "H2", "H3", "H4"])
def test_hamming_cases_last_row_is_a_best_match(oracle, name):
    q, t = MC.hamming_case(name)
    idx, dist, idx2, dist2 = MC.oracle_answer(oracle, "hamming", name, q, t)
    assert idx[-1] == len(t) - 1 and dist[-1] == 3 and dist2[-1] > 3


# ---- float L2 --------------------------------------------------------------------------------------

def f16_domain(q, t):
    return max(np.abs(q).max(), np.abs(t).max()) < 2.0 ** 15


@pytest.mark.parametrize("name", list(MC.TRIPLES))
def test_triples_cases_queue_every_query(oracle, name):
    nq, dim, scale, dom, chunks = MC.TRIPLES[name]
    q, t = MC.triples_case(name)
    assert q.shape == (nq, dim) and t.shape == (3 * MC.NBASE, dim)
    assert MC.must_queue(q, t) == nq
    idx, d, idx2, d2 = MC.oracle_answer(oracle, "l2", name, q, t)
    assert (idx < MC.NBASE).all() and (idx2 == idx + MC.NBASE).all() and (d == d2).all()
    s = MC.smallest3(q, t)
    np.testing.assert_array_equal(np.sqrt(s[:, 0]), d)      # the numpy sums are the oracle's, bit for bit
    np.testing.assert_array_equal(np.sqrt(s[:, 1]), d2)
    assert (s[:, 0] == s[:, 2]).all()
    if dim <= 128:
        assert f16_domain(q, t) == (dom == 16)
    else:
        assert dom == 32


@pytest.mark.parametrize("name", list(MC.CLUSTERS))
def test_cluster_cases_queue_a_fifth(oracle, name):
    dim, offset, scale, dom = MC.CLUSTERS[name]
    q, t = MC.clusters_case(name)
    assert q.shape == (700, dim) and t.shape == (1200, dim) and len(t) % 32 != 0
    mq = MC.must_queue(q, t)
    assert mq >= len(q) / 5
    assert mq < len(q)              # real near-ties beside the exact ones: the filter has work to do
    idx, d, idx2, d2 = MC.oracle_answer(oracle, "l2", name, q, t)
    s = MC.smallest3(q, t)
    np.testing.assert_array_equal(np.sqrt(s[:, 0]), d)
    np.testing.assert_array_equal(np.sqrt(s[:, 1]), d2)
    if dim <= 128:
        assert f16_domain(q, t) == (dom == 16)
    else:
        assert dom == 32


@pytest.mark.parametrize("name", list(MC.OVERFLOW))
def test_overflow_cases_norm_share(oracle, name):
    """normal * 3e18: at dim 32 a part of the fp32 norms overflows and a part stays finite (the mixed
    case); at dim 200 every one overflows (the sum of 200 squares of ~3e18 is ~1.8e39). The fp64
    distances stay finite either way, and every query still ties three ways."""
    nq, dim = MC.OVERFLOW[name]
    q, t = MC.overflow_case(name)
    share = MC.f32_norm_inf_share(t)
    print(f"{name}: {share:.3f} of the train rows have an infinite fp32 norm")
    if dim == 32:
        assert 0.1 <= share <= 0.5
    else:
        assert share == 1.0
    assert MC.must_queue(q, t) == nq
    idx, d, idx2, d2 = MC.oracle_answer(oracle, "l2", name, q, t)
    assert (idx >= 0).all() and (idx2 == idx + MC.OVERFLOW_NBASE).all()
    assert np.isfinite(d.astype(np.float32)).all() and np.isfinite(d2.astype(np.float32)).all()
    assert not f16_domain(q, t)


@pytest.mark.parametrize("name", list(MC.PLAIN))
def test_plain_cases_shape(name):
    nq, nt, dim = MC.PLAIN[name]
    q, t = MC.plain_case(name)
    assert q.shape == (nq, dim) and t.shape == (nt, dim) and dim > 128 and nq > 256


@pytest.mark.parametrize("name", list(MC.ORDER))
def test_order_sensitive_rows(oracle, name):
    """In dimension order row 0 is nearer than row 1; summed from the last dimension it is the other
    way round, and every other row is far away."""
    dim, _ = MC.ORDER[name]
    q, t = MC.order_case(name)
    idx, d, idx2, d2 = MC.oracle_answer(oracle, "l2", name, q, t)
    assert (idx == 0).all() and (idx2 == 1).all()
    fwd = MC.exact_d2(q[:1], t)[0]
    rev = MC.exact_d2(q[:1, ::-1], t[:, ::-1])[0]
    assert fwd[0] == 2.0 ** 28 and fwd[1] == 2.0 ** 28 + 2.0 ** -22 and fwd[0] < fwd[1]
    assert rev[1] == fwd[1] and rev[0] > rev[1]
    assert fwd[2:].min() > 3.9e8
    assert max(np.abs(q).max(), np.abs(t).max()) < 2.0 ** 15
