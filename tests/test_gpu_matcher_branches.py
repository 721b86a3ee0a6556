"""Every kernel instantiation and dispatch branch of the three brute-force matchers (needs an MI355X).

The shapes of test_gpu_matchers.py / test_gpu_matcher_shards.py / test_gpu_l2u8.py follow the
workloads; the ones here follow the launch code (matcher section, lists which test reaches
which branch). Every comparison is array_equal on all four outputs against the oracle: there is no
tolerance anywhere. Which instantiation ran is read back from the library (mcvHammingLastQueryTiles,
mcvL2LastGemmForm, mcvL2LastExactScans, mcvL2LastScanChunks) and asserted, so a retuned constant
makes a test fail instead of silently missing its branch. The inputs and the reference-only predicates
are tests/_matcher_cases.py's; test_matcher_cases.py checks them on the CPU."""
import numpy as np
import pytest
import torch

from minicv_amd import device as D, native as N

import _l2u8_ref as R
import _matcher_cases as MC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def to_dev(a, offset=0):
    """a on the device; offset > 0: as a view that starts `offset` elements into its allocation, so the
    device pointer is not 16-byte aligned."""
    a = np.ascontiguousarray(a)
    if offset == 0:
        return torch.from_numpy(np.array(a)).to(DEV)    # a writable copy: the case arrays are read-only
    buf = torch.empty(a.size + offset + 16, dtype=torch.from_numpy(np.empty(0, a.dtype)).dtype, device=DEV)
    view = buf[offset:offset + a.size].view(a.shape)
    view.copy_(torch.from_numpy(np.array(a)))
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    return view


# ---- Hamming ---------------------------------------------------------------------------------------

def run_hamming(q, t, form, offset=0):
    tq, tt = to_dev(q, offset), to_dev(t, offset)
    out = [torch.empty(q.shape[0], dtype=torch.int32, device=DEV) for _ in range(4)]
    D.match_hamming(tq, tt, *out, form=form)
    torch.cuda.synchronize()
    qt = N.lib().mcvHammingLastQueryTiles()
    return [o.cpu().numpy() for o in out], qt


def hamming_both_forms(q, t, ref, query_tiles, offset=0):
    """Both kernel forms against the reference and against each other; -> the GEMM form's outputs."""
    gemm, qt = run_hamming(q, t, "gemm", offset)
    print(f"mcvHammingLastQueryTiles() = {qt} (gemm)")
    assert qt == query_tiles
    pop, qt = run_hamming(q, t, "popcount", offset)
    assert qt == 0
    for g, p, r in zip(gemm, pop, ref):
        np.testing.assert_array_equal(g, r)
        np.testing.assert_array_equal(p, r)
        np.testing.assert_array_equal(g, p)
    return gemm


@pytest.mark.parametrize("name", list(MC.HAMMING))
def test_hamming_two_query_tiles(gpu, oracle, name):
    """H1-H5: mcv_hamming_mfma<8 | 16, 2, 4> (QT = 2), every output against the oracle in both forms."""
    q, t = MC.hamming_case(name)
    ref = MC.oracle_answer(oracle, "hamming", name, q, t)
    idx = hamming_both_forms(q, t, ref, 2)[0]
    if name == "H5":
        assert idx.max() == (1 << 22) - 2      # the index field's last value but one: row nt - 1


def test_hamming_index_field_limit_rejected(gpu):
    """nt = 2^22 does not fit the key's 22-bit index field: refused with the limit named, nothing launched."""
    nt = 1 << 22
    q = torch.zeros((40, 32), dtype=torch.uint8, device=DEV)
    t = torch.empty((nt, 32), dtype=torch.uint8, device=DEV)
    out = [torch.empty(40, dtype=torch.int32, device=DEV) for _ in range(4)]
    for form in ("gemm", "popcount"):
        with pytest.raises(N.NativeError, match=r"nt 4194304 outside \[0, 2\^22\)"):
            D.match_hamming(q, t, *out, form=form)


def test_hamming_plants(gpu, oracle):
    """H6: duplicates across tiles and segments, all-zero and all-one rows, the last row as a best match
    on its own, at H2's shape (QT = 2)."""
    q, t, idx, dist, idx2, dist2, qsat, tsat = MC.hamming_plants_case()
    got = hamming_both_forms(q, t, (idx, dist, idx2, dist2), 2)
    for g, r in zip(got, oracle.match_hamming(q, t)):
        np.testing.assert_array_equal(g, r)
    zero = np.zeros(len(q), np.int32)
    far = np.where(np.arange(len(qsat)) % 2 == 0, 8 * t.shape[1], 0).astype(np.int32)
    got = hamming_both_forms(qsat, tsat, (zero, far, zero + 1, far), 2)
    assert set(np.unique(got[1])) == {0, 8 * t.shape[1]}
    for g, r in zip(got, oracle.match_hamming(qsat, tsat)):
        np.testing.assert_array_equal(g, r)


@pytest.mark.parametrize("nq,nt,nbytes", MC.HAMMING_ALIGN)
def test_hamming_misaligned_views(gpu, oracle, nq, nt, nbytes):
    """H7: device views one byte into their allocations take the repack at full width (the GEMM form
    reads 16-byte vectors); the answer is the aligned call's and the oracle's."""
    from minicv_amd import synthetic as S
    q, t, _ = S.hamming_problem(nq, nt, nbytes=nbytes, seed=nq + nt + nbytes)
    ref = oracle.match_hamming(q, t)
    aligned = hamming_both_forms(q, t, ref, 1)
    shifted = hamming_both_forms(q, t, ref, 1, offset=1)
    for a, s in zip(aligned, shifted):
        np.testing.assert_array_equal(a, s)


# ---- float L2 --------------------------------------------------------------------------------------

def run_l2(q, t, offset=0):
    tq, tt = to_dev(q, offset), to_dev(t, offset)
    nq = q.shape[0]
    idx, idx2 = (torch.empty(nq, dtype=torch.int32, device=DEV) for _ in range(2))
    d, d2 = (torch.empty(nq, dtype=torch.float32, device=DEV) for _ in range(2))
    D.match_l2(tq, tt, idx, d, idx2, d2)
    torch.cuda.synchronize()
    L = N.lib()
    diag = {"form": L.mcvL2LastGemmForm(), "scans": L.mcvL2LastExactScans(), "chunks": L.mcvL2LastScanChunks()}
    return (idx.cpu().numpy(), d.cpu().numpy(), idx2.cpu().numpy(), d2.cpu().numpy()), diag


def check_l2(name, q, t, ref, offset=0):
    got, diag = run_l2(q, t, offset)
    print(f"{name}: mcvL2LastGemmForm() = {diag['form']}, mcvL2LastExactScans() = {diag['scans']} of {len(q)}, "
          f"mcvL2LastScanChunks() = {diag['chunks']}")
    ri, rd, ri2, rd2 = ref
    np.testing.assert_array_equal(got[0], ri)
    np.testing.assert_array_equal(got[2], ri2)
    np.testing.assert_array_equal(got[1].view(np.uint32), rd.astype(np.float32).view(np.uint32))
    np.testing.assert_array_equal(got[3].view(np.uint32), rd2.astype(np.float32).view(np.uint32))
    return got, diag


# the exact scan's work units by GEMM form (kL2ScanBlocks x kL2ScanThreadsU / 256 in the f16 domain,
# kL2ScanBlocks otherwise): used only to say which T the L4 queues should get, never as a coverage
# claim — the T == 1 cases assert mcvL2LastScanChunks() itself
SCAN_UNITS = {16: 512, 32: 256}


@pytest.mark.parametrize("name", list(MC.TRIPLES))
def test_l2_triples_every_query_scanned(gpu, oracle, name):
    """L1-L4: every query ties three ways, so all of them take the exact scan; L1-L3 are long enough
    queues that the scan runs one chunk per batch (T == 1) and writes the final results itself —
    mcv_l2_scan<32 / 64 / 128> in the f16 domain, l2_exact_scan_body<128, 512> behind the RAW f32 GEMM,
    mcv_l2_exact_scan<256> behind mcv_l2_mfma<256>; L4 are one- and few-batch queues (T > 1)."""
    nq, dim, scale, dom, chunks = MC.TRIPLES[name]
    q, t = MC.triples_case(name)
    ref = MC.oracle_answer(oracle, "l2", name, q, t)
    got, diag = check_l2(name, q, t, ref)
    assert diag["form"] == dom
    assert diag["scans"] == nq
    if chunks is not None:
        assert diag["chunks"] == chunks
    else:
        assert diag["chunks"] == SCAN_UNITS[dom] // -(-nq // 32) and diag["chunks"] > 1
    assert (got[0] < MC.NBASE).all() and (got[2] == got[0] + MC.NBASE).all()


@pytest.mark.parametrize("name", [n for n in MC.CLUSTERS if not n.startswith("L9")])
def test_l2_cluster_filters(gpu, oracle, name):
    """L5 / L6: the scan filters at every DP on real near-ties (several train tiles per chunk); L6 is
    out of the f16 domain with dim < DP, nq < nqPad and nt % 32 != 0 (the RAW staging's edges)."""
    dim, offset, scale, dom = MC.CLUSTERS[name]
    q, t = MC.clusters_case(name)
    ref = MC.oracle_answer(oracle, "l2", name, q, t)
    got, diag = check_l2(name, q, t, ref)
    assert diag["form"] == dom
    assert diag["scans"] >= MC.must_queue(q, t)
    assert diag["chunks"] > 1


@pytest.mark.parametrize("name", list(MC.PLAIN))
def test_l2_wide_rows_many_blocks(gpu, oracle, name):
    """L7: mcv_l2_mfma<256> with several query blocks and train chunks."""
    q, t = MC.plain_case(name)
    got, diag = check_l2(name, q, t, MC.oracle_answer(oracle, "l2", name, q, t))
    assert diag["form"] == 32


@pytest.mark.parametrize("name", list(MC.OVERFLOW))
def test_l2_fp32_norm_overflow_boundary(gpu, oracle, name):
    """L8: coordinates ~3e18 — a part of the fp32 norms overflows (dim 32) or all of them (dim 200)
    while every fp64 distance stays finite: the scan thresholds' overflow guards decide nothing and
    the exact sums give the oracle's answer."""
    q, t = MC.overflow_case(name)
    got, diag = check_l2(name, q, t, MC.oracle_answer(oracle, "l2", name, q, t))
    assert diag["form"] == 32
    assert (got[0] >= 0).all() and (got[2] == got[0] + MC.OVERFLOW_NBASE).all()
    assert np.isfinite(got[1]).all() and np.isfinite(got[3]).all()


@pytest.mark.parametrize("name", ["L9-128", "L9-64"])
def test_l2_misaligned_views(gpu, oracle, name):
    """L9: device views one float into their allocations: mcv_l2_prep16<false> through the pointer (dim
    % 4 == 0) and the scalar path of l2_exact2; the answer is the aligned call's and the oracle's."""
    dim, offset, scale, dom = MC.CLUSTERS[name]
    q, t = MC.clusters_case(name)
    ref = MC.oracle_answer(oracle, "l2", name, q, t)
    aligned, da = check_l2(name, q, t, ref)
    shifted, ds = check_l2(name + " shifted", q, t, ref, offset=1)
    assert da["form"] == ds["form"] == dom
    assert ds["scans"] >= MC.must_queue(q, t)
    for a, s in zip(aligned, shifted):
        np.testing.assert_array_equal(a.view(np.uint32), s.view(np.uint32))


@pytest.mark.parametrize("name", list(MC.ORDER))
def test_l2_exact2_keeps_the_dimension_order(gpu, oracle, name):
    """mcv_l2_refine's own exact sums decide these queries (both candidates are 1e8 nearer than any
    other row, so the certificate holds and nothing is queued), and the two candidates' order depends on
    summing in dimension order: l2_exact2's scalar path through a misaligned view (dim 128, 64) and
    through dim % 4 != 0 (dim 61), next to the float4 path of the aligned call."""
    dim, offset = MC.ORDER[name]
    q, t = MC.order_case(name)
    ref = MC.oracle_answer(oracle, "l2", name, q, t)
    for off in sorted({0, offset}):
        got, diag = check_l2(f"{name} offset {off}", q, t, ref, offset=off)
        assert diag["form"] == 16 and diag["scans"] == 0
        assert (got[0] == 0).all() and (got[2] == 1).all()


# ---- uint8 L2 --------------------------------------------------------------------------------------

@pytest.mark.parametrize("nq,nt,dim", [(300, 1000, 128), (150, 333, 17)])
def test_l2u8_misaligned_views(gpu, nq, nt, dim):
    """U1: device views one byte into their allocations take mcv_l2u8_prep's byte-load path (at dim 128
    through the pointer alone)."""
    q, t = R.random_u8(nq, nt, dim, seed=nq + nt + dim)
    ref = R.match_l2_u8(q, t)
    for offset in (0, 1):
        tq, tt = to_dev(q, offset), to_dev(t, offset)
        idx, idx2 = (torch.empty(nq, dtype=torch.int32, device=DEV) for _ in range(2))
        d, d2 = (torch.empty(nq, dtype=torch.float32, device=DEV) for _ in range(2))
        D.match_l2_u8(tq, tt, idx, d, idx2, d2)
        torch.cuda.synchronize()
        R.assert_same([x.cpu().numpy() for x in (idx, d, idx2, d2)], ref)
