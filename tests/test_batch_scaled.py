"""Batched findScaled on the CPU: the exports and their declarations, the host twin against the
per-problem twin and the oracle bit for bit, every refusal (before the device, nothing written), and
the CSR / work-list index code under AddressSanitizer + UBSan in a stand-alone program. No kernel is
launched here."""
import shutil
import subprocess

import numpy as np
import pytest

import _scaled_batch as B
from minicv_amd import camera as CM
from minicv_amd import native as N

EXPORTS = ("cvFindScaledPoseBatch", "cvFindScaledPoseBatchCosts", "mcvHostFindScaledPoseBatch",
           "mcvTestScaledBatchStats")
CHECKED = ("cvFindScaledPoseBatch", "mcvHostFindScaledPoseBatch")


def test_exports_declared(native):
    txt = (N.ROOT / "include" / "minicv_native.h").read_text()
    for name in EXPORTS:
        assert name in N.SIGNATURES and getattr(native.lib(), name) is not None
        assert f"MCV_API int {name}(" in txt
    import minicv_amd
    assert minicv_amd.findScaledBatch is CM.findScaledBatch
    assert minicv_amd.findScaledBatchCosts is CM.findScaledBatchCosts


def test_abi_version_unchanged(native):
    assert native.lib().mcvAbiVersion() == 3
    assert "#define MCV_ABI_VERSION 3\n" in (N.ROOT / "include" / "minicv_native.h").read_text()


def test_mixed_batch_shape():
    b = B.mixed()
    sizes = b.sizes()
    assert sizes[0] == 0 and sizes[-1] == 0 and 8 not in set(b.set_idx.tolist())
    assert (b.set_idx == 9).sum() == 4 and set(B.MIXED_SIZES) == set(sizes.tolist())
    on200 = [p for p in range(b.P) if b.set_idx[p] == 9]
    keys = {(tuple(b.cam_rows[p]), tuple(b.rots[p]), tuple(b.trans[p])) for p in on200}
    assert len(keys) == 4
    assert len({tuple(r) for r in b.cam_rows}) > 8   # the cameras differ between problems


def test_host_twin_equals_per_problem_twin_and_oracle(native, oracle):
    b = B.mixed()
    k, costs, scales, ev, _ = B.call("mcvHostFindScaledPoseBatch", b)
    assert k == int(np.isfinite(costs).sum()) and k >= 10, native.last_error()
    B.assert_results((costs, scales, ev), B.oracle_results(oracle, b), "twin against the oracle")
    for p in range(b.P):
        W, O = b.set_of(p)
        sc, co = B.host_costs(b, p)
        if W.shape[0]:
            sc_ref, co_ref, used = oracle.scaled_costs(B.cam14(b.cams[p]), W, O, b.poses[p].Rotation,
                                                       b.poses[p].Translation)
            np.testing.assert_array_equal(sc, sc_ref)
            np.testing.assert_array_equal(co, co_ref)
        else:
            used = np.zeros(0, np.uint8)
        # the single twin's arrays choose what the batch twin reports
        cand = np.flatnonzero(np.repeat(used.astype(bool), 2) & np.isfinite(co))
        assert ev[p] == 2 * int(used.sum())
        if cand.size == 0:
            assert costs[p] == np.inf and scales[p] == 0.0
        else:
            best = cand[np.argmin(co[cand])]   # argmin: the first of equal minima
            assert costs[p] == co[best] and scales[p] == sc[best]


def test_host_twin_set_idx_none_and_reversed(native):
    b = B.mixed()
    ref = B.call("mcvHostFindScaledPoseBatch", b)[1:4]
    e = b.expanded()
    assert e.set_idx is None and e.S == e.P
    B.assert_results(B.call("mcvHostFindScaledPoseBatch", e)[1:4], ref, "setIdx = None")
    r = b.reversed()
    B.assert_results(B.call("mcvHostFindScaledPoseBatch", r)[1:4], tuple(a[::-1] for a in ref), "reversed")
    k, costs, scales, ev, _ = B.call("mcvHostFindScaledPoseBatch", b, evaluated=False)
    assert k >= 0 and np.all(ev == B.SENT_I)
    B.assert_results((costs, scales), ref[:2], "evaluated = None")


@pytest.mark.parametrize("name", CHECKED)
def test_refusals_before_the_device(native, name):
    """The same with and without a GPU; a refused call writes nothing."""
    b = B.mixed()

    def refused(word, **kw):
        k, _, _, _, untouched = B.call(name, b, **kw)
        assert k == -1 and untouched, (kw, k)
        assert word in native.last_error() and name in native.last_error(), native.last_error()

    for null in ("cams", "rots", "trans", "off", "costs", "scales", "world", "obs"):
        refused("null", null=(null,))
    refused("negative P", P=-1)
    refused("negative S", S=-2)
    refused("S == P", set_idx=None)                       # a null setIdx with S != P
    bad = b.offsets.copy()
    bad[0] = 1
    refused("offsets[0]", offsets=bad)
    bad = b.offsets.copy()
    bad[4] = bad[3] - 1
    refused("decrease at set 3", offsets=bad)
    for v in (-1, b.S):
        idx = b.set_idx.copy()
        idx[5] = v
        refused("setIdx[5]", set_idx=idx)
    refused("offsets[S]", offsets=[0, (1 << 28) + 1], S=1, P=1, set_idx=[0])
    refused("candidates", offsets=[0, 1 << 27], S=1, P=3, set_idx=[0, 0, 0])
    # P == 0 succeeds without looking at anything else
    k, _, _, _, untouched = B.call(name, b, P=0, null=("cams", "off", "costs"))
    assert k == 0 and untouched and native.last_error() == ""


def test_costs_helper_and_stats_check_their_arguments(native):
    L = N.lib()
    b = B.mixed()
    assert L.mcvTestScaledBatchStats(None) == -1
    assert L.cvFindScaledPoseBatchCosts(None, None, None, None, 0, None, None, None, 0, None, None) == 0
    assert L.cvFindScaledPoseBatchCosts(None, None, None, None, 2, None, None, None, 2, None, None) == -1
    assert "null" in native.last_error()
    sc = np.full(4, B.SENT_D)
    idx = b.set_idx.copy()
    idx[0] = b.S
    assert L.cvFindScaledPoseBatchCosts(b.cam_rows.ctypes.data, b.rots.ctypes.data, b.trans.ctypes.data,
                                        idx.ctypes.data, b.P, b.world.ctypes.data, b.obs.ctypes.data,
                                        b.offsets.ctypes.data, b.S, sc.ctypes.data, sc.ctypes.data) == -1
    assert "setIdx[0]" in native.last_error() and np.all(sc == B.SENT_D)


def test_all_empty_batch_needs_no_device(native):
    """Every problem on an empty set: the reference's [] case, answered like the single call's N == 0."""
    b = B.build((0, 0, 0), None, 7)
    for name in CHECKED:
        k, costs, scales, ev, _ = B.call(name, b)
        assert k == 0 and np.all(costs == np.inf) and np.all(scales == 0.0) and np.all(ev == 0)
    for cost, pose in CM.findScaledBatch(0.1, b.cams, b.sets, b.poses):
        assert cost == np.inf and pose.ScaleSign == 0 and not pose.Translation.any() and not pose.Rotation.any()


def test_device_export_fails_loudly_without_gpu(native):
    if native.lib().mcvDeviceCount() > 0:
        return   # the valid calls are the GPU suite's subject
    b = B.mixed()
    k, _, _, _, untouched = B.call("cvFindScaledPoseBatch", b)
    assert k == -1 and untouched and "no HIP device" in native.last_error()
    with pytest.raises(N.NativeError, match="no HIP device"):
        CM.findScaledBatch(0.1, b.cams, b.sets, b.poses, b.set_idx)
    with pytest.raises(N.NativeError, match="no HIP device"):
        CM.findScaledBatchCosts(b.cams, b.sets, b.poses, b.set_idx)


def test_index_code_under_sanitizers(tmp_path):
    """tests/asan/scaled_batch_asan_main.cpp: a stand-alone program (its own main, nothing preloaded,
    nothing loaded into Python) over scaled_batch_index.h, built with -fsanitize=address,undefined:
    empty sets first, in the middle and last, shared sets, one-row sets, sizes at the block edges."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "scaled_batch_asan"
    src = N.ROOT / "tests" / "asan" / "scaled_batch_asan_main.cpp"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{N.ROOT / 'minicv_amd' / 'csrc'}", str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "scaled_batch_asan ok" in r.stdout and "ERROR" not in r.stderr
