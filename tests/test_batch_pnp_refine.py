"""CPU tests of cvRefinePnPBatch and cvSolvePnPRansacRefineBatch (the LM / VVS refinement of many cameras in one
call, alone and fused behind the RANSAC batch): the exports are declared and exported, every argument check
runs before the device is touched and before an output is written, and the index arithmetic of a call
(mcvHostRefinePnPBatchLayout: the selected rows of every problem and their place in the compact array) is
checked against numpy, and under sanitizers in a program of its own."""
import ctypes as C
import shutil
import subprocess

import numpy as np
import pytest

from minicv_amd import native as N
from minicv_amd import opencv

NAME = "cvRefinePnPBatch"
FUSED = "cvSolvePnPRansacRefineBatch"
HOOK = "mcvHostRefinePnPBatchLayout"
K0 = [800.0, 0, 640.0, 0, 820.0, 360.0, 0, 0, 1.0]
SENT = -7.25          # fills tVecs / rVecs before a refused call
SENT_B = 0xA5         # fills refined


class Call:
    """One well-formed cvRefinePnPBatch call (two problems of 20 points), fields replaceable."""

    def __init__(self):
        rng = np.random.default_rng(1)
        self.img = np.ascontiguousarray(rng.uniform(0, 1000, (40, 2)))
        self.world = np.ascontiguousarray(rng.uniform(-3, 3, (40, 3)))
        self.offsets = np.array([0, 20, 40], dtype=np.int32)
        self.K = np.array([K0, K0], dtype=np.float64)
        self.dist = np.zeros((2, 4))
        self.mask = np.ones(40, dtype=np.uint8)
        self.t = np.full((2, 3), SENT)
        self.r = np.full((2, 3), SENT)
        self.refined = np.full(2, SENT_B, dtype=np.uint8)
        self.kind = 0
        self.B = 2

    def run(self, **null):
        p = lambda name, arr: None if name in null else arr.ctypes.data
        return N.lib().cvRefinePnPBatch(p("img", self.img), p("world", self.world), p("offsets", self.offsets), self.B,
                                        p("K", self.K), p("dist", self.dist), p("mask", self.mask), self.kind,
                                        p("t", self.t), p("r", self.r), p("refined", self.refined))

    def untouched(self):
        return bool(np.all(self.t == SENT) and np.all(self.r == SENT) and np.all(self.refined == SENT_B))


class FusedCall:
    """One well-formed cvSolvePnPRansacRefineBatch call."""

    def __init__(self):
        c = Call()
        self.img, self.world, self.offsets, self.K, self.dist, self.B = c.img, c.world, c.offsets, c.K, c.dist, 2
        self.t = np.full((2, 3), SENT)
        self.r = np.full((2, 3), SENT)
        self.mask = np.full(40, SENT_B, dtype=np.uint8)
        self.counts = np.full(2, -7, dtype=np.int32)
        self.cfg = N.RansacConfig(8.0, 0.99, 100, N.METHOD_RANSAC, 1, 1, 0, 0, 5)
        self.kind = 0

    def run(self, **null):
        p = lambda name, arr: None if name in null else arr.ctypes.data
        cfg = None if "cfg" in null else C.addressof(self.cfg)
        return N.lib().cvSolvePnPRansacRefineBatch(p("img", self.img), p("world", self.world),
                                                   p("offsets", self.offsets), self.B, p("K", self.K),
                                                   p("dist", self.dist), cfg, self.kind, p("t", self.t),
                                                   p("r", self.r), p("mask", self.mask), p("counts", self.counts))

    def untouched(self):
        return bool(np.all(self.t == SENT) and np.all(self.r == SENT) and np.all(self.mask == SENT_B) and
                    np.all(self.counts == -7))


def _device_visible():
    return N.lib().mcvDeviceCount() > 0


def test_exports_declared(native):
    txt = (N.ROOT / "include" / "minicv_native.h").read_text()
    for name in (NAME, FUSED, HOOK):
        assert name in N.SIGNATURES and getattr(native.lib(), name) is not None
        assert f"MCV_API int {name}(" in txt
    import minicv_amd
    for name in ("refinePnPBatch", "solvePnPRansacWithRefine", "solvePnPRansacWithRefineBatch"):
        assert callable(getattr(opencv, name))
        assert getattr(minicv_amd, name) is getattr(opencv, name)


def test_abi_version_unchanged(native):
    assert native.lib().mcvAbiVersion() == 3


@pytest.mark.parametrize("which", ["img", "world", "offsets", "K", "t", "r"])
def test_null_arguments_rejected(native, which):
    c = Call()
    assert c.run(**{which: True}) == -1
    assert "null" in native.last_error() and NAME in native.last_error()
    assert c.untouched()


def test_bad_arguments_rejected(native):
    c = Call()
    c.B = -1
    assert c.run() == -1 and "negative B" in native.last_error() and c.untouched()
    c = Call()
    c.offsets[0] = 1
    assert c.run() == -1 and "offsets[0]" in native.last_error() and c.untouched()
    c = Call()
    c.offsets[:] = [0, 30, 20]
    assert c.run() == -1 and "decrease" in native.last_error() and "problem 1" in native.last_error()
    assert NAME in native.last_error() and c.untouched()
    for kind in (-1, 2):
        c = Call()
        c.kind = kind
        assert c.run() == -1 and "refineKind" in native.last_error() and NAME in native.last_error()
        assert c.untouched()
        # the kind is refused even when nothing else would need a device
        c.B = 0
        assert c.run() == -1 and "refineKind" in native.last_error() and c.untouched()


def test_empty_batch_and_wrappers(native):
    c = Call()
    c.B = 0
    assert c.run() == 0 and native.last_error() == "" and c.untouched()
    assert c.run(dist=True, mask=True, refined=True) == 0 and native.last_error() == ""
    assert opencv.refinePnPBatch([], [], [], None, [], []) == []
    assert opencv.solvePnPRansacWithRefineBatch([], [], []) == []
    a, w = np.zeros((6, 2)), np.zeros((6, 3))
    z = np.zeros((1, 3))
    with pytest.raises(ValueError):
        opencv.refinePnPBatch([a], [w, w], [K0], None, z, z)
    with pytest.raises(ValueError):
        opencv.refinePnPBatch([a], [w[:5]], [K0], None, z, z)
    with pytest.raises(ValueError):
        opencv.refinePnPBatch([a], [w], [K0, K0], None, z, z)
    with pytest.raises(ValueError):
        opencv.refinePnPBatch([a], [w], [K0], None, z, z, masks=[np.ones(5)])
    with pytest.raises(ValueError):
        opencv.refinePnPBatch([a], [w], [K0], None, z, z, masks=[])
    with pytest.raises(KeyError):
        opencv.refinePnPBatch([a], [w], [K0], None, z, z, kind="GN")


def test_problems_that_cannot_run_need_no_device(native):
    """Fewer than 3 selected rows, or a camera set_camera refuses: the pose stays, refined = 0, the first such
    problem is named with the single call's message. A call made of such problems alone touches no device."""
    c = Call()
    c.mask[:] = 0
    c.mask[[0, 5]] = 1          # problem 0: 2 rows
    c.mask[20:] = 1
    c.K[1, 0] = 0.0             # problem 1: fx = 0
    t0, r0 = c.t.copy(), c.r.copy()
    assert c.run() == 0
    assert "problem 0" in native.last_error() and "need at least 3 correspondences (N=2)" in native.last_error()
    assert NAME in native.last_error()
    np.testing.assert_array_equal(c.t.view(np.uint64), t0.view(np.uint64))
    np.testing.assert_array_equal(c.r.view(np.uint64), r0.view(np.uint64))
    assert not c.refined.any()
    c.mask[:20] = 1
    c.K[0, 4] = np.inf
    assert c.run() == 0 and "problem 0" in native.last_error() and "fx, fy" in native.last_error()
    res = opencv.refinePnPBatch([c.img[:20], c.img[20:]], [c.world[:20], c.world[20:]], c.K, None, r0, t0,
                                masks=[np.zeros(20), np.zeros(20)])
    assert [x[0] for x in res] == [False, False]
    assert "(N=0)" in native.last_error()


def test_device_calls_fail_loudly_without_gpu(native):
    if _device_visible():
        return   # the valid calls are the GPU suite's subject
    for kind in (0, 1):
        for null in ({}, {"mask": True}, {"dist": True}, {"refined": True}):
            c = Call()
            c.kind = kind
            assert c.run(**null) == -1 and "no HIP device" in native.last_error()
            assert c.untouched()
    c = Call()
    with pytest.raises(N.NativeError, match="no HIP device"):
        opencv.refinePnPBatch([c.img[:20], c.img[20:]], [c.world[:20], c.world[20:]], c.K, None, np.zeros((2, 3)),
                              np.ones((2, 3)))
    f = FusedCall()
    assert f.run() == -1 and "no HIP device" in native.last_error()
    with pytest.raises(N.NativeError, match="no HIP device"):
        opencv.solvePnPRansacWithRefineBatch([c.img[:20], c.img[20:]], [c.world[:20], c.world[20:]], c.K)
    with pytest.raises(N.NativeError, match="no HIP device"):
        opencv.solvePnPRansacWithRefine(c.img[:20], c.world[:20], K0)


# ---- the fused export refuses what cvSolvePnPRansacBatch refuses ------------------------------------
@pytest.mark.parametrize("which", ["img", "world", "offsets", "K", "t", "r", "mask", "counts"])
def test_fused_null_arguments_rejected(native, which):
    f = FusedCall()
    assert f.run(**{which: True}) == -1
    assert "null" in native.last_error() and FUSED in native.last_error()
    assert f.untouched()


def test_fused_bad_arguments_rejected(native):
    f = FusedCall()
    f.B = -1
    assert f.run() == -1 and "negative B" in native.last_error() and f.untouched()
    f = FusedCall()
    f.offsets = np.array([1, 20, 40], dtype=np.int32)
    assert f.run() == -1 and "offsets[0]" in native.last_error() and f.untouched()
    f = FusedCall()
    f.offsets = np.array([0, 30, 20], dtype=np.int32)
    assert f.run() == -1 and "decrease" in native.last_error() and "problem 1" in native.last_error()
    for kind in (-1, 2):
        f = FusedCall()
        f.kind = kind
        assert f.run() == -1 and "refineKind" in native.last_error() and FUSED in native.last_error()
        assert f.untouched()
    f = FusedCall()
    f.B = 0
    assert f.run() == 0 and native.last_error() == ""


@pytest.mark.parametrize("field,value,word", [
    ("method", N.METHOD_LSQ, "method"), ("method", N.METHOD_LMEDS, "method"),
    ("flags", N.FLAG_FUSED_ERROR, "MCV_FLAG_FUSED_ERROR"), ("flags", N.FLAG_FAST_MINIMAL, "MCV_FLAG_FAST_MINIMAL"),
    ("flags", 4, "bit 4"), ("deviceCount", 2, "deviceCount"), ("confidence", 1.0, "confidence"),
    ("confidence", float("nan"), "confidence")])
def test_fused_unsupported_configuration_rejected(native, field, value, word):
    f = FusedCall()
    setattr(f.cfg, field, value)
    assert f.run() == -1
    assert word in native.last_error() and FUSED in native.last_error()
    assert f.untouched()


# ---- the layout -------------------------------------------------------------------------------------
SIZES = (0, 1, 2, 3, 31, 32, 33, 255, 256, 257)


def _offsets(sizes):
    o = np.zeros(len(sizes) + 1, dtype=np.int32)
    o[1:] = np.cumsum(sizes)
    return o


def _layout(offsets, mask):
    B = len(offsets) - 1
    counts = np.full(max(B, 1), -7, dtype=np.int32)
    comp = np.full(B + 1, -7, dtype=np.int32)
    big = N.lib().mcvHostRefinePnPBatchLayout(offsets.ctypes.data, B, None if mask is None else mask.ctypes.data,
                                              counts.ctypes.data, comp.ctypes.data)
    assert big >= 0, N.last_error()
    return big, counts[:B], comp


def _masks(offsets):
    total = int(offsets[-1])
    first, last = np.zeros(total, np.uint8), np.zeros(total, np.uint8)
    for a, b in zip(offsets[:-1], offsets[1:]):
        if b > a:
            first[a] = 1
            last[b - 1] = 1
    odd = np.zeros(total, np.uint8)
    odd[::3] = 255
    odd[1::3] = 2
    return {"zero": np.zeros(total, np.uint8), "one": np.ones(total, np.uint8), "first": first, "last": last,
            "bytes_255_and_2": odd}


@pytest.mark.parametrize("which", ["zero", "one", "first", "last", "bytes_255_and_2", None])
def test_layout_against_numpy(native, which):
    offsets = _offsets(SIZES)
    mask = None if which is None else _masks(offsets)[which]
    big, counts, comp = _layout(offsets, mask)
    sel = np.ones(int(offsets[-1]), bool) if mask is None else mask != 0
    exp = np.array([int(sel[a:b].sum()) for a, b in zip(offsets[:-1], offsets[1:])], dtype=np.int32)
    np.testing.assert_array_equal(counts, exp)
    np.testing.assert_array_equal(comp, np.concatenate([[0], np.cumsum(exp)]))
    assert big == int(exp.max())
    if which == "bytes_255_and_2":   # every non-zero byte selects
        assert int(exp.sum()) == int(np.count_nonzero(mask)) > int(offsets[-1]) // 2
    if which in ("first", "last"):
        assert exp.tolist() == [0] + [1] * (len(SIZES) - 1)
    if which is None:
        np.testing.assert_array_equal(comp, offsets)


def test_layout_hook_checks_its_arguments(native):
    L = N.lib()
    o = _offsets([3, 4])
    c, q = np.zeros(2, np.int32), np.zeros(3, np.int32)
    assert L.mcvHostRefinePnPBatchLayout(None, 2, None, c.ctypes.data, q.ctypes.data) == -1
    assert L.mcvHostRefinePnPBatchLayout(o.ctypes.data, 2, None, None, q.ctypes.data) == -1
    assert L.mcvHostRefinePnPBatchLayout(o.ctypes.data, 2, None, c.ctypes.data, None) == -1
    assert L.mcvHostRefinePnPBatchLayout(o.ctypes.data, -1, None, c.ctypes.data, q.ctypes.data) == -1
    bad = np.array([0, 5, 4], dtype=np.int32)
    assert L.mcvHostRefinePnPBatchLayout(bad.ctypes.data, 2, None, c.ctypes.data, q.ctypes.data) == -1
    assert "problem 1" in native.last_error()
    assert L.mcvHostRefinePnPBatchLayout(o.ctypes.data, 0, None, c.ctypes.data, q.ctypes.data) == 0 and q[0] == 0


def test_index_code_under_sanitizers(tmp_path):
    """tests/asan/pnp_refine_batch_asan_main.cpp: a stand-alone program (its own main, nothing preloaded,
    nothing loaded into Python) over pnp_refine_batch_index.h, built with -fsanitize=address,undefined."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "pnp_refine_batch_asan"
    src = N.ROOT / "tests" / "asan" / "pnp_refine_batch_asan_main.cpp"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{N.ROOT / 'minicv_amd' / 'csrc'}", str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pnp_refine_batch_asan ok" in r.stdout and "ERROR" not in r.stderr
