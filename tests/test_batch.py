"""CPU tests of cvFindModelBatch (B independent RANSAC problems in one call): every argument check runs
before the device is touched, and the index arithmetic of a call (mcvHostBatchLayout: the descriptor
table, 64-bit slot offsets, the rounds under the slot cap) and the plan of a hypothesis round
(mcvHostBatchRound: which problems run, their counts, the compact stride) are checked against their definitions,
the plan also under sanitizers in a program of its own."""
import ctypes as C
import shutil
import subprocess

import numpy as np
import pytest

from minicv_amd import native as N
from minicv_amd import opencv

MODELS = (N.MODEL_HOMOGRAPHY, N.MODEL_FUNDAMENTAL, N.MODEL_AFFINE, N.MODEL_SIMILARITY)
SAMPLE = {N.MODEL_HOMOGRAPHY: 4, N.MODEL_FUNDAMENTAL: 8, N.MODEL_AFFINE: 3, N.MODEL_SIMILARITY: 2}


class Call:
    """One well-formed call (two problems of 20 points), fields replaceable one at a time."""

    def __init__(self):
        rng = np.random.default_rng(1)
        self.a = np.ascontiguousarray(rng.uniform(0, 100, (40, 2)))
        self.b = np.ascontiguousarray(rng.uniform(0, 100, (40, 2)))
        self.offsets = np.array([0, 20, 40], dtype=np.int32)
        self.models = np.zeros((2, 9))
        self.mask = np.zeros(40, dtype=np.uint8)
        self.counts = np.zeros(2, dtype=np.int32)
        self.cfg = N.RansacConfig(3.0, 0.99, 100, N.METHOD_RANSAC, 1, 1, 0, 0, 0)
        self.model = N.MODEL_AFFINE
        self.B = 2

    def run(self, **null):
        p = lambda name, arr: None if name in null else arr.ctypes.data
        cfg = None if "cfg" in null else C.addressof(self.cfg)
        return N.lib().cvFindModelBatch(self.model, p("a", self.a), p("b", self.b), p("offsets", self.offsets), self.B,
                                        cfg, p("models", self.models), p("mask", self.mask), p("counts", self.counts))


def _device_visible():
    return N.lib().mcvDeviceCount() > 0


@pytest.mark.parametrize("which", ["a", "b", "offsets", "models", "counts"])
def test_null_arguments_rejected(native, which):
    assert Call().run(**{which: True}) == -1
    assert "null" in native.last_error()


def test_bad_offsets_rejected(native):
    c = Call()
    c.B = -1
    assert c.run() == -1 and "negative B" in native.last_error()
    c = Call()
    c.offsets[0] = 1
    assert c.run() == -1 and "offsets[0]" in native.last_error()
    c = Call()
    c.offsets[:] = [0, 30, 20]
    assert c.run() == -1 and "decrease" in native.last_error() and "problem 1" in native.last_error()


@pytest.mark.parametrize("field,value,word", [
    ("method", N.METHOD_LSQ, "method"), ("method", N.METHOD_LMEDS, "method"), ("method", 3, "method"),
    ("flags", N.FLAG_FUSED_ERROR, "MCV_FLAG_FUSED_ERROR"), ("flags", N.FLAG_FAST_MINIMAL, "MCV_FLAG_FAST_MINIMAL"),
    ("flags", N.FLAG_SEVEN_POINT, "MCV_FLAG_SEVEN_POINT"), ("flags", 4, "bit 4"),
    ("flags", N.FLAG_CV_SAMPLER | N.FLAG_FUSED_ERROR, "MCV_FLAG_FUSED_ERROR"),
    ("deviceCount", 2, "deviceCount"), ("confidence", 1.0, "confidence"), ("confidence", 0.0, "confidence")])
def test_unsupported_configuration_rejected(native, field, value, word):
    for model in MODELS:
        c = Call()
        c.model = model
        setattr(c.cfg, field, value)
        assert c.run() == -1
        assert word in native.last_error() and "cvFindModelBatch" in native.last_error()


@pytest.mark.parametrize("model", [N.MODEL_ESSENTIAL, N.MODEL_PNP, -1, 6])
def test_other_models_rejected(native, model):
    c = Call()
    c.model = model
    assert c.run() == -1 and "model" in native.last_error()
    with pytest.raises(N.NativeError, match="model"):
        opencv.findModelBatch(model, [c.a[:20]], [c.b[:20]])


def test_checks_run_before_the_device(native):
    """The refusals above never reach the device: they are the same with and without a GPU. A valid call
    without a GPU fails with the no-device message, an empty batch succeeds."""
    c = Call()
    c.B = 0
    assert c.run() == 0 and native.last_error() == ""
    assert opencv.findModelBatch(N.MODEL_HOMOGRAPHY, [], []) == []
    if _device_visible():
        return   # the valid call is the GPU suite's subject
    for model in MODELS:
        for cfg_null in (False, True):
            c = Call()
            c.model = model
            assert c.run(**({"cfg": True} if cfg_null else {})) == -1
            assert "no HIP device" in native.last_error()
    with pytest.raises(N.NativeError, match="no HIP device"):
        opencv.findModelBatch(N.MODEL_AFFINE, [c.a[:20], c.a[20:]], [c.b[:20], c.b[20:]])


# ---- the layout ------------------------------------------------------------------------------------
def _layout(sizes, m, max_iters, cap):
    B = len(sizes)
    offsets = np.zeros(B + 1, dtype=np.int32)
    offsets[1:] = np.cumsum(sizes)
    desc = np.full((max(B, 1), 4), -7, dtype=np.int64)
    info = np.full(4, -7, dtype=np.int64)
    D = N.lib().mcvHostBatchLayout(offsets.ctypes.data, B, m, max_iters, cap, desc.ctypes.data, info.ctypes.data)
    assert D >= 0, N.last_error()
    return D, desc[:B], info, offsets


def _expected(sizes, m, max_iters, cap):
    """The definition, in Python integers."""
    iters = max(max_iters, 1)
    dev = [p for p, n in enumerate(sizes) if n > m]
    D = len(dev)
    per = min(max(cap // D, 1), iters) if D else iters
    rounds = -(-iters // per) if D else 0
    desc, off = [], 0
    for p, n in enumerate(sizes):
        d = dev.index(p) if p in dev else None
        desc.append([off, n, -1 if d is None else d * per, -1 if d is None else d * iters])
        off += n
    return D, desc, [D, per, rounds, D * per]


@pytest.mark.parametrize("m", [2, 3, 4, 8])
def test_layout_mixed_sizes(native, m):
    sizes = [9, 10, 0, 63, m, m - 1, 64, 0, 65, m + 1, 1001]   # odd and even N, empty, N == m, N < m
    D, desc, info, offsets = _layout(sizes, m, 2000, 1 << 21)
    eD, edesc, einfo = _expected(sizes, m, 2000, 1 << 21)
    assert D == eD == sum(n > m for n in sizes)
    assert desc.tolist() == edesc and info.tolist() == einfo
    assert info[2] == 1                                   # everything fits one round
    np.testing.assert_array_equal(desc[:, 0], offsets[:-1])   # float4 points: nothing is padded
    # the slices and the slot ranges of the device problems are disjoint and in order
    dev = desc[desc[:, 2] >= 0]
    assert (np.diff(dev[:, 2]) == info[1]).all() and (np.diff(dev[:, 3]) == 2000).all()


def test_layout_slot_offsets_past_2_31(native):
    sizes = [100] * 5
    iters = 1 << 30
    D, desc, info, _ = _layout(sizes, 4, iters, 1 << 40)
    assert D == 5 and info[1] == iters and info[2] == 1
    assert desc[:, 2].tolist() == [d * iters for d in range(5)]
    assert desc[:, 3].tolist() == [d * iters for d in range(5)]
    assert desc[2, 2] == 1 << 31 and desc[4, 2] == 1 << 32 and info[3] == 5 << 30


@pytest.mark.parametrize("delta,rounds", [(-1, 2), (0, 1), (1, 1)])
def test_layout_round_split_at_the_cap(native, delta, rounds):
    """D x maxIters slots against cap = D x maxIters + delta: one round from the cap on, two just below."""
    sizes = [50, 3, 60, 70]    # three device problems at m = 4
    iters = 1000
    cap = 3 * iters + delta
    D, desc, info, _ = _layout(sizes, 4, iters, cap)
    assert D == 3
    assert info.tolist() == _expected(sizes, 4, iters, cap)[2]
    assert info[2] == rounds
    assert info[1] == (iters if delta >= 0 else (3 * iters - 1) // 3)
    assert info[1] * info[2] >= iters > info[1] * (info[2] - 1)   # the rounds cover the budget, none is empty
    assert info[3] <= max(cap, D)


def test_layout_small_caps_and_defaults(native):
    sizes = [30, 31, 32]
    D, desc, info, _ = _layout(sizes, 2, 10, 2)      # cap below the problem count: one hypothesis each
    assert info.tolist() == [3, 1, 10, 3]
    D, desc, info, _ = _layout(sizes, 2, 0, 1 << 21)  # maxIters 0 evaluates one hypothesis, as the single call
    assert info.tolist() == [3, 1, 1, 3]
    D, desc, info, _ = _layout(sizes, 2, 2000, 0)     # cap <= 0: the export's own cap, 2^21 slots
    assert info.tolist() == _expected(sizes, 2, 2000, 1 << 21)[2]
    D, desc, info, _ = _layout([2000] * 2000, 2, 2000, 0)
    assert info.tolist() == _expected([2000] * 2000, 2, 2000, 1 << 21)[2] and info[2] == 2


def test_layout_empty_batch(native):
    D, desc, info, _ = _layout([], 4, 2000, 1 << 21)
    assert D == 0 and info.tolist() == [0, 2000, 0, 0]
    D, desc, info, _ = _layout([3, 0, 4], 4, 2000, 1 << 21)   # no problem reaches the device
    assert D == 0 and info[2] == 0 and (desc[:, 2:] == -1).all()


def test_batch_cap_hook_round_trip(native):
    L = native.lib()
    prev = L.mcvTestBatchCap(12345)
    try:
        assert L.mcvTestBatchCap(0) == 12345
        assert L.mcvTestBatchCap(-5) == 1 << 21
    finally:
        L.mcvTestBatchCap(prev)
    assert prev == 1 << 21


# ---- the plan of a hypothesis round ------------------------------------------------------------------
SIZES3 = np.array([30, 7, 64], dtype=np.int32)            # three device problems
PT3 = np.array([0, 30, 37], dtype=np.int32)
ROW3 = np.array([0, 10, 20], dtype=np.int64)


def _round(pt_off, n, row_off, niters, stopped, active, begin, size):
    """mcvHostBatchRound on numpy arrays: (the round's device indices, its descriptors, stride)."""
    D, nA = len(n), len(active)
    niters = np.ascontiguousarray(niters, dtype=np.int64)
    stopped = np.ascontiguousarray(stopped, dtype=np.int32)
    active = np.ascontiguousarray(active, dtype=np.int32)
    desc = np.full((max(nA, 1), 6), -7, dtype=np.int64)
    out = np.full(max(nA, 1), -7, dtype=np.int32)
    info = np.full(2, -7, dtype=np.int64)
    k = N.lib().mcvHostBatchRound(pt_off.ctypes.data, n.ctypes.data, row_off.ctypes.data, niters.ctypes.data,
                                  stopped.ctypes.data, D, active.ctypes.data, nA, begin, size, desc.ctypes.data,
                                  out.ctypes.data, info.ctypes.data)
    assert k >= 0, N.last_error()
    assert info[0] == k and (desc[k:] == -7).all() and (out[k:] == -7).all()   # nothing past the round is written
    return out[:k].tolist(), desc[:k], int(info[1])


def _expected_round(pt_off, n, row_off, niters, stopped, active, begin, size):
    """The definition, in numpy."""
    a = np.asarray(active, dtype=np.int64)
    niters, stopped = np.asarray(niters, dtype=np.int64), np.asarray(stopped)
    keep = a[(stopped[a] == 0) & (niters[a] - begin > 0)]
    cnt = np.minimum(niters[keep] - begin, size)
    stride = int(cnt.max()) if len(keep) else 0
    desc = np.stack([pt_off[keep], n[keep], np.full(len(keep), begin), cnt, np.arange(len(keep)) * stride,
                     row_off[keep]], axis=1).astype(np.int64).reshape(len(keep), 6)
    return keep.tolist(), desc, stride


def _walk(pt_off, n, row_off, niters, stopped, sizes, after_round=None):
    """Rounds of the given sizes from begin = 0 on, the active list carried along as the driver does; returns
    every round's hypothesis counts. after_round(r, niters, stopped) plays the replay's part."""
    niters, stopped = np.array(niters, dtype=np.int64), np.array(stopped, dtype=np.int32)
    active, begin, seen = list(range(len(n))), 0, []
    for r, size in enumerate(sizes):
        got = _round(pt_off, n, row_off, niters, stopped, active, begin, size)
        exp = _expected_round(pt_off, n, row_off, niters, stopped, active, begin, size)
        assert got[0] == exp[0] and got[2] == exp[2]
        np.testing.assert_array_equal(got[1], exp[1])
        assert got[2] == (int(got[1][:, 3].max()) if got[0] else 0)      # the stride is the largest count
        seen.append(got[1][:, 3].tolist())
        active, begin = got[0], begin + size
        if after_round:
            after_round(r, niters, stopped)
    return seen, active


def test_round_plan_splits_the_budget(native):
    seen, active = _walk(PT3, SIZES3, ROW3, [10] * 3, [0] * 3, [4, 4, 4, 4])
    assert seen == [[4] * 3, [4] * 3, [2] * 3, []] and active == []


def test_round_plan_follows_a_lowered_budget(native):
    def lower(r, niters, stopped):
        if r == 0:
            niters[1] = 5
    seen, active = _walk(PT3, SIZES3, ROW3, [10] * 3, [0] * 3, [4, 4, 4], lower)
    assert seen == [[4, 4, 4], [4, 1, 4], [2, 2]] and active == [0, 2]


def test_round_plan_drops_a_stopped_problem(native):
    seen, active = _walk(PT3, SIZES3, ROW3, [10] * 3, [0, 1, 0], [4, 4])
    assert seen == [[4, 4], [4, 4]] and active == [0, 2]
    ids, desc, stride = _round(PT3, SIZES3, ROW3, [10] * 3, [0, 1, 0], [0, 1, 2], 0, 4)
    assert desc[:, 0].tolist() == [0, 37] and desc[:, 4].tolist() == [0, 4] and desc[:, 5].tolist() == [0, 20]


def test_round_plan_smaller_first_round(native):
    seen, active = _walk(PT3, SIZES3, ROW3, [10] * 3, [0] * 3, [2, 4, 4, 4])
    assert seen == [[2] * 3, [4] * 3, [4] * 3, []]


def test_round_plan_single_problem_and_all_stopped(native):
    one = (PT3[:1], SIZES3[:1], ROW3[:1])
    seen, _ = _walk(*one, [10], [0], [4, 4, 4, 4])
    assert seen == [[4], [4], [2], []]
    ids, desc, stride = _round(PT3, SIZES3, ROW3, [10] * 3, [1] * 3, [0, 1, 2], 0, 4)
    assert ids == [] and len(desc) == 0 and stride == 0
    ids, desc, stride = _round(PT3, SIZES3, ROW3, [10] * 3, [0] * 3, [], 0, 4)
    assert ids == [] and stride == 0


def test_round_plan_refuses_bad_arguments(native):
    L = N.lib()
    nit, stp = np.full(3, 10, dtype=np.int64), np.zeros(3, dtype=np.int32)
    act = np.arange(3, dtype=np.int32)
    desc, out, info = np.zeros((3, 6), dtype=np.int64), np.zeros(3, dtype=np.int32), np.zeros(2, dtype=np.int64)

    def call(pt=PT3, n=SIZES3, niters=nit, stopped=stp, D=3, active=act, nA=3, begin=0, size=4, desc=desc, out=out,
             info=info):
        p = lambda a: None if a is None else a.ctypes.data
        return L.mcvHostBatchRound(p(pt), p(n), p(ROW3), p(niters), p(stopped), D, p(active), nA, begin, size, p(desc),
                                   p(out), p(info))

    assert call() == 3
    for null in ("pt", "n", "niters", "stopped", "active", "desc", "out", "info"):
        assert call(**{null: None}) == -1 and "mcvHostBatchRound" in native.last_error()
    for bad in (dict(D=-1), dict(nA=-1), dict(nA=4), dict(begin=-1), dict(begin=1 << 31), dict(size=0),
                dict(size=1 << 31)):
        assert call(**bad) == -1
    for lst in ([0, 2, 1], [0, 1, 1], [0, 1, 3], [-1, 0, 1]):
        assert call(active=np.array(lst, dtype=np.int32)) == -1 and "ascending" in native.last_error()


def test_index_code_under_sanitizers(tmp_path):
    """tests/asan/ransac_batch_index_asan_main.cpp: a stand-alone program (its own main, nothing preloaded,
    nothing loaded into Python) over ransac_batch_index.h, built with -fsanitize=address,undefined."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "ransac_batch_index_asan"
    src = N.ROOT / "tests" / "asan" / "ransac_batch_index_asan_main.cpp"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{N.ROOT / 'minicv_amd' / 'csrc'}", str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ransac_batch_index_asan ok" in r.stdout and "ERROR" not in r.stderr
