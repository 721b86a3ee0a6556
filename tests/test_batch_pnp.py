"""CPU tests of cvSolvePnPRansacBatch (B independent solvePnPRansac problems in one call): the export is
declared and exported, every argument check runs before the device is touched, and the index arithmetic of a
call (mcvHostBatchLayout with m = 4 for P3P / AP3P and m = 5 for the other kinds, under the family's cap of
2^18 hypotheses per round) is checked against its definition."""
import ctypes as C

import numpy as np
import pytest

from minicv_amd import native as N
from minicv_amd import opencv

CAP = N.BATCH_PNP_HYP_CAP
NAME = "cvSolvePnPRansacBatch"
K0 = [800.0, 0, 640.0, 0, 820.0, 360.0, 0, 0, 1.0]


class Call:
    """One well-formed cvSolvePnPRansacBatch call (two problems of 20 points), fields replaceable."""

    def __init__(self):
        rng = np.random.default_rng(1)
        self.img = np.ascontiguousarray(rng.uniform(0, 1000, (40, 2)))
        self.world = np.ascontiguousarray(rng.uniform(-3, 3, (40, 3)))
        self.offsets = np.array([0, 20, 40], dtype=np.int32)
        self.K = np.array([K0, K0], dtype=np.float64)
        self.dist = np.zeros((2, 4))
        self.t = np.zeros((2, 3))
        self.r = np.zeros((2, 3))
        self.mask = np.zeros(40, dtype=np.uint8)
        self.counts = np.zeros(2, dtype=np.int32)
        self.cfg = N.RansacConfig(8.0, 0.99, 100, N.METHOD_RANSAC, 1, 1, 0, 0, 5)
        self.B = 2

    def run(self, **null):
        p = lambda name, arr: None if name in null else arr.ctypes.data
        cfg = None if "cfg" in null else C.addressof(self.cfg)
        return N.lib().cvSolvePnPRansacBatch(p("img", self.img), p("world", self.world), p("offsets", self.offsets),
                                             self.B, p("K", self.K), p("dist", self.dist), cfg, p("t", self.t),
                                             p("r", self.r), p("mask", self.mask), p("counts", self.counts))


def _device_visible():
    return N.lib().mcvDeviceCount() > 0


def test_exports_declared(native):
    txt = (N.ROOT / "include" / "minicv_native.h").read_text()
    for name in (NAME, "mcvTestBatchSweepPnp"):
        assert name in N.SIGNATURES and getattr(native.lib(), name) is not None
        assert f"MCV_API int {name}(" in txt
    assert callable(opencv.solvePnPRansacBatch)
    import minicv_amd
    assert minicv_amd.solvePnPRansacBatch is opencv.solvePnPRansacBatch


def test_abi_version_unchanged(native):
    assert native.lib().mcvAbiVersion() == 3


@pytest.mark.parametrize("which", ["img", "world", "offsets", "K", "t", "r", "mask", "counts"])
def test_null_arguments_rejected(native, which):
    assert Call().run(**{which: True}) == -1
    assert "null" in native.last_error() and NAME in native.last_error()


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
    assert NAME in native.last_error()


@pytest.mark.parametrize("field,value,word", [
    ("method", N.METHOD_LSQ, "method"), ("method", N.METHOD_LMEDS, "method"), ("method", 3, "method"),
    ("flags", N.FLAG_FUSED_ERROR, "MCV_FLAG_FUSED_ERROR"), ("flags", N.FLAG_FAST_MINIMAL, "MCV_FLAG_FAST_MINIMAL"),
    ("flags", 4, "bit 4"), ("flags", N.FLAG_CV_SAMPLER | N.FLAG_FUSED_ERROR, "MCV_FLAG_FUSED_ERROR"),
    ("flags", N.FLAG_FIXED_ITERS | N.FLAG_FAST_MINIMAL, "MCV_FLAG_FAST_MINIMAL"),
    ("deviceCount", 2, "deviceCount"), ("confidence", 1.0, "confidence"), ("confidence", 0.0, "confidence"),
    ("confidence", -0.5, "confidence"), ("confidence", float("nan"), "confidence")])
def test_unsupported_configuration_rejected(native, field, value, word):
    c = Call()
    setattr(c.cfg, field, value)
    assert c.run() == -1
    assert word in native.last_error() and NAME in native.last_error()
    assert not c.counts.any() and not c.mask.any()


def test_checks_run_before_the_device(native):
    """The refusals above never reach the device: they are the same with and without a GPU. A valid call
    without a GPU fails with the no-device message, an empty batch succeeds."""
    c = Call()
    c.B = 0
    assert c.run() == 0 and native.last_error() == ""
    assert c.run(cfg=True, dist=True) == 0 and native.last_error() == ""
    assert opencv.solvePnPRansacBatch([], [], []) == []
    if _device_visible():
        return   # the valid call is the GPU suite's subject
    for null in ({}, {"cfg": True}, {"dist": True}):
        assert Call().run(**null) == -1
        assert "no HIP device" in native.last_error()
    for flags in (N.FLAG_NO_REFINE, N.FLAG_FIXED_ITERS, N.FLAG_CV_SAMPLER,
                  N.FLAG_NO_REFINE | N.FLAG_FIXED_ITERS | N.FLAG_CV_SAMPLER):
        for kind in range(6):
            c = Call()
            c.cfg.flags = flags
            c.cfg.pnpKind = kind
            assert c.run() == -1 and "no HIP device" in native.last_error()
    c = Call()
    with pytest.raises(N.NativeError, match="no HIP device"):
        opencv.solvePnPRansacBatch([c.img[:20], c.img[20:]], [c.world[:20], c.world[20:]], c.K)


def test_wrapper_argument_shapes(native):
    a, w = np.zeros((6, 2)), np.zeros((6, 3))
    with pytest.raises(ValueError):
        opencv.solvePnPRansacBatch([a], [w, w], [K0])
    with pytest.raises(ValueError):
        opencv.solvePnPRansacBatch([a], [w[:5]], [K0])
    with pytest.raises(ValueError):
        opencv.solvePnPRansacBatch([a], [w], [K0, K0])
    with pytest.raises(ValueError):
        opencv.solvePnPRansacBatch([a], [w], [K0], dists=np.zeros((2, 4)))


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


@pytest.mark.parametrize("m", [4, 5])
def test_layout_mixed_sizes(native, m):
    sizes = [9, 6, 0, 63, 5, 4, 64, 0, 3, 1, 601, 5, 513]   # N < 4, N == 4, N == 5, N > 5, empty
    D, desc, info, offsets = _layout(sizes, m, 100, CAP)
    eD, edesc, einfo = _expected(sizes, m, 100, CAP)
    assert D == eD == sum(n > m for n in sizes) == (8 if m == 4 else 6)
    assert desc.tolist() == edesc and info.tolist() == einfo
    assert info[1] == 100 and info[2] == 1               # everything fits one round
    np.testing.assert_array_equal(desc[:, 0], offsets[:-1])   # nothing is padded
    dev = desc[desc[:, 2] >= 0]
    assert (np.diff(dev[:, 2]) == 100).all() and (np.diff(dev[:, 3]) == 100).all()
    off_device = [p for p, n in enumerate(sizes) if n <= m]
    assert (desc[off_device, 2:] == -1).all()            # the problems that never reach the device
    assert (desc[[4, 11], 2] >= 0).all() == (m == 4)     # N == 5 runs RANSAC on the device with AP3P only


@pytest.mark.parametrize("m", [4, 5])
def test_layout_default_budget_fits_one_round(native, m):
    """B = 1024 problems of the default 100 iterations are one round under the cap of 2^18; 2622 are two."""
    D, _, info, _ = _layout([200] * 1024, m, 100, CAP)
    assert info.tolist() == [1024, 100, 1, 102400]
    D, _, info, _ = _layout([200] * 2622, m, 100, CAP)
    assert info.tolist() == _expected([200] * 2622, m, 100, CAP)[2] and info[2] == 2 and info[1] == CAP // 2622


@pytest.mark.parametrize("m", [4, 5])
@pytest.mark.parametrize("delta,rounds", [(-1, 2), (0, 1), (1, 1)])
def test_layout_round_split_at_the_cap(native, m, delta, rounds):
    """D x maxIters hypotheses against cap = 2^18 + delta: one round from the cap on, two just below."""
    D0, iters = 256, 1024                       # 256 x 1024 = 2^18 hypotheses
    sizes = [50, m, 3, 0] + [60] * (D0 - 1)     # 256 device problems
    cap = CAP + delta
    D, desc, info, _ = _layout(sizes, m, iters, cap)
    assert D == D0
    assert info.tolist() == _expected(sizes, m, iters, cap)[2]
    assert info[2] == rounds
    assert info[1] == (iters if delta >= 0 else iters - 1)
    assert info[1] * info[2] >= iters > info[1] * (info[2] - 1)   # the rounds cover the budget, none is empty
    assert info[3] <= cap


def test_layout_small_caps(native):
    sizes = [30, 31, 32]
    D, desc, info, _ = _layout(sizes, 4, 10, 2)      # cap below the problem count: one hypothesis each
    assert info.tolist() == [3, 1, 10, 3]
    D, desc, info, _ = _layout(sizes, 5, 0, CAP)     # maxIters 0 evaluates one hypothesis, as the single call
    assert info.tolist() == [3, 1, 1, 3]
    D, desc, info, _ = _layout([5, 4, 0, 3], 5, 100, CAP)   # no problem reaches the device
    assert D == 0 and info[2] == 0 and (desc[:, 2:] == -1).all()
    D, desc, info, _ = _layout([5, 4, 0, 3], 4, 100, CAP)   # AP3P: N == 5 does
    assert D == 1 and desc[0].tolist() == [0, 5, 0, 0]
