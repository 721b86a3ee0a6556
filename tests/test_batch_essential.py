"""CPU tests of cvFindEssentialMatBatch / cvRecoverPoseBatch (B independent essential-matrix problems in one
call): every argument check runs before the device is touched, and the index arithmetic of a call
(mcvHostBatchLayout with m = 5 and the family's cap of 2^18 hypotheses per round) is checked against its
definition."""
import ctypes as C

import numpy as np
import pytest

from minicv_amd import native as N
from minicv_amd import opencv

CAP = N.BATCH_E_HYP_CAP


class FindCall:
    """One well-formed cvFindEssentialMatBatch call (two problems of 20 points), fields replaceable."""
    name = "cvFindEssentialMatBatch"

    def __init__(self):
        rng = np.random.default_rng(1)
        self.a = np.ascontiguousarray(rng.uniform(0, 100, (40, 2)))
        self.b = np.ascontiguousarray(rng.uniform(0, 100, (40, 2)))
        self.offsets = np.array([0, 20, 40], dtype=np.int32)
        self.focal = np.array([800.0, 700.0])
        self.pp = np.array([[640.0, 360.0], [600.0, 300.0]])
        self.E = np.zeros((2, 9))
        self.mask = np.zeros(40, dtype=np.uint8)
        self.counts = np.zeros(2, dtype=np.int32)
        self.cfg = N.RansacConfig(1.0, 0.999, 100, N.METHOD_RANSAC, 1, 1, 0, 0, 0)
        self.B = 2

    def run(self, **null):
        p = lambda name, arr: None if name in null else arr.ctypes.data
        cfg = None if "cfg" in null else C.addressof(self.cfg)
        return N.lib().cvFindEssentialMatBatch(p("a", self.a), p("b", self.b), p("offsets", self.offsets), self.B,
                                               p("focal", self.focal), p("pp", self.pp), cfg, p("E", self.E),
                                               p("mask", self.mask), p("counts", self.counts))


class PoseCall:
    """One well-formed cvRecoverPoseBatch call."""
    name = "cvRecoverPoseBatch"

    def __init__(self):
        rng = np.random.default_rng(2)
        self.a = np.ascontiguousarray(rng.uniform(0, 100, (40, 2)))
        self.b = np.ascontiguousarray(rng.uniform(0, 100, (40, 2)))
        self.offsets = np.array([0, 20, 40], dtype=np.int32)
        self.configs = (N.RecoverPoseConfig * 2)(N.RecoverPoseConfig(800.0, N.V2d(640.0, 360.0), 0.999, 1.0),
                                                 N.RecoverPoseConfig(700.0, N.V2d(600.0, 300.0), 0.99, 2.0))
        self.R = np.zeros((2, 9))
        self.t = np.zeros((2, 3))
        self.ms = np.zeros(40, dtype=np.uint8)
        self.good = np.zeros(2, dtype=np.int32)
        self.B = 2

    def run(self, **null):
        p = lambda name, arr: None if name in null else arr.ctypes.data
        cfgs = None if "configs" in null else C.addressof(self.configs)
        return N.lib().cvRecoverPoseBatch(cfgs, p("a", self.a), p("b", self.b), p("offsets", self.offsets), self.B,
                                          p("R", self.R), p("t", self.t), p("ms", self.ms), p("good", self.good))


def _device_visible():
    return N.lib().mcvDeviceCount() > 0


@pytest.mark.parametrize("which", ["a", "b", "offsets", "focal", "pp", "E", "counts"])
def test_find_null_arguments_rejected(native, which):
    assert FindCall().run(**{which: True}) == -1
    assert "null" in native.last_error() and FindCall.name in native.last_error()


@pytest.mark.parametrize("which", ["configs", "a", "b", "offsets", "R", "t", "ms", "good"])
def test_pose_null_arguments_rejected(native, which):
    assert PoseCall().run(**{which: True}) == -1
    assert "null" in native.last_error() and PoseCall.name in native.last_error()


@pytest.mark.parametrize("call", [FindCall, PoseCall])
def test_bad_offsets_rejected(native, call):
    c = call()
    c.B = -1
    assert c.run() == -1 and "negative B" in native.last_error()
    c = call()
    c.offsets[0] = 1
    assert c.run() == -1 and "offsets[0]" in native.last_error()
    c = call()
    c.offsets[:] = [0, 30, 20]
    assert c.run() == -1 and "decrease" in native.last_error() and "problem 1" in native.last_error()
    assert call.name in native.last_error()


@pytest.mark.parametrize("field,value,word", [
    ("method", N.METHOD_LSQ, "method"), ("method", N.METHOD_LMEDS, "method"), ("method", 3, "method"),
    ("flags", N.FLAG_FUSED_ERROR, "MCV_FLAG_FUSED_ERROR"), ("flags", N.FLAG_FAST_MINIMAL, "MCV_FLAG_FAST_MINIMAL"),
    ("flags", 4, "bit 4"), ("flags", N.FLAG_CV_SAMPLER | N.FLAG_FUSED_ERROR, "MCV_FLAG_FUSED_ERROR"),
    ("flags", N.FLAG_FIXED_ITERS | N.FLAG_FAST_MINIMAL, "MCV_FLAG_FAST_MINIMAL"),
    ("deviceCount", 2, "deviceCount"), ("confidence", 1.0, "confidence"), ("confidence", 0.0, "confidence"),
    ("confidence", float("nan"), "confidence")])
def test_unsupported_configuration_rejected(native, field, value, word):
    c = FindCall()
    setattr(c.cfg, field, value)
    assert c.run() == -1
    assert word in native.last_error() and FindCall.name in native.last_error()


@pytest.mark.parametrize("prob", [0.0, 1.0, 1.5, -0.1, float("nan")])
def test_pose_confidence_rejected(native, prob):
    c = PoseCall()
    c.configs[1].Probability = prob
    assert c.run() == -1
    assert "confidence" in native.last_error() and "problem 1" in native.last_error()
    with pytest.raises(N.NativeError, match="confidence"):
        opencv.recoverPoseBatch(list(c.configs), [c.a[:20], c.a[20:]], [c.b[:20], c.b[20:]])


def test_checks_run_before_the_device(native):
    """The refusals above never reach the device: they are the same with and without a GPU. A valid call
    without a GPU fails with the no-device message, an empty batch succeeds."""
    for call in (FindCall, PoseCall):
        c = call()
        c.B = 0
        assert c.run() == 0 and native.last_error() == ""
    assert opencv.findEssentialMatBatch([], [], [], []) == []
    assert opencv.recoverPoseBatch([], [], []) == []
    assert opencv.recoverPoseBatch(opencv.recoverPoseConfig(), [], []) == []
    if _device_visible():
        return   # the valid call is the GPU suite's subject
    for cfg_null in (False, True):
        assert FindCall().run(**({"cfg": True} if cfg_null else {})) == -1
        assert "no HIP device" in native.last_error()
    assert PoseCall().run() == -1 and "no HIP device" in native.last_error()
    c = FindCall()
    with pytest.raises(N.NativeError, match="no HIP device"):
        opencv.findEssentialMatBatch([c.a[:20], c.a[20:]], [c.b[:20], c.b[20:]], c.focal, c.pp)


def test_accepted_flags_reach_the_device_check(native):
    """NO_REFINE, FIXED_ITERS and CV_SAMPLER are supported: such a call is not refused by the argument checks
    (without a GPU it gets as far as the no-device message)."""
    if _device_visible():
        return   # the accepted flags are the GPU suite's subject
    for flags in (N.FLAG_NO_REFINE, N.FLAG_FIXED_ITERS, N.FLAG_CV_SAMPLER,
                  N.FLAG_NO_REFINE | N.FLAG_FIXED_ITERS | N.FLAG_CV_SAMPLER):
        c = FindCall()
        c.cfg.flags = flags
        assert c.run() == -1 and "no HIP device" in native.last_error()


def test_wrapper_argument_shapes(native):
    a = np.zeros((6, 2))
    with pytest.raises(ValueError):
        opencv.findEssentialMatBatch([a], [a, a], [1.0], [(0, 0)])
    with pytest.raises(ValueError):
        opencv.findEssentialMatBatch([a], [a], [1.0, 2.0], [(0, 0)])
    with pytest.raises(ValueError):
        opencv.findEssentialMatBatch([a], [a[:5]], [1.0], [(0, 0)])
    with pytest.raises(ValueError):
        opencv.recoverPoseBatch([opencv.recoverPoseConfig()] * 2, [a], [a])


def test_exports_declared(native):
    txt = (N.ROOT / "include" / "minicv_native.h").read_text()
    for name in ("cvFindEssentialMatBatch", "cvRecoverPoseBatch", "mcvTestBatchSweepE"):
        assert name in N.SIGNATURES and getattr(native.lib(), name) is not None
        assert f"MCV_API int {name}(" in txt


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


def test_layout_mixed_sizes(native):
    sizes = [9, 6, 0, 63, 5, 4, 64, 0, 65, 1, 601, 5]   # N < 5, N == 5, N > 5, empty
    D, desc, info, offsets = _layout(sizes, 5, 1000, CAP)
    eD, edesc, einfo = _expected(sizes, 5, 1000, CAP)
    assert D == eD == sum(n > 5 for n in sizes) == 6
    assert desc.tolist() == edesc and info.tolist() == einfo
    assert info[1] == 1000 and info[2] == 1               # everything fits one round
    np.testing.assert_array_equal(desc[:, 0], offsets[:-1])   # nothing is padded
    dev = desc[desc[:, 2] >= 0]
    assert (np.diff(dev[:, 2]) == 1000).all() and (np.diff(dev[:, 3]) == 1000).all()
    assert (desc[[2, 4, 5, 7, 9, 11], 2:] == -1).all()    # the problems that never reach the device


def test_layout_default_budget_fits_one_round(native):
    """B = 256 problems of the default 1000 iterations are one round under the cap of 2^18; 263 are two."""
    D, _, info, _ = _layout([200] * 256, 5, 1000, CAP)
    assert info.tolist() == [256, 1000, 1, 256000]
    D, _, info, _ = _layout([200] * 263, 5, 1000, CAP)
    assert info.tolist() == _expected([200] * 263, 5, 1000, CAP)[2] and info[2] == 2 and info[1] == CAP // 263


@pytest.mark.parametrize("delta,rounds", [(-1, 2), (0, 1), (1, 1)])
def test_layout_round_split_at_the_cap(native, delta, rounds):
    """D x maxIters hypotheses against cap = 2^18 + delta: one round from the cap on, two just below."""
    D0, iters = 256, 1024                    # 256 x 1024 = 2^18 hypotheses
    sizes = [50, 5, 3] + [60] * (D0 - 1)     # 256 device problems at m = 5
    cap = CAP + delta
    D, desc, info, _ = _layout(sizes, 5, iters, cap)
    assert D == D0
    assert info.tolist() == _expected(sizes, 5, iters, cap)[2]
    assert info[2] == rounds
    assert info[1] == (iters if delta >= 0 else iters - 1)
    assert info[1] * info[2] >= iters > info[1] * (info[2] - 1)   # the rounds cover the budget, none is empty
    assert info[3] <= cap


def test_layout_small_caps(native):
    sizes = [30, 31, 32]
    D, desc, info, _ = _layout(sizes, 5, 10, 2)      # cap below the problem count: one hypothesis each
    assert info.tolist() == [3, 1, 10, 3]
    D, desc, info, _ = _layout(sizes, 5, 0, CAP)     # maxIters 0 evaluates one hypothesis, as the single call
    assert info.tolist() == [3, 1, 1, 3]
    D, desc, info, _ = _layout([5, 4, 0], 5, 1000, CAP)   # no problem reaches the device
    assert D == 0 and info[2] == 0 and (desc[:, 2:] == -1).all()
