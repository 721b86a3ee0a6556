"""CPU tests of cvMatchFeaturesBatch / cvMatchAndFindModelBatch (the matches of many image pairs in one
call): every argument check runs before the device is touched and names the export, and the index
arithmetic of a call (mcvHostMatchBatchLayout: directed problems, workgroup table) is checked against its
definition."""
import ctypes as C

import numpy as np
import pytest

from minicv_amd import native as N
from minicv_amd import opencv

SIZES = [0, 1, 2, 31, 32, 33, 127, 128, 129, 257]


def _features(n, width=32, dtype=np.uint8, seed=0):
    rng = np.random.default_rng(seed + n)
    d = rng.integers(0, 256, size=(n, width)).astype(dtype)
    return opencv.Features(rng.uniform(0, 100, (n, 2)), d)


class Call:
    """One well-formed call (three images, two pairs), fields replaceable one at a time."""

    def __init__(self, fused):
        self.fused = fused
        self.images = [_features(20), _features(30), _features(25)]
        self.ip = np.array([[0, 1], [2, 0]], dtype=np.int32)
        self.B = 2
        self.nImages = 3
        self.maxPairs = 45
        self.pairs = np.zeros((45, 2), dtype=np.int32)
        self.dist = np.zeros(45, dtype=np.float32)
        self.offsets = np.zeros(3, dtype=np.int32)
        self.models = np.zeros((2, 9))
        self.mask = np.zeros(45, dtype=np.uint8)
        self.counts = np.zeros(2, dtype=np.int32)
        self.mcfg = N.MatchConfig(0.8, 0, 0.0, N.MODEL_HOMOGRAPHY)
        self.rcfg = N.RansacConfig(3.0, 0.99, 100, N.METHOD_RANSAC, 1, 1, 0, 0, 0)
        self.norm = N.NORM_AUTO

    @property
    def name(self):
        return "cvMatchAndFindModelBatch" if self.fused else "cvMatchFeaturesBatch"

    def run(self, **null):
        structs = (N.DetectorResult * len(self.images))(*[f.struct for f in self.images])
        p = lambda name, arr: None if name in null else arr.ctypes.data
        images = None if "images" in null else C.addressof(structs)
        mcfg = None if "mcfg" in null else C.addressof(self.mcfg)
        if self.fused:
            return N.lib().cvMatchAndFindModelBatch(
                images, self.nImages, p("imagePairs", self.ip), self.B, mcfg, self.norm, C.addressof(self.rcfg),
                p("pairs", self.pairs), self.maxPairs, p("offsets", self.offsets), p("models", self.models),
                p("mask", self.mask), p("counts", self.counts))
        return N.lib().cvMatchFeaturesBatch(images, self.nImages, p("imagePairs", self.ip), self.B, mcfg, self.norm,
                                            p("pairs", self.pairs), p("dist", self.dist), self.maxPairs,
                                            p("offsets", self.offsets))

    def refused(self, native, word, **null):
        assert self.run(**null) == -1
        err = native.last_error()
        assert self.name in err and word in err, err
        return err


FUSED = [False, True]


@pytest.mark.parametrize("fused", FUSED)
@pytest.mark.parametrize("which", ["images", "imagePairs", "pairs", "offsets"])
def test_null_arguments_rejected(native, fused, which):
    Call(fused).refused(native, "null", **{which: True})


@pytest.mark.parametrize("which", ["models", "mask", "counts"])
def test_fused_null_outputs_rejected(native, which):
    Call(True).refused(native, "null", **{which: True})


@pytest.mark.parametrize("fused", FUSED)
def test_bad_image_index_rejected(native, fused):
    for bad in (-1, 3):
        c = Call(fused)
        c.ip[1, 1] = bad
        err = c.refused(native, "problem 1")
        assert "image %d" % bad in err


@pytest.mark.parametrize("fused", FUSED)
def test_mixed_widths_and_types_rejected(native, fused):
    c = Call(fused)
    c.images[2] = _features(25, width=64)
    c.refused(native, "mixed descriptor widths")
    c = Call(fused)
    c.images[1] = _features(30, dtype=np.float32)
    c.refused(native, "mixed descriptor element types")
    c = Call(fused)
    c.images = [_features(n, dtype=np.float32) for n in (20, 30, 25)]
    err = c.refused(native, "float32")
    assert "cvMatchFeaturesNorm" in err      # the message names the single call that serves float32
    c = Call(fused)
    c.images[1].struct.DescriptorEntries += 1
    c.refused(native, "not a multiple")


@pytest.mark.parametrize("fused", FUSED)
def test_norm_and_sizes_rejected(native, fused):
    for norm in (1, 2, 5, 7, -1):
        c = Call(fused)
        c.norm = norm
        c.refused(native, "norm %d" % norm)
    c = Call(fused)
    c.B = -1
    c.refused(native, "negative B")
    c = Call(fused)
    c.maxPairs = -1
    c.refused(native, "negative maxPairs")
    c = Call(fused)
    c.nImages = -1
    c.refused(native, "negative nImages")
    c = Call(fused)
    c.images = [_features(n, width=65) for n in (20, 30, 25)]     # Hamming: at most 64 bytes
    c.refused(native, "65")
    c = Call(fused)
    c.norm = N.NORM_L2
    c.images = [_features(n, width=513) for n in (20, 30, 25)]    # byte SIFT: at most 512
    c.refused(native, "513")


@pytest.mark.parametrize("model", [N.MODEL_ESSENTIAL, N.MODEL_PNP, -1, 6])
def test_fused_unsupported_model_rejected(native, model):
    c = Call(True)
    c.mcfg.model = model
    c.refused(native, "model")


@pytest.mark.parametrize("field,value,word", [
    ("method", N.METHOD_LMEDS, "method"), ("method", N.METHOD_LSQ, "method"), ("deviceCount", 2, "deviceCount"),
    ("flags", N.FLAG_FUSED_ERROR, "MCV_FLAG_FUSED_ERROR"), ("flags", 4, "bit 4"), ("confidence", 1.0, "confidence")])
def test_fused_rejects_what_find_model_batch_rejects(native, field, value, word):
    for model in (N.MODEL_HOMOGRAPHY, N.MODEL_FUNDAMENTAL, N.MODEL_AFFINE, N.MODEL_SIMILARITY):
        c = Call(True)
        c.mcfg.model = model
        setattr(c.rcfg, field, value)
        err = c.refused(native, word)
        assert "cvFindModelBatch" in err


@pytest.mark.parametrize("fused", FUSED)
def test_checks_run_before_the_device(native, fused):
    """The refusals above are the same with and without a GPU. An empty batch and a batch of empty images
    succeed without one; a valid call without a GPU fails with the no-device message."""
    c = Call(fused)
    c.B = 0
    c.offsets[:] = -7
    assert c.run() == 0 and native.last_error() == "" and c.offsets[0] == 0
    if not fused:    # (the fused call goes on to cvFindModelBatch, which needs a device for B > 0)
        c = Call(fused)
        c.images = [_features(0), _features(0), _features(0)]
        c.offsets[:] = -7
        assert c.run() == 0 and c.offsets.tolist() == [0, 0, 0]
    assert opencv.matchFeaturesBatch([], []) == []
    if native.lib().mcvDeviceCount() > 0:
        return   # the valid call is the GPU suite's subject
    for cfg_null in (False, True):
        c = Call(fused)
        assert c.run(**({"mcfg": True} if cfg_null else {})) == -1
        assert "no HIP device" in native.last_error()
    with pytest.raises(N.NativeError, match="no HIP device"):
        opencv.matchFeaturesBatch(Call(False).images, [(0, 1)])
    with pytest.raises(N.NativeError, match="float32"):
        opencv.matchFeaturesBatch([_features(5, dtype=np.float32)] * 2, [(0, 1)])


# ---- the layout ------------------------------------------------------------------------------------
def _layout(counts, pairs, cross, norm):
    counts = np.asarray(counts, dtype=np.int32)
    ip = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    B = ip.shape[0]
    info = np.full(4, -7, dtype=np.int32)
    G = N.lib().mcvHostMatchBatchLayout(counts.ctypes.data, len(counts), ip.ctypes.data, B, int(cross), norm, None,
                                        info.ctypes.data, None, 0)
    assert G >= 0, N.last_error()
    D = (2 if cross else 1) * B
    prob = np.full((max(D, 1), 5), -7, dtype=np.int32)
    wg = np.full((max(G, 1), 2), -7, dtype=np.int32)
    G2 = N.lib().mcvHostMatchBatchLayout(counts.ctypes.data, len(counts), ip.ctypes.data, B, int(cross), norm,
                                         prob.ctypes.data, info.ctypes.data, wg.ctypes.data, G)
    assert G2 == G and info[0] == D and info[2] == G
    return prob[:D], info, wg[:G]


def _expected(counts, pairs, cross, rows):
    """The definition, in Python integers, from the rows-per-workgroup value the hook reports."""
    directed = [(i, j) for i, j in pairs] + ([(j, i) for i, j in pairs] if cross else [])
    prob, out = [], 0
    for i, j in directed:
        prob.append([i, j, counts[i], counts[j], out])
        out += counts[i]
    order = sorted(range(len(directed)), key=lambda d: (-prob[d][3], d))
    wg = [[d, t] for d in order for t in range(-(-prob[d][2] // rows))]
    return prob, wg, sum(counts[i] for i, _ in pairs)


@pytest.mark.parametrize("cross", [False, True])
@pytest.mark.parametrize("norm", [N.NORM_HAMMING, N.NORM_L2, N.NORM_AUTO])
def test_layout_against_definition(native, cross, norm):
    n = len(SIZES)
    pairs = [(i, j) for i in range(n) for j in range(n) if (i + 2 * j) % 3 != 1] + [(3, 3), (9, 9), (0, 0)]
    prob, info, wg = _layout(SIZES, pairs, cross, norm)
    rows = int(info[1])
    assert rows == (N.MATCH_BATCH_ROWS_L2 if norm == N.NORM_L2 else N.MATCH_BATCH_ROWS_HAMMING)
    eprob, ewg, total_q = _expected(SIZES, pairs, cross, rows)
    assert prob.tolist() == eprob
    assert wg.tolist() == ewg
    assert info[3] == total_q
    # every (problem, query tile) with nq > 0 exactly once, none for an empty query image
    seen = set(map(tuple, wg.tolist()))
    assert len(seen) == len(wg)
    want = {(d, t) for d, p in enumerate(eprob) for t in range(-(-p[2] // rows))}
    assert seen == want
    assert all(eprob[d][2] > 0 and t * rows < eprob[d][2] for d, t in seen)
    assert not any(eprob[d][2] == 0 for d, _ in seen)
    # large problems start first
    nt = [eprob[d][3] for d, _ in wg.tolist()]
    assert nt == sorted(nt, reverse=True)


def test_layout_edges(native):
    prob, info, wg = _layout([5, 0], [], False, N.NORM_HAMMING)
    assert info.tolist() == [0, N.MATCH_BATCH_ROWS_HAMMING, 0, 0] and len(wg) == 0
    prob, info, wg = _layout([0, 0], [(0, 1), (1, 0)], True, N.NORM_HAMMING)
    assert info[0] == 4 and info[2] == 0 and info[3] == 0
    prob, info, wg = _layout([64, 65], [(0, 1), (1, 0)], False, N.NORM_HAMMING)
    assert wg.tolist() == [[0, 0], [1, 0], [1, 1]]     # nt 65 first, then the two tiles of the 65 queries
    counts = np.array([3], dtype=np.int32)
    bad = np.array([0, 1], dtype=np.int32)
    info = np.zeros(4, dtype=np.int32)
    assert N.lib().mcvHostMatchBatchLayout(counts.ctypes.data, 1, bad.ctypes.data, 1, 0, N.NORM_HAMMING, None,
                                           info.ctypes.data, None, 0) == -1
