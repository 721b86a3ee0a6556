"""SIFT detection on the GPU: cvDetectFeatures against the host twin and the numpy
reference on the shared case list (tests/_sift_ref.py), every output bit equal; the Gaussian pyramid and
the candidates of a call against the reference's (mcvTestSiftStage); FeatureCount on tied responses; calls
of changing sizes and types on one thread and on two threads at once; the blob image; the call's launch
counts and its determinism; and detectFeatures -> matchAndFindModel end to end."""
import ctypes as C
import threading

import numpy as np
import pytest

import _sift_ref as R
from minicv_amd import native as N
from minicv_amd import opencv

pytestmark = pytest.mark.gpu
GPU, TWIN = "cvDetectFeatures", "mcvHostDetectFeatures"


def stats():
    st = (C.c_longlong * 8)()
    assert N.lib().mcvTestSiftStats(st) == 0
    return list(st)


def fixed_counts(img, cfg):
    return [N.sift_launches(img.shape[1], img.shape[0], cfg["OctaveLayers"], cfg["FeatureCount"]), N.SIFT_SYNCS,
            N.SIFT_COPIES, N.SIFT_MEMSETS]


def assert_counts(name, st):
    """The statistics of a call on case `name`: what it found, and what its size and configuration launch."""
    want = R.expected(name)
    cnt = want[2]
    assert st[4:] == [cnt["candidates"], cnt["refined"], cnt["oriented"], len(want[0])], (name, st)
    if N.sift_octaves(*R.image(name).shape[1::-1]) == 0:
        assert st[:4] == [0, 0, 0, 0], (name, st)
    else:
        assert st[:4] == fixed_counts(R.image(name), R.config(name)), (name, st)


@pytest.mark.parametrize("name", list(R.CASES))
def test_parity(native, gpu, name):
    want = R.expected(name)
    got = R.run_case(GPU, name)
    st = stats()
    R.assert_same(got, want, f"{name}: cvDetectFeatures against the reference")
    twin = R.run_case(TWIN, name)
    R.assert_same(got, (twin.keypoints, twin.descriptors), f"{name}: cvDetectFeatures against the twin")
    assert_counts(name, st)


def read_stage(what, dtype, items):
    """mcvTestSiftStage into a buffer of exactly `items` elements (one fewer is refused) -> the array."""
    L = N.lib()
    buf, cnt = np.zeros(items, dtype), C.c_longlong(-1)
    if items:
        assert L.mcvTestSiftStage(what, buf.ctypes.data, buf.nbytes - 1, C.byref(cnt)) == -1
        assert "too small" in N.last_error() and cnt.value == -1 and not buf.any()
    assert L.mcvTestSiftStage(what, buf.ctypes.data, buf.nbytes, C.byref(cnt)) == 0, N.last_error()
    assert cnt.value * (4 if what == 1 else 1) == items, (what, cnt.value, items)
    return buf


STAGE_CASES = ("texture_97x61", "narrow_24x9", "seam_257x33", "seam_129x65", "seam_128x32", "tall_9x300",
               "sigma_max_layers_1", "sigma_0_8", "layers_6")


@pytest.mark.parametrize("name", STAGE_CASES)
def test_stages(native, gpu, name):
    """The Gaussian pyramid of a call, float by float, and its candidates as a set, against the reference:
    a wrong tap, halo or seam names the first pyramid position it spoils."""
    octaves, cands = R.stages(name)
    R.run_case(GPU, name)
    st = stats()
    want = np.concatenate([G.reshape(-1) for G in octaves])
    pyr = read_stage(0, np.float32, want.size)
    bad = np.flatnonzero(pyr.view(np.uint32) != want.view(np.uint32))
    if bad.size:
        at = int(bad[0])
        for o, G in enumerate(octaves):
            if at < G.size:
                i, r, c = np.unravel_index(at, G.shape)
                raise AssertionError(f"{name}: pyramid differs first at octave {o}, image {int(i)}, row {int(r)}, "
                                     f"column {int(c)} of {G.shape[2]} x {G.shape[1]}: got {pyr[bad[0]]!r}, "
                                     f"reference {want[bad[0]]!r}; {bad.size} of {want.size} floats differ")
            at -= G.size
    got = [tuple(q) for q in read_stage(1, np.int32, 4 * len(cands)).reshape(-1, 4).tolist()]
    assert len(set(got)) == len(got), (name, "a candidate twice")
    assert sorted(got) == sorted(cands), (name, sorted(set(got) ^ set(cands))[:5])
    assert stats() == st, (name, "mcvTestSiftStage changed the call's statistics")


def subsequence(kp, full):
    """The places in `full` of the keypoints `kp` (None for one that is not there)."""
    at = {k.tobytes(): i for i, k in enumerate(full)}
    assert len(at) == len(full)
    return [at.get(k.tobytes()) for k in kp]


def test_feature_count_on_ties(native, gpu):
    """810 keypoints of a repeated pattern, so four LDS tiles in the select pass and responses shared across
    positions: FeatureCount above the count changes nothing, and each cut through a run of equal
    responses keeps exactly what the reference's stable sort keeps, the earlier keys of the run."""
    img, full = R.image("tiled"), R.expected("tiled")
    n = len(full[0])
    for fc in (n + 5, 10 ** 9):
        R.assert_same(R.run(GPU, img, dict(FeatureCount=fc)), full, f"FeatureCount {fc} > PointCount {n}")
    order = np.argsort(-full[0]["response"], kind="stable")
    for fc in R.TILED_FC:
        keep = np.sort(order[:fc])
        got = R.run_case(GPU, f"tiled_fc_{fc}")
        have = subsequence(got.keypoints, full[0])
        if have != keep.tolist():
            extra, missing = sorted(set(have) - set(keep.tolist()), key=str), sorted(set(keep.tolist()) - set(have))
            raise AssertionError(f"FeatureCount {fc}: kept {extra[:5]} (responses "
                                 f"{[float(full[0]['response'][i]) for i in extra[:5] if i is not None]}) instead of "
                                 f"{missing[:5]} (responses {[float(full[0]['response'][i]) for i in missing[:5]]})")
        R.assert_same(got, (full[0][keep], full[1][keep]), f"FeatureCount {fc}")


# sizes, bucket counts, capacities and the descriptor type move up and down from call to call
SEQUENCE = ("noise_256", "narrow_24x9", "sigma_max_layers_1", "one_pixel", "tiled_fc_257", "layers_6",
            "float_descriptors", "seam_257x33", "constant", "narrow_24x9")


def test_history_independence(native, gpu):
    """One thread, one workspace: no call sees what an earlier, larger or differently typed call left."""
    for step, name in enumerate(SEQUENCE):
        got = R.run_case(GPU, name)
        st = stats()
        R.assert_same(got, R.expected(name), f"call {step + 1}, {name}")
        assert_counts(name, st)


def test_two_host_threads(native, gpu):
    """Two host threads, each with its own workspace and stream, call at the same time: each makes the
    calls of its half of SEQUENCE three times over. Every result is the reference's, and the statistics a
    thread reads after a call are that call's."""
    for name in SEQUENCE:
        R.expected(name)
    halves = (SEQUENCE[:5], SEQUENCE[5:])
    done, errors = [[], []], []
    go = threading.Barrier(2, timeout=60)

    def work(t):
        try:
            go.wait()
            for _ in range(3):
                for name in halves[t]:
                    got = R.run_case(GPU, name)
                    done[t].append((name, got, stats()))
        except BaseException as e:   # reported by the main thread
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(120)
    assert not any(th.is_alive() for th in threads), "a thread did not finish within 120 s"
    assert not errors, errors
    for t in range(2):
        assert [d[0] for d in done[t]] == list(halves[t]) * 3
        for step, (name, got, st) in enumerate(done[t]):
            R.assert_same(got, R.expected(name), f"thread {t}, call {step + 1}, {name}")
            assert_counts(name, st)


@pytest.mark.parametrize("name", ["tiled", "sigma_max_layers_1"])
def test_float_descriptors_of_other_cases(native, gpu, name):
    img, cfg = R.image(name), {**R.config(name), "DescriptorType": 5}
    f, twin, b = R.run(GPU, img, cfg), R.run(TWIN, img, cfg), R.run_case(GPU, name)
    assert f.descriptors.dtype == np.float32 and len(f) == len(R.expected(name)[0]) > 0
    R.assert_same(f, (twin.keypoints, twin.descriptors), f"{name}: float descriptors against the twin")
    assert np.array_equal(f.keypoints, b.keypoints)
    assert np.array_equal(np.clip(np.rint(f.descriptors), 0, 255).astype(np.uint8), b.descriptors)


def test_blobs(native, gpu):
    R.check_blobs(R.run_case(GPU, "blobs").keypoints)


def test_one_descriptor_path_for_every_radius(native, gpu):
    """The s = 20 blob's descriptor window (radius 100 and more) and the small blob's go through the
    same kernel: there is no short / long cut to count, only the totals."""
    got = R.run_case(GPU, "big_blob")
    st = stats()
    big = [d for d in R.detections(got.keypoints) if abs(d[0] - 100.3) < 0.5 and abs(d[1] - 80.6) < 0.5]
    assert len(big) == 1 and big[0][2] > 30.0 and st[7] == len(got) > 2


def test_float_descriptors_feature_count_and_colour(native, gpu):
    f, b = R.run_case(GPU, "float_descriptors"), R.run_case(GPU, "texture_97x61")
    assert np.array_equal(np.clip(np.rint(f.descriptors), 0, 255).astype(np.uint8), b.descriptors)
    img, full = R.image("texture_97x61"), R.expected("texture_97x61")
    R.assert_same(R.run(GPU, img, dict(FeatureCount=len(full[0]))), full, "FeatureCount == PointCount")
    for name in ("rgb", "rgba"):
        a, g = R.run(GPU, R.image(name)), R.run(GPU, R.grey(R.image(name)))
        assert len(a) > 20 and np.array_equal(a.keypoints, g.keypoints) and np.array_equal(a.descriptors, g.descriptors)


def test_determinism_and_counts(native, gpu):
    img, cfg = R.image("noise_256"), R.config("noise_256")
    runs = []
    for _ in range(3):
        f = R.run(GPU, img)
        runs.append((f.keypoints.tobytes(), f.descriptors.tobytes(), stats()))
    assert runs[0] == runs[1] == runs[2]
    assert runs[0][2][:4] == fixed_counts(img, cfg) and runs[0][2][7] == len(R.expected("noise_256")[0])
    # another content, the same size: the same launches, synchronisations, copies and memsets
    for other in (np.full((256, 256), 9, np.uint8), R.texture(256, 256, 2)):
        n = len(R.run(GPU, other))
        st = stats()
        assert st[:4] == runs[0][2][:4] and st[7] == n and st[4:] != runs[0][2][4:]


# Inliers of the host twin's features of the two windows through the same matchAndFindModel call,
# recorded on an MI355X: 1574 and 1550 keypoints, 1308 matches, all of them inliers.
TWIN_INLIERS = 1308


def test_end_to_end(native, gpu):
    """Two 200 x 160 windows of one 260 x 200 texture, offset by (16, 8): detectFeatures on both, then
    matchAndFindModel(similarity, L2 on the byte descriptors) finds the shift."""
    tex = R.texture(260, 200, 31, k=3)
    a, b = np.ascontiguousarray(tex[0:160, 0:200]), np.ascontiguousarray(tex[8:168, 16:216])
    fa, fb = opencv.detectFeatures(a), opencv.detectFeatures(b)
    params = opencv.RansacParams(threshold=1.0, confidence=0.99, max_iters=2000, seed=1)
    cnt, M, pairs, mask = opencv.matchAndFindModel(fa, fb, model=N.MODEL_SIMILARITY, norm=N.NORM_L2, params=params)
    ta, tb = R.run(TWIN, a), R.run(TWIN, b)
    tcnt = opencv.matchAndFindModel(ta, tb, model=N.MODEL_SIMILARITY, norm=N.NORM_L2, params=params)[0]
    print(f"end to end: {len(fa)} and {len(fb)} keypoints, {len(pairs)} matches, {cnt} inliers; twin {tcnt}")
    corners = np.array([[0, 0, 1], [199, 0, 1], [0, 159, 1], [199, 159, 1]], dtype=np.float64)
    mapped = corners @ M.T
    err = np.abs(mapped[:, :2] / mapped[:, 2:] - (corners[:, :2] - [16.0, 8.0])).max()
    assert err <= 0.5, (err, M)
    assert TWIN_INLIERS >= 60 and tcnt >= 60
    assert cnt >= TWIN_INLIERS // 2, (cnt, TWIN_INLIERS)   # half of the recorded 1308
    # the same features through the matcher alone
    p, d = opencv.matchFeatures(fa, fb, norm=N.NORM_L2)
    assert len(p) >= cnt and np.all(np.diff(p[:, 0]) > 0)
