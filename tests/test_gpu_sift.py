"""SIFT detection on the GPU: cvDetectFeatures against the host twin and the numpy
reference on the shared case list (tests/_sift_ref.py), every output bit equal; the blob image; the
call's launch counts and its determinism; and detectFeatures -> matchAndFindModel end to end."""
import ctypes as C

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


@pytest.mark.parametrize("name", list(R.CASES))
def test_parity(native, gpu, name):
    want = R.expected(name)
    got = R.run_case(GPU, name)
    st = stats()
    R.assert_same(got, want, f"{name}: cvDetectFeatures against the reference")
    twin = R.run_case(TWIN, name)
    R.assert_same(got, (twin.keypoints, twin.descriptors), f"{name}: cvDetectFeatures against the twin")
    cnt = want[2]
    assert st[4:] == [cnt["candidates"], cnt["refined"], cnt["oriented"], len(want[0])], (name, st)
    if N.sift_octaves(*R.image(name).shape[1::-1]) == 0:
        assert st[:4] == [0, 0, 0, 0]
    else:
        assert st[:4] == fixed_counts(R.image(name), R.config(name)), (name, st)


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
