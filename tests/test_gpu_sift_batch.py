"""Batched SIFT detection on the GPU: every results[i] of cvDetectFeaturesBatch bit equal to
cvDetectFeatures on that image (the single call is pinned to the numpy reference by tests/test_gpu_sift.py)
and, on the small cases, to the reference itself; the order of the images and their neighbours change
nothing; the other configurations; FeatureCount per image; launch counts that do not grow with the batch;
determinism; calls of changing sizes on one thread and on two threads at once; and detectFeaturesBatch ->
matchAndFindModelBatch end to end."""
import threading

import numpy as np
import pytest

import _sift_batch as SB
import _sift_ref as R
from minicv_amd import native as N
from minicv_amd import opencv

pytestmark = pytest.mark.gpu

REFERENCE_TOO = ("texture_97x61", "narrow_24x9", "seam_128x32", "rgb")


def mixed():
    return [R.image(name) for name in SB.DEFAULTS]


def test_mixed_batch(native, gpu):
    """All default cases in one call: sizes from 1 x 1 to 257 x 33, one to four channels, images with no
    octave and with no keypoint."""
    arrays = mixed()
    got, st = SB.batch(arrays)
    total = SB.assert_batch_equals_singles(got, arrays, "mixed batch")
    for name in REFERENCE_TOO:
        R.assert_same(got[SB.DEFAULTS.index(name)], R.expected(name), f"{name}: the batch against the reference")
    for name in ("one_pixel", "constant"):
        f = got[SB.DEFAULTS.index(name)]
        assert len(f) == 0 and f.descriptors.shape == (0, 128), name
    assert st[4:] == total and st[7] == sum(len(f) for f in got) > 810, (st, total)   # tiled alone has 810
    assert st[:4] == SB.plan(arrays)[1:5], st
    # the raw results of the empty images: PointCount 0 with non-NULL members, as the single call returns them
    ims = SB.image_structs(arrays)
    ret, res, err = SB.batch_raw(ims, len(arrays))
    try:
        assert ret == st[7], err
        for i, name in enumerate(SB.DEFAULTS):
            assert res[i].Points and res[i].Descriptors and res[i].PointCount == len(got[i]), name
            assert res[i].DescriptorEntries == 128 * len(got[i]) and res[i].DescriptorElementType == 0
    finally:
        N.lib().cvFreeFeaturesBatch(N.C.addressof(res), len(arrays))
    assert SB.all_zero(res, len(arrays))


def test_order_and_neighbours(native, gpu):
    """The same images reversed, with the largest image first, last and in the middle, [a, a, b, a], and each
    image alone: an image's bytes do not depend on where it stands or what stands next to it. This shows up
    a block that runs outside its image, a shared counter or a wrong bucket base."""
    arrays = mixed()
    want = [SB.blob(f) for f in SB.batch(arrays)[0]]
    assert [SB.blob(f) for f in SB.batch(arrays[::-1])[0]] == want[::-1]
    big = max(range(len(arrays)), key=lambda i: arrays[i].size)
    rest = [i for i in range(len(arrays)) if i != big]
    for order in ([big] + rest, rest + [big], rest[:6] + [big] + rest[6:]):
        got = SB.batch([arrays[i] for i in order])[0]
        assert [SB.blob(f) for f in got] == [want[i] for i in order], order
    a, b = SB.DEFAULTS.index("texture_97x61"), SB.DEFAULTS.index("seam_257x33")
    got = [SB.blob(f) for f in SB.batch([arrays[a], arrays[a], arrays[b], arrays[a]])[0]]
    assert got == [want[a], want[a], want[b], want[a]]
    for i, arr in enumerate(arrays):
        got, st = SB.batch([arr])
        assert SB.blob(got[0]) == want[i], SB.DEFAULTS[i]
        assert st[:4] == SB.plan([arr])[1:5]


@pytest.mark.parametrize("name", ["layers_1", "layers_6", "sigma_0_8", "sigma_max_layers_1", "contrast_0",
                                  "float_descriptors"])
def test_other_configurations(native, gpu, name):
    """One batch of texture_97x61, narrow_24x9, seam_129x65 and the case's own image under the case's
    configuration. Sigma 4 with one layer blurs with radius 111, wider than narrow_24x9's octaves, in the
    LDS tiles of the single call (no opt-in above 64 KiB)."""
    cfg = R.CASES[name][1]
    assert cfg
    arrays = [R.image("texture_97x61"), R.image("narrow_24x9"), R.image("seam_129x65"), R.image(name)]
    got, st = SB.batch(arrays, **cfg)
    total = SB.assert_batch_equals_singles(got, arrays, name, **cfg)
    assert st[4:] == total and st[7] > 0
    assert st[:4] == SB.plan(arrays, **cfg)[1:5]
    want_dtype = np.float32 if cfg.get("DescriptorType") == 5 else np.uint8
    assert all(f.descriptors.dtype == want_dtype for f in got)


@pytest.mark.parametrize("fc", [257, 10, 10 ** 9])
def test_feature_count_per_image(native, gpu, fc):
    """FeatureCount applies to every image by itself: 257 cuts the 810 keypoints of `tiled` inside a run of
    tied responses one past a select tile and leaves texture_97x61 whole; 10 cuts all three."""
    arrays = [R.image("tiled"), R.image("texture_97x61"), R.image("tiled")]
    got, st = SB.batch(arrays, FeatureCount=fc)
    SB.assert_batch_equals_singles(got, arrays, f"FeatureCount {fc}", FeatureCount=fc)
    full = [len(R.expected("tiled")[0]), len(SB.single(arrays[1])[0])]
    assert [len(f) for f in got] == [min(fc, full[0]), min(fc, full[1]), min(fc, full[0])]
    assert st[:4] == SB.plan(arrays, FeatureCount=fc)[1:5]
    if fc == 257:
        for i in (0, 2):
            R.assert_same(got[i], R.expected("tiled_fc_257"), f"tiled_fc_257 at place {i}")


def test_counts_do_not_grow_with_the_batch(native, gpu):
    tex = R.image("texture_97x61")
    counts = []
    for b in (1, 3, 40):
        got, st = SB.batch([tex] * b)
        counts.append(st[:4])
        assert st[7] == b * len(got[0]) and all(SB.blob(f) == SB.blob(got[0]) for f in got)
    assert counts[0] == counts[1] == counts[2] == [N.sift_batch_launches([(97, 61)]), N.SIFT_BATCH_SYNCS,
                                                   N.SIFT_BATCH_COPIES, N.SIFT_BATCH_MEMSETS]
    # another content of the same sizes: the same four counts, other keypoints
    first = SB.batch([tex] * 3)[1]
    for other in (np.full((61, 97), 9, np.uint8), R.texture(97, 61, 2)):
        st = SB.batch([other] * 3)[1]
        assert st[:4] == counts[0] and st[4:] != first[4:]


def test_determinism(native, gpu):
    arrays = mixed()
    runs = []
    for _ in range(3):
        got, st = SB.batch(arrays)
        runs.append(([SB.blob(f) for f in got], st))
    assert runs[0] == runs[1] == runs[2]


def test_history_independence(native, gpu):
    """One thread, one workspace: a large mixed batch, one small image, float descriptors, a batch without
    an octave and the mixed batch again. No call sees what an earlier, larger or differently typed one left."""
    arrays = mixed()
    empty = [R.image("one_pixel")] * 3
    steps = [(arrays, {}), ([R.image("narrow_24x9")], {}), (arrays[:4], dict(DescriptorType=5)), (empty, {}),
             (arrays, {})]
    for step, (imgs, cfg) in enumerate(steps):
        got, st = SB.batch(imgs, **cfg)
        total = SB.assert_batch_equals_singles(got, imgs, f"call {step + 1}", **cfg)
        assert st[4:] == total and st[:4] == SB.plan(imgs, **cfg)[1:5], (step, st)
    assert SB.batch(empty)[1] == [0] * 8


def test_two_host_threads(native, gpu):
    """Two host threads, each with its own workspace and stream, run their own sequences of batches at the
    same time; every result is the single call's and the statistics a thread reads are its own call's."""
    arrays = mixed()
    plans = ([(arrays, {}), ([R.image("narrow_24x9")], {}), (arrays[:4], dict(DescriptorType=5))],
             [([R.image("tiled"), R.image("texture_97x61")], dict(FeatureCount=10)), ([R.image("one_pixel")] * 2, {}),
              (arrays[::-1], {})])
    for seq in plans:   # the yardsticks, before the threads start
        for imgs, cfg in seq:
            for a in imgs:
                SB.single(a, **cfg)
    done, errors = [[], []], []
    go = threading.Barrier(2, timeout=60)

    def work(t):
        try:
            go.wait()
            for _ in range(2):
                for imgs, cfg in plans[t]:
                    done[t].append((imgs, cfg, *SB.batch(imgs, **cfg)))
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
        assert len(done[t]) == 2 * len(plans[t])
        for step, (imgs, cfg, got, st) in enumerate(done[t]):
            total = SB.assert_batch_equals_singles(got, imgs, f"thread {t}, call {step + 1}", **cfg)
            assert st[4:] == total and st[:4] == SB.plan(imgs, **cfg)[1:5], (t, step, st)


def test_end_to_end(native, gpu):
    """Three 200 x 160 windows of one 260 x 200 texture at known offsets: detectFeaturesBatch, then
    matchAndFindModelBatch (similarity, L2 on the byte descriptors) over the three pairs finds every shift
    to within 0.5 px at the window corners, the bound of test_gpu_sift.py::test_end_to_end, and returns what
    it returns on the features of three single detectFeatures calls."""
    tex = R.texture(260, 200, 31, k=3)
    offsets = [(0, 0), (16, 8), (40, 24)]
    wins = [np.ascontiguousarray(tex[y:y + 160, x:x + 200]) for x, y in offsets]
    pairs = [(0, 1), (0, 2), (1, 2)]
    feats = opencv.detectFeaturesBatch(wins)
    ones = [opencv.detectFeatures(w) for w in wins]
    for i in range(3):
        R.assert_same(feats[i], (ones[i].keypoints, ones[i].descriptors), f"window {i}")
    params = opencv.RansacParams(threshold=1.0, confidence=0.99, max_iters=2000, seed=1)
    kw = dict(model=N.MODEL_SIMILARITY, norm=N.NORM_L2, params=params)
    got, want = opencv.matchAndFindModelBatch(feats, pairs, **kw), opencv.matchAndFindModelBatch(ones, pairs, **kw)
    corners = np.array([[0, 0, 1], [199, 0, 1], [0, 159, 1], [199, 159, 1]], dtype=np.float64)
    for (i, j), (cnt, M, pr, mask), (wcnt, wM, wpr, wmask) in zip(pairs, got, want):
        shift = np.subtract(offsets[j], offsets[i]).astype(np.float64)
        mapped = corners @ M.T
        err = np.abs(mapped[:, :2] / mapped[:, 2:] - (corners[:, :2] - shift)).max()
        print(f"pair {i}-{j}: {len(feats[i])} and {len(feats[j])} keypoints, {len(pr)} matches, {cnt} inliers, "
              f"corner error {err:.4f} px")
        assert cnt > 0 and err <= 0.5, ((i, j), cnt, err, M)
        assert cnt == wcnt and np.array_equal(pr, wpr) and np.array_equal(mask, wmask) and np.array_equal(M, wM)
