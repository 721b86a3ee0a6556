"""SIFT detection on the CPU: the host twin (mcvHostDetectFeatures, sift_ref.h) against the
independent numpy reference on the shared case list, every output bit equal; that each case still reaches
the branch it is there for; the blob image's detections; every refusal of cvDetectFeatures, of the twin
and of mcvTestSiftStage; the declarations; and sift_ref.h under AddressSanitizer + UBSan in a stand-alone
program. No kernel is launched."""
import ctypes as C
import shutil
import subprocess

import numpy as np
import pytest

import _sift_ref as R
from minicv_amd import native as N
from minicv_amd import opencv

BOTH = ("cvDetectFeatures", "mcvHostDetectFeatures")
TWIN = "mcvHostDetectFeatures"


@pytest.mark.parametrize("name", list(R.CASES))
def test_twin_equals_reference(native, name):
    R.assert_same(R.run_case(TWIN, name), R.expected(name), name)


def test_cases_cover_what_they_are_for():
    n = {name: len(R.expected(name)[0]) for name in R.CASES}
    assert n["noise_256"] > 2000 and n["one_pixel"] == 0 and n["constant"] == 0 and n["narrow_24x9"] > 0
    assert n["texture_97x61"] > 50 and n["feature_count_10"] == 10
    # exact duplicates exist and are removed (two candidates refine to one position)
    assert R.expected("layers_2")[2]["oriented"] > n["layers_2"]
    # the s = 20 blob is found, with a descriptor radius far above the others'
    big = [d for d in R.detections(R.expected("big_blob")[0]) if abs(d[0] - 100.3) < 0.5 and abs(d[1] - 80.6) < 0.5]
    assert len(big) == 1 and big[0][2] > 30.0
    # the largest blur: radii up to kSiftMaxRadius, and keypoints in more than one octave
    cfg = R.config("sigma_max_layers_1")
    assert R.blur_taps(R.sigmas(cfg["OctaveLayers"], cfg["Sigma"])[3])[1] == 111
    assert len({R.keypoint_octave(k) for k in R.expected("sigma_max_layers_1")[0]}) >= 2
    # Sigma^2 - 1 <= 0.01: the base blur has three taps
    for name in ("sigma_1_0", "sigma_0_8"):
        cfg = R.config(name)
        assert R.blur_taps(R.sigmas(cfg["OctaveLayers"], cfg["Sigma"])[0])[1] == 1 and n[name] > 20, name
    assert n["layers_1"] > 50 and n["layers_6"] > 50
    assert n["edge_2"] < n["texture_97x61"] <= n["edge_1e6"]
    assert R.expected("contrast_0")[2]["candidates"] >= R.expected("texture_97x61")[2]["candidates"]
    # the seams of the row tile (256), the column tile (64 x 32) and the extrema tile (64 x 4): an octave
    # of exactly one tile and one of a tile plus one, along each axis
    sizes = [s for name in R.SEAM_CASES for s in R.octave_sizes(name)]
    for what, hit in (("w % 256 == 1", [w % 256 == 1 for w, h in sizes]), ("w % 64 == 1", [w % 64 == 1 for w, h in sizes]),
                      ("h % 32 == 1", [h % 32 == 1 for w, h in sizes]), ("h % 4 == 1", [h % 4 == 1 for w, h in sizes]),
                      ("w == 256", [w == 256 for w, h in sizes]), ("w == 64", [w == 64 for w, h in sizes]),
                      ("h == 32", [h == 32 for w, h in sizes])):
        assert any(hit), (what, sizes)
    assert all(n[name] > (30 if name == "tall_9x300" else 100) for name in R.SEAM_CASES), n
    # every descriptor window of the small blob image is cut to its octave's diagonal
    kp, sizes = R.expected("clamped_radius")[0], R.octave_sizes("clamped_radius")
    assert len(kp) > 0
    for k in kp:
        assert R.descriptor_radius(R.keypoint_scale(k)) >= R.diagonal(*sizes[R.keypoint_octave(k)]), k
    # FeatureCount on ties: four select tiles of 256 records, responses shared across positions, and every
    # cut between two records of equal response
    kp = R.expected("tiled")[0]
    assert n["tiled"] > 768
    where = {}
    for k in kp:
        where.setdefault(float(k["response"]), set()).add((float(k["x"]), float(k["y"])))
    assert sum(len(p) > 1 for p in where.values()) >= 20
    order = np.argsort(-kp["response"], kind="stable")
    for fc in R.TILED_FC:
        assert n[f"tiled_fc_{fc}"] == fc < n["tiled"]
        assert kp["response"][order[fc - 1]] == kp["response"][order[fc]], fc


def test_stage_export_refusals(native):
    """mcvTestSiftStage refuses an unknown stage, a null argument, a capacity that cannot hold anything and a
    thread that has made no call; no device is needed for any of them."""
    import threading
    L = native.lib()
    txt = (N.ROOT / "include" / "minicv_native.h").read_text()
    assert "MCV_API int mcvTestSiftStage(int what, void* out, long long capBytes, long long* count);" in txt
    assert "mcvTestSiftStage" in N.SIGNATURES
    buf, cnt = np.zeros(16, np.float32), C.c_longlong(-7)
    for what in (-1, 2, 99):
        assert L.mcvTestSiftStage(what, buf.ctypes.data, buf.nbytes, C.byref(cnt)) == -1
        assert "unknown stage" in N.last_error()
    for what in (0, 1):
        assert L.mcvTestSiftStage(what, None, buf.nbytes, C.byref(cnt)) == -1 and "null argument" in N.last_error()
        assert L.mcvTestSiftStage(what, buf.ctypes.data, buf.nbytes, None) == -1 and "null argument" in N.last_error()
        assert L.mcvTestSiftStage(what, buf.ctypes.data, -1, C.byref(cnt)) == -1 and "too small" in N.last_error()
    got = []

    def fresh_thread():
        b, c = np.zeros(16, np.float32), C.c_longlong(-7)
        got.append([(L.mcvTestSiftStage(what, b.ctypes.data, b.nbytes, C.byref(c)), N.last_error(), c.value)
                    for what in (0, 1)])

    t = threading.Thread(target=fresh_thread)
    t.start()
    t.join(60)
    assert not t.is_alive() and len(got) == 1
    for rc, err, c in got[0]:
        assert rc == -1 and "no finished cvDetectFeatures call" in err and c == -7
    assert cnt.value == -7 and not buf.any()


def test_blobs(native):
    """160 x 120, six Gaussian blobs: the reference and the twin find exactly one detection per blob.
    The reference's position errors are 0.000 - 0.031 px and its size ratios 0.984 - 0.998."""
    R.check_blobs(R.expected("blobs")[0])
    R.check_blobs(R.run_case(TWIN, "blobs").keypoints)


def test_float_descriptors_round_to_the_bytes(native):
    f = R.run_case(TWIN, "float_descriptors")
    b = R.run_case(TWIN, "texture_97x61")
    assert f.descriptors.dtype == np.float32 and b.descriptors.dtype == np.uint8
    assert np.array_equal(f.keypoints, b.keypoints)
    assert np.array_equal(np.clip(np.rint(f.descriptors), 0, 255).astype(np.uint8), b.descriptors)
    assert f.struct.DescriptorElementType == 5 and f.struct.DescriptorEntries == 128 * len(f)


def test_feature_count(native):
    img, full = R.image("texture_97x61"), R.expected("texture_97x61")
    n = len(full[0])
    R.assert_same(R.run(TWIN, img, dict(FeatureCount=n)), full, "FeatureCount == PointCount")
    R.assert_same(R.run(TWIN, img, dict(FeatureCount=n + 5)), full, "FeatureCount > PointCount")
    ten = R.run_case(TWIN, "feature_count_10")
    keep = np.sort(np.argsort(-full[0]["response"], kind="stable")[:10])
    assert np.array_equal(ten.keypoints, full[0][keep]) and np.array_equal(ten.descriptors, full[1][keep])


@pytest.mark.parametrize("name", ["rgb", "rgba"])
def test_colour_equals_its_grey(native, name):
    img = R.image(name)
    a, b = R.run(TWIN, img), R.run(TWIN, R.grey(img))
    assert len(a) > 20 and np.array_equal(a.keypoints, b.keypoints) and np.array_equal(a.descriptors, b.descriptors)


def refused(export, img_args, mode=4, cfg=None):
    """The raw call -> the error text; asserts NULL."""
    L = N.lib()
    p = getattr(L, export)(*img_args, mode, N.C.addressof(cfg) if cfg is not None else None)
    assert not p, (export, img_args, mode)
    return N.last_error()


@pytest.mark.parametrize("export", BOTH)
def test_still_refused(native, export):
    img = R.image("texture_97x61")
    ok = (img.ctypes.data, 97, 61, 1)
    for mode in (0, 1, 2, 3, 5):
        assert "only SIFT (mode 4)" in refused(export, ok, mode)
    for ch in (2, 5):
        assert "channels must be 1, 3 or 4" in refused(export, (img.ctypes.data, 97, 61, ch))
    assert "null image" in refused(export, (None, 97, 61, 1))
    for w, h in ((0, 61), (97, 0), (-1, 61), (97, -3)):
        assert "must be positive" in refused(export, (img.ctypes.data, w, h, 1))
    for w, h in ((N.SIFT_MAX_SIDE + 1, 1), (1, N.SIFT_MAX_SIDE + 1)):
        assert f"capped at {N.SIFT_MAX_SIDE}" in refused(export, (img.ctypes.data, w, h, 1))
    D = N.SiftConfig.default
    for cfg, text in ((D(OctaveLayers=0), "OctaveLayers"), (D(OctaveLayers=N.SIFT_MAX_LAYERS + 1), "OctaveLayers"),
                      (D(Sigma=0.0), "Sigma"), (D(Sigma=-1.0), "Sigma"), (D(Sigma=N.SIFT_MAX_SIGMA * 1.01), "Sigma"),
                      (D(Sigma=float("nan")), "Sigma"), (D(ContrastThreshold=-0.01), "ContrastThreshold"),
                      (D(ContrastThreshold=float("nan")), "ContrastThreshold"), (D(EdgeThreshold=0.0), "EdgeThreshold"),
                      (D(EdgeThreshold=-2.0), "EdgeThreshold"), (D(DescriptorType=1), "DescriptorType"),
                      (D(DescriptorType=6), "DescriptorType")):
        assert text in refused(export, ok, 4, cfg), text
    with pytest.raises(N.NativeError, match="only SIFT"):
        opencv._detect_features(export, img, N.FEATURE_ORB, None)
    with pytest.raises(ValueError):
        opencv.detectFeatures(img.astype(np.float32))


def test_export_fails_loudly_without_gpu(native):
    if native.lib().mcvDeviceCount() > 0:
        return   # the valid calls are the GPU suite's subject
    with pytest.raises(N.NativeError, match="no HIP device"):
        opencv.detectFeatures(R.image("texture_97x61"))


def test_declarations(native):
    txt = (N.ROOT / "include" / "minicv_native.h").read_text()
    for name in ("mcvHostDetectFeatures", "cvDetectFeatures"):
        assert name in N.SIGNATURES and f"MCV_API DetectorResult* {name}(" in txt
    assert "MCV_API int mcvTestSiftStats(" in txt and native.lib().mcvTestSiftStats(None) == -1
    assert "#define MCV_ABI_VERSION 3" in txt and native.lib().mcvAbiVersion() == 3
    for k, v in (("AKAZE", N.FEATURE_AKAZE), ("ORB", N.FEATURE_ORB), ("BRISK", N.FEATURE_BRISK), ("SIFT", N.FEATURE_SIFT)):
        assert any(ln.split() == ["#define", f"MCV_FEATURE_MODE_{k}", str(v)] for ln in txt.split("\n"))
    assert N.C.sizeof(N.SiftConfig) == 40 and N.C.sizeof(N.KeyPoint2d) == 28 == opencv.KEYPOINT_DTYPE.itemsize
    d = N.SiftConfig.default()
    assert [getattr(d, k) for k, _ in N.SiftConfig._fields_] == [0, 3, 0.04, 10.0, 1.6, 0]
    ktxt = (N.ROOT / "minicv_amd" / "csrc" / "kernels.h").read_text()
    L = N.SIFT_LAUNCHES
    assert (f"kSiftLaunchesFixed = {L['fixed']}, kSiftLaunchesPerBlur = {L['per_blur']}, "
            f"kSiftLaunchesExtrema = {L['extrema']}") in ktxt
    assert f"kSiftLaunchesDownsample = {L['downsample']}, kSiftLaunchesSelect = {L['select']};" in ktxt
    assert f"kSiftSyncs = {N.SIFT_SYNCS}, kSiftCopies = {N.SIFT_COPIES}, kSiftMemsets = {N.SIFT_MEMSETS};" in ktxt
    mtxt = (N.ROOT / "minicv_amd" / "csrc" / "sift_math.h").read_text()
    assert f"kSiftMaxSide = {N.SIFT_MAX_SIDE};" in mtxt and f"kSiftMaxLayers = {N.SIFT_MAX_LAYERS};" in mtxt
    assert N.sift_octaves(1, 1) == 0 and N.sift_octaves(24, 9) == 2 and N.sift_octaves(256, 256) == 7
    assert N.sift_launches(1, 1) == 0 and N.sift_launches(256, 256) == 10 + 7 * 11 + 6
    import minicv_amd
    assert minicv_amd.detectFeatures is opencv.detectFeatures and minicv_amd.SiftConfig is N.SiftConfig
    assert issubclass(opencv.DetectedFeatures, opencv.Features)


def test_result_is_a_features(native):
    f = R.run_case(TWIN, "texture_97x61")
    kp = R.expected("texture_97x61")[0]
    assert isinstance(f, opencv.Features) and f.struct.PointCount == len(kp) == len(f)
    assert f.points.shape == (len(kp), 2) and np.array_equal(f.points[:, 0], kp["x"])
    for name in ("size", "angle", "response", "octave"):
        assert np.array_equal(getattr(f, name), kp[name])
    assert np.all(kp["class_id"] == -1) and np.all((kp["angle"] >= 0) & (kp["angle"] < 360))
    e = R.run_case(TWIN, "constant")
    assert len(e) == 0 and e.struct.PointCount == 0 and e.descriptors.shape == (0, 128)


def test_host_twin_under_sanitizers(tmp_path):
    """tests/native/sift_asan_main.cpp: a stand-alone program (its own main, nothing preloaded, nothing
    loaded into Python) over sift_ref.h, built with -fsanitize=address,undefined and run on the 97 x 61
    and 24 x 9 cases, the radius-111 blurs, their reflections over the 18- and 9-wide octaves of the tall
    image, the clamped descriptor window and six layers, each with its own configuration; its keypoints
    and descriptor bytes equal the reference's."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe, inp = tmp_path / "sift_asan", tmp_path / "cases.txt"
    src = N.ROOT / "tests" / "native" / "sift_asan_main.cpp"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", f"-I{N.ROOT / 'minicv_amd' / 'csrc'}", str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    names = ["texture_97x61", "narrow_24x9", "sigma_max_layers_1", "clamped_radius", "tall_9x300", "layers_6"]
    with open(inp, "w") as f:
        for name in names:
            img, cfg = R.image(name), R.config(name)
            f.write(" ".join(map(repr, [img.shape[1], img.shape[0], *(cfg[k] for k, _ in N.SiftConfig._fields_),
                                        *img.reshape(-1).tolist()])) + "\n")
    r = subprocess.run([str(exe), str(inp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == f"sift_asan ok: {len(names)} cases" and "ERROR" not in r.stderr
    at = 0
    for name in names:
        kp, desc, _ = R.expected(name)
        assert int(lines[at]) == len(kp), name
        got = np.array([[int(v) for v in ln.split()] for ln in lines[at + 1:at + 1 + len(kp)]], dtype=np.int64)
        want = np.concatenate([kp.view(np.uint32).reshape(len(kp), 7).astype(np.int64), desc.astype(np.int64)], axis=1)
        assert np.array_equal(got, want), name
        at += 1 + len(kp)
