"""Batched SIFT detection on the CPU: the declarations of cvDetectFeaturesBatch and its
companions; every refusal, through the export and through mcvTestSiftBatchPlan with the same message; the
plan's counts, which depend on the largest nOctaves, OctaveLayers and FeatureCount > 0 alone, and its
buckets and workspace bytes against a formula written out here; the Python wrapper's own checks; and
sift_batch_plan.h under AddressSanitizer + UBSan in a stand-alone program. No kernel is launched."""
import ctypes as C
import shutil
import subprocess

import numpy as np
import pytest

import _sift_batch as SB
import _sift_ref as R
from minicv_amd import native as N
from minicv_amd import opencv

EXPORT, PLAN = "cvDetectFeaturesBatch", "mcvTestSiftBatchPlan"


def test_declarations(native):
    txt = (N.ROOT / "include" / "minicv_native.h").read_text()
    for decl in ("MCV_API long long cvDetectFeaturesBatch(const mcvImage* images, int nImages, int mode, void* config,",
                 "MCV_API void cvFreeFeaturesBatch(DetectorResult* results, int nImages);",
                 "MCV_API int mcvTestSiftBatchStats(long long* stats8);",
                 "MCV_API int mcvTestSiftBatchPlan(const mcvImage* images, int nImages, int mode, const void* config, "
                 "long long* out8);", "} mcvImage;", "#define MCV_ABI_VERSION 3"):
        assert decl in txt, decl
    for name in (EXPORT, "cvFreeFeaturesBatch", "mcvTestSiftBatchStats", PLAN):
        assert name in N.SIGNATURES
    assert C.sizeof(N.mcvImage) == 24 and [k for k, _ in N.mcvImage._fields_] == ["data", "width", "height", "channels",
                                                                                 "reserved"]
    assert native.lib().mcvAbiVersion() == 3
    mtxt = (N.ROOT / "minicv_amd" / "csrc" / "sift_math.h").read_text()
    assert N.SIFT_BATCH_MAX_IMAGES >= 1024 and f"kSiftBatchMaxImages = {N.SIFT_BATCH_MAX_IMAGES};" in mtxt
    assert N.SIFT_BATCH_MAX_CANDIDATES == 1 << 24 and "kSiftBatchMaxCandidates = 1 << 24;" in mtxt
    assert N.SIFT_BATCH_MAX_WORKSPACE_BYTES == 1 << 35 and "kSiftBatchMaxWorkspaceBytes = 1ull << 35;" in mtxt
    ptxt = (N.ROOT / "minicv_amd" / "csrc" / "sift_batch_plan.h").read_text()
    assert f"kSiftBatchLaunchesFixed = {N.SIFT_BATCH_LAUNCHES_FIXED};" in ptxt
    assert (f"kSiftBatchSyncs = {N.SIFT_BATCH_SYNCS}, kSiftBatchCopies = {N.SIFT_BATCH_COPIES}, "
            f"kSiftBatchMemsets = {N.SIFT_BATCH_MEMSETS};") in ptxt
    assert f"kSiftBatchScanBlocks = {N.SIFT_BATCH_SCAN_BLOCKS};" in ptxt
    assert f"kSiftBatchImageBytes = {N.SIFT_BATCH_IMAGE_BYTES};" in ptxt
    assert N.SIFT_BATCH_SYNCS == N.SIFT_SYNCS   # four, as in the single call
    # the caps are stated in the public header's comment too
    for text in ("at most 4096 images", "1 << 24 extremum candidates", "1 << 35"):
        assert text in txt, text
    assert native.lib().mcvTestSiftBatchStats(None) == -1 and "null argument" in N.last_error()
    import minicv_amd
    assert minicv_amd.detectFeaturesBatch is opencv.detectFeaturesBatch
    native.lib().cvFreeFeaturesBatch(None, 3)   # NULL is fine
    zero = (N.DetectorResult * 3)()
    native.lib().cvFreeFeaturesBatch(C.addressof(zero), 3)   # and so are all-zero entries
    assert SB.all_zero(zero, 3)


def refused_both(ims, n, text, mode=4, cfg=None):
    """The raw calls of both exports: -1, the same message after the export's own name, containing `text`;
    the export leaves every results[i] all zero."""
    rc, out, perr = SB.plan_raw(ims, n, mode, cfg)
    assert rc == -1 and out == [-7] * 8, (text, rc, out)
    ret, res, err = SB.batch_raw(ims, n, mode, cfg)
    assert ret == -1, (text, ret)
    assert n <= 0 or SB.all_zero(res, n), text
    assert err.startswith(EXPORT + ": ") and perr.startswith(PLAN + ": "), (err, perr)
    assert err[len(EXPORT):] == perr[len(PLAN):], (err, perr)
    assert text in err, (text, err)
    return err


def test_refusals(native):
    img = R.image("texture_97x61")
    good = [img, R.image("narrow_24x9"), R.image("rgb")]

    def with_bad(at, **field):
        ims = SB.image_structs(good)
        for k, v in field.items():
            setattr(ims[at], k, v)
        return ims

    ok = SB.image_structs(good)
    for mode in (0, 1, 2, 3, 5):
        refused_both(ok, 3, "only SIFT (mode 4)", mode=mode)
    for ch in (2, 5):
        assert "image 1: channels must be 1, 3 or 4" in refused_both(with_bad(1, channels=ch), 3, "channels")
    assert "image 2: null image" in refused_both(with_bad(2, data=None), 3, "null image")
    for at, field in ((0, dict(width=0)), (1, dict(height=0)), (2, dict(width=-1)), (1, dict(height=-3))):
        refused_both(with_bad(at, **field), 3, f"image {at}: width and height must be positive")
    for at, field in ((2, dict(width=N.SIFT_MAX_SIDE + 1)), (0, dict(height=N.SIFT_MAX_SIDE + 1))):
        refused_both(with_bad(at, **field), 3, f"image {at}: width and height are capped at {N.SIFT_MAX_SIDE}")
    refused_both(with_bad(1, reserved=1), 3, "image 1: reserved must be 0")
    refused_both(with_bad(2, reserved=-5), 3, "image 2: reserved must be 0")
    D = N.SiftConfig.default
    for cfg, text in ((D(OctaveLayers=0), "OctaveLayers"), (D(OctaveLayers=N.SIFT_MAX_LAYERS + 1), "OctaveLayers"),
                      (D(Sigma=0.0), "Sigma"), (D(Sigma=N.SIFT_MAX_SIGMA * 1.01), "Sigma"), (D(Sigma=float("nan")), "Sigma"),
                      (D(ContrastThreshold=-0.01), "ContrastThreshold"), (D(EdgeThreshold=0.0), "EdgeThreshold"),
                      (D(DescriptorType=1), "DescriptorType")):
        refused_both(ok, 3, text, cfg=cfg)
        refused_both(ok, 0, text, cfg=cfg)   # the configuration is checked for an empty batch too
    refused_both(ok, -1, "nImages must not be negative")
    many = SB.image_structs([img] * (N.SIFT_BATCH_MAX_IMAGES + 1))
    refused_both(many, N.SIFT_BATCH_MAX_IMAGES + 1, f"exceeds the cap of {N.SIFT_BATCH_MAX_IMAGES} images")
    refused_both(None, 3, "null images")
    # the workspace cap: nothing is read by the checks, so one small buffer stands for every 8192 x 8192 image
    huge = (N.mcvImage * N.SIFT_BATCH_MAX_IMAGES)()
    for i in range(N.SIFT_BATCH_MAX_IMAGES):
        huge[i] = N.mcvImage(img.ctypes.data, N.SIFT_MAX_SIDE, N.SIFT_MAX_SIDE, 1, 0)
    err = refused_both(huge, N.SIFT_BATCH_MAX_IMAGES, "split the batch")
    assert f"exceeds the cap of {N.SIFT_BATCH_MAX_WORKSPACE_BYTES} bytes" in err
    # null results (the export alone), and an empty batch
    assert native.lib().cvDetectFeaturesBatch(C.addressof(ok), 3, 4, None, None) == -1 and "null results" in N.last_error()
    assert native.lib().cvDetectFeaturesBatch(None, 0, 4, None, None) == 0
    assert SB.plan_raw(None, 0)[:2] == (0, [0] * 6 + [formula([])[1], 0])
    assert native.lib().mcvTestSiftBatchPlan(C.addressof(ok), 3, 4, None, None) == -1 and "null argument" in N.last_error()


def test_export_fails_loudly_without_gpu(native):
    if native.lib().mcvDeviceCount() > 0:
        return   # the valid calls are the GPU suite's subject
    ims = SB.image_structs([R.image("texture_97x61"), R.image("one_pixel")])
    ret, res, err = SB.batch_raw(ims, 2)
    assert ret == -1 and "no HIP device" in err and SB.all_zero(res, 2)
    with pytest.raises(N.NativeError, match="no HIP device"):
        opencv.detectFeaturesBatch([R.image("texture_97x61")])


def octaves_of(a):
    h, w = a.shape[:2]
    return [((2 * w) >> o, (2 * h) >> o) for o in range(R.n_octaves(w, h))]


def formula(arrays, nl=3, sigma=1.6):
    """-> (buckets, workspace bytes) of a batch, written out: a bucket per (image, octave, layer, row); the
    bytes of the images, two scratch planes of the doubled size per image, the pyramids, the taps, the
    per-image table, the counter words (four, one per image, two per bucket and one, one per image and one,
    the scan's partial sums and one) and the candidate list of 16-byte records."""
    n = len(arrays)
    buckets = sum(nl * h for a in arrays for w, h in octaves_of(a))
    img = sum(a.size for a in arrays)
    scratch = sum(2 * 4 * s[0][0] * s[0][1] for s in map(octaves_of, arrays) if s)
    pyramid = sum(4 * (nl + 3) * w * h for a in arrays for w, h in octaves_of(a))
    taps = 4 * sum(2 * R.blur_taps(s)[1] + 1 for s in R.sigmas(nl, sigma))
    interior = sum(nl * max(w - 2 * R.BORDER, 0) * max(h - 2 * R.BORDER, 0) for a in arrays for w, h in octaves_of(a))
    counters = 4 * (4 + n + buckets + (buckets + 1) + (n + 1) + (N.SIFT_BATCH_SCAN_BLOCKS + 1))
    cand = 16 * min(max(interior, 1), N.SIFT_BATCH_MAX_CANDIDATES)
    return buckets, img + scratch + pyramid + taps + N.SIFT_BATCH_IMAGE_BYTES * n + counters + cand


def test_plan(native):
    tex = R.image("texture_97x61")
    one = SB.plan([tex])
    assert one[0] == N.sift_octaves(97, 61) == 5 and one[7] == 0
    assert one[1:5] == [N.sift_batch_launches([(97, 61)]), N.SIFT_BATCH_SYNCS, N.SIFT_BATCH_COPIES, N.SIFT_BATCH_MEMSETS]
    assert one[1] == N.SIFT_BATCH_LAUNCHES_FIXED + 5 * 11 + 4
    # the four counts do not grow with the number of images
    for b in (2, 40):
        assert SB.plan([tex] * b)[:5] == one[:5], b
    # a mixed batch plans what its largest image alone plans
    mixed = [R.image(name) for name in SB.DEFAULTS]
    sizes = [a.shape[1::-1] for a in mixed]
    largest = max(mixed, key=lambda a: N.sift_octaves(*a.shape[1::-1]))
    got = SB.plan(mixed)
    assert got[:5] == SB.plan([largest])[:5] and got[1] == N.sift_batch_launches(sizes)
    assert got[0] == max(N.sift_octaves(*s) for s in sizes) and got[7] == 1   # one_pixel has no octave
    # and move with OctaveLayers and with FeatureCount > 0
    for nl in (1, 6):
        p = SB.plan(mixed, OctaveLayers=nl)
        assert p[1] == N.sift_batch_launches(sizes, nl) != got[1] and p[2:5] == got[2:5]
    fc = SB.plan(mixed, FeatureCount=10)
    assert fc[1] == got[1] + 1 == N.sift_batch_launches(sizes, 3, 10) and fc[2:5] == got[2:5]
    assert SB.plan(mixed, FeatureCount=10 ** 9)[1] == fc[1]
    # buckets and workspace bytes
    for arrays, cfg in (([tex], {}), (mixed, {}), ([tex] * 40, {}), (mixed[::-1], dict(OctaveLayers=6)),
                        (mixed, dict(OctaveLayers=1, Sigma=4.0)), ([R.image("one_pixel")] * 3, {})):
        p = SB.plan(arrays, **cfg)
        assert tuple(p[5:7]) == formula(arrays, cfg.get("OctaveLayers", 3), cfg.get("Sigma", 1.6)), (len(arrays), cfg)
    # the octave sizes the formula walks are the reference's
    for name in SB.DEFAULTS:
        assert octaves_of(R.image(name)) == R.octave_sizes(name)
    # only images without an octave: nothing is launched, synchronised, copied or set
    assert SB.plan([R.image("one_pixel")] * 3)[:6] == [0, 0, 0, 0, 0, 0] and SB.plan([R.image("one_pixel")] * 3)[7] == 3
    assert N.sift_batch_launches([(1, 1)] * 3) == 0 and N.sift_batch_launches([]) == 0


def test_python_wrapper_checks(native):
    img = R.image("texture_97x61")
    for bad in (img.astype(np.float32), np.zeros((2, 3, 4, 1), np.uint8), img.astype(np.int16)):
        with pytest.raises(ValueError, match=r"images\[1\]"):
            opencv.detectFeaturesBatch([img, bad])
    with pytest.raises(N.NativeError, match="only SIFT"):
        opencv.detectFeaturesBatch([img], mode=N.FEATURE_ORB)
    assert opencv.detectFeaturesBatch([]) == []


def test_plan_under_sanitizers(native, tmp_path):
    """tests/native/sift_batch_plan_asan_main.cpp: a stand-alone program (its own main, nothing preloaded,
    nothing loaded into Python) over sift_batch_plan.h, built with -fsanitize=address,undefined and run on
    mixed sizes, the caps and the size arithmetic's overflow refusals; the plans it prints are
    mcvTestSiftBatchPlan's."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe, inp = tmp_path / "sift_batch_plan_asan", tmp_path / "batches.txt"
    src = N.ROOT / "tests" / "native" / "sift_batch_plan_asan_main.cpp"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", f"-I{N.ROOT / 'minicv_amd' / 'csrc'}", str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    side, cap = N.SIFT_MAX_SIDE, N.SIFT_BATCH_MAX_IMAGES
    mixed = [(1, a.shape[1], a.shape[0], SB.channels(a), 0) for a in (R.image(name) for name in SB.DEFAULTS)]
    D = R.DEFAULT
    # (mode, nImages, config overrides, groups of (count, w, h, channels, reserved))
    batches = [(4, len(mixed), {}, mixed), (4, len(mixed), dict(OctaveLayers=6, FeatureCount=5), mixed[::-1]),
               (4, 40, {}, [(40, 97, 61, 1, 0)]), (4, 3, {}, [(3, 1, 1, 1, 0)]), (4, 0, {}, []),
               (4, 1024, {}, [(1000, 320, 240, 1, 0), (24, 333, 77, 4, 0)]), (4, 16, dict(OctaveLayers=1, Sigma=4.0), [(16, 1920, 1080, 3, 0)]),
               (4, cap, {}, [(cap, side, side, 1, 0)]), (4, cap, {}, [(cap, side, side, 4, 0)]),
               (4, cap + 1, {}, [(cap + 1, 8, 8, 1, 0)]), (4, -1, {}, []), (2, 1, {}, [(1, 8, 8, 1, 0)]),
               (4, 3, {}, [(2, 8, 8, 1, 0), (1, 8, 8, 1, 7)]), (4, 2, {}, [(1, 8, 8, 1, 0), (1, side + 1, 8, 1, 0)]),
               (4, 1, dict(Sigma=5.0), [(1, 8, 8, 1, 0)])]
    with open(inp, "w") as f:
        for mode, n, cfg, groups in batches:
            c = {**D, **cfg}
            f.write(" ".join(map(repr, [mode, n, *(c[k] for k, _ in N.SiftConfig._fields_), len(groups),
                                        *(v for g in groups for v in g)])) + "\n")
    r = subprocess.run([str(exe), str(inp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == f"sift_batch_plan_asan ok: {len(batches)} batches" and "ERROR" not in r.stderr
    assert lines[-2] == "overflow refused: 4, kept: 2" and len(lines) == len(batches) + 2
    pixel = np.zeros(1, np.uint8)
    refusals = 0
    for (mode, n, cfg, groups), line in zip(batches, lines):
        shapes = [g[1:] for g in groups for _ in range(g[0])]
        ims = (N.mcvImage * max(len(shapes), 1))()
        for i, (w, h, ch, res) in enumerate(shapes):
            ims[i] = N.mcvImage(pixel.ctypes.data, w, h, ch, res)
        rc, out, err = SB.plan_raw(ims if shapes else None, n, mode, N.SiftConfig.default(**cfg))
        if rc == 0:
            assert line == "ok " + " ".join(map(str, out)), (line, out)
        else:
            refusals += 1
            assert line == "refused: plan" + err[len(PLAN):], (line, err)
    assert refusals == 8
