"""Track triangulation on the CPU: the definition (hyp_rays.h through the host twins) against the
pure-Python reference bit for bit, the constants and layouts of the contract, the argument checks,
and the twin's CSR / dedupe code under AddressSanitizer + UBSan in a stand-alone program.
No kernel is launched here."""
import ctypes as C
import math
import shutil
import subprocess

import numpy as np
import pytest

import _triangulate_ref as R
from minicv_amd import camera as CM
from minicv_amd import native as N
from minicv_amd import synthetic as S

EXPORTS = ("cvIntersectRays", "cvTriangulateTracks", "mcvTriangulateTracksDevice", "mcvHostIntersectRays",
           "mcvHostTriangulateTracks", "mcvTestTriangulateStats")


def test_sin_min_angle_is_the_bisection_result():
    """kSinMinAngle = the largest double for which the reference's predicate
    asin(clamp 0 1 len) * DegreesPerRadian > 2.0 is false on this libm."""
    def pred(s):
        return math.asin(min(max(s, 0.0), 1.0)) * (180.0 / math.pi) > 2.0
    lo, hi = 0.0, 1.0
    assert not pred(lo) and pred(hi)
    while math.nextafter(lo, 1.0) < hi:
        mid = (lo + hi) / 2
        if pred(mid):
            hi = mid
        else:
            lo = mid
    assert lo.hex() == "0x1.1de58c9f7dc27p-5"
    assert N.SIN_MIN_ANGLE == lo == R.K_SIN
    txt = (N.ROOT / "minicv_amd" / "csrc" / "hyp_rays.h").read_text()
    assert "kSinMinAngle = 0x1.1de58c9f7dc27p-5;" in txt


def test_ray3d_layout():
    assert C.sizeof(N.Ray3d) == 48 and C.sizeof(N.Camera) == 112
    assert N.Ray3d.direction.offset == 24


def test_exports_declared(native):
    txt = (N.ROOT / "include" / "minicv_native.h").read_text()
    for name in EXPORTS:
        assert name in N.SIGNATURES and getattr(native.lib(), name) is not None
        assert f"MCV_API int {name}(" in txt
    assert "#define MCV_MAX_TRACK_LEN 4096" in txt and N.MAX_TRACK_LEN == 4096
    import minicv_amd
    assert minicv_amd.triangulateTracks is CM.triangulateTracks
    for f in (CM.unproject1, CM.intersection, CM.intersectRays):
        assert callable(f)


def test_abi_version_unchanged(native):
    assert native.lib().mcvAbiVersion() == 3


@pytest.mark.parametrize("name", list(R.CASES))
def test_host_twins_equal_reference(native, name):
    p = R.problem(name)
    k, pts, cnt = R.host_rays(p)
    assert k == int((p.counts > 0).sum()), native.last_error()
    R.assert_same((pts, cnt), p, "mcvHostIntersectRays")
    k, pts, cnt, cost, vis = R.host_tracks(p)
    assert k == int((p.counts > 0).sum()), native.last_error()
    R.assert_same((pts, cnt, cost, vis), p, "mcvHostTriangulateTracks")
    assert p.enough_points()


def test_scale_case_is_a_second_trip_case():
    """What makes `scale` a second-trip case, from the mirrored constants, and what keeps it honest."""
    ktxt = (N.ROOT / "minicv_amd" / "csrc" / "kernels.h").read_text()
    assert f"kTriGrid = {N.TRI_GRID};" in ktxt and f"kTriShortMax = {N.TRI_SHORT_MAX};" in ktxt
    p = R.scale()
    assert p.n > N.TRI_GRID * 256 and p.nLong > 8 * N.TRI_GRID and p.T > 8 * N.TRI_GRID
    L = p.lengths()
    assert set(L.tolist()) == {3, N.TRI_SHORT_MAX + 1} and int((L > N.TRI_SHORT_MAX).sum()) == p.nLong
    is_long = L > N.TRI_SHORT_MAX
    assert not any(np.array_equal(is_long[:-k], is_long[k:]) for k in (64, 256, 1024))   # no period of the launch shape
    s = p.lengths()[p.sample]
    assert len(s) == R.SCALE_SAMPLE and int((s > N.TRI_SHORT_MAX).sum()) == R.SCALE_SAMPLE // 2
    assert p.ref.enough_points() and p.ref.counters["duplicate"] >= 1 and p.ref.counters["angle"] >= 1
    # the vectorised unproject is the reference's, to the bit
    assert np.array_equal(R.bits(p.rays[p.sample_obs]), R.bits(p.ref.rays))


def test_host_twins_on_the_scale_case(native):
    p = R.scale()
    k, pts, cnt, cost, vis = R.host_tracks(p)
    assert k == int((cnt > 0).sum()) > p.T // 2, native.last_error()
    p.assert_sample((pts, cnt, cost, vis), "mcvHostTriangulateTracks")
    k2, rpts, rcnt = R.host_rays(p)
    assert k2 == k
    R.assert_bits((rpts, rcnt), (pts, cnt), "mcvHostIntersectRays against mcvHostTriangulateTracks")


def test_host_twin_optional_statistics(native):
    p = R.problem("statistics")
    k, pts, cnt, cost, vis = R.host_tracks(p, stats=False)
    R.assert_same((pts, cnt), p, "without statistics")
    assert np.all(cost == 7.0) and np.all(vis == -7)


def test_unproject1_matches_reference():
    p = R.problem("statistics")
    cam = CM.Camera(p.cams[3, 0:3], p.cams[3, 3:6], p.cams[3, 6:9], p.cams[3, 9:12], p.cams[3, 12:14])
    for ox, oy in ((0.25, -0.5), (0.0, 0.0), (-1.5, 1.25)):
        got = CM.unproject1(cam, (ox, oy))
        assert np.array_equal(R.bits(got), R.bits(np.array(R.ref_unproject(p.cams[3].tolist(), ox, oy))))


def test_noise_free_tracks_recover_the_truth(native):
    """Exact observations of a point at scale 10: every pair's midpoint is the point up to the rounding
    of the rays (a few ulps at scale 10, ~1e-15) amplified by at most 1 / sin 2 deg ~ 29 through
    getClosestTs, so 1e-9 leaves four orders of margin."""
    cams, idx, obs, off, truth = S.track_problem(300, 77, lengths=(2, 3, 4, 6, 9, 12, 20, 33), n_cameras=48)
    p = R.Problem(cams, idx, obs, off)
    k, pts, cnt, cost, vis = R.host_tracks(p)
    R.assert_same((pts, cnt, cost, vis), p, "noise-free")
    has = cnt > 0
    assert has.sum() >= 0.9 * len(cnt)
    assert np.max(np.abs(pts[has] - truth[has])) < 1e-9
    assert np.all(vis[has] == np.diff(off)[has]) and np.max(cost[has]) < 1e-18


_call = R.call_export


HOST_POINTER = ("cvIntersectRays", "cvTriangulateTracks", "mcvHostIntersectRays", "mcvHostTriangulateTracks")


@pytest.mark.parametrize("name", HOST_POINTER)
def test_bad_arguments_rejected_before_the_device(native, name):
    """The checks are the same with and without a GPU, and a refused call writes nothing."""
    p = R.problem("length_cutoff")
    ray_form = "Rays" in name
    for null in (("rays", "off", "pts", "cnt") if ray_form else ("cams", "idx", "obs", "off", "pts", "cnt")):
        k, untouched, _ = _call(name, p, null=null)
        assert k == -1 and untouched and "null" in native.last_error() and name in native.last_error()
    bad = p.offsets.copy()
    bad[0] = 1
    k, untouched, _ = _call(name, p, offsets=bad)
    assert k == -1 and untouched and "offsets[0]" in native.last_error()
    bad = p.offsets.copy()
    bad[3] = bad[2] - 1
    k, untouched, _ = _call(name, p, offsets=bad)
    assert k == -1 and untouched and "decrease at track 2" in native.last_error()
    k, untouched, _ = _call(name, p, offsets=[0, 2, 2 + N.MAX_TRACK_LEN + 1])
    assert k == -1 and untouched and "track 1 has 4097 rays" in native.last_error()
    if not ray_form:
        for v in (-1, p.cams.shape[0]):
            idx = p.idx.copy()
            idx[5] = v
            k, untouched, _ = _call(name, p, idx=idx)
            assert k == -1 and untouched and "cameraIdx[5]" in native.last_error()
    # T == 0 succeeds without looking at anything else
    k, untouched, _ = _call(name, p, offsets=[0])
    assert k == 0 and untouched and native.last_error() == ""


def test_device_export_checks_its_pointers(native):
    L = N.lib()
    assert L.mcvTriangulateTracksDevice(None, 1, None, None, None, 0, None, None, None, None) == 0
    assert L.mcvTriangulateTracksDevice(None, 1, None, None, None, 3, None, None, None, None) == -1
    assert "null" in native.last_error()
    assert L.mcvTriangulateTracksDevice(None, 1, None, None, None, -3, None, None, None, None) == -1
    assert "negative T" in native.last_error()
    assert L.mcvTestTriangulateStats(None) == -1


def test_exports_fail_loudly_without_gpu(native):
    if native.lib().mcvDeviceCount() > 0:
        return   # the valid calls are the GPU suite's subject
    p = R.problem("length_cutoff")
    for name in ("cvIntersectRays", "cvTriangulateTracks"):
        k, untouched, _ = _call(name, p)
        assert k == -1 and untouched and "no HIP device" in native.last_error()
    with pytest.raises(N.NativeError, match="no HIP device"):
        CM.triangulateTracks(p.cams, p.idx, p.obs, p.offsets, stats=True)
    with pytest.raises(N.NativeError, match="no HIP device"):
        CM.intersectRays(p.rays, p.offsets)
    with pytest.raises(N.NativeError, match="no HIP device"):
        CM.intersection(p.rays[:3])
    one = np.zeros(16, np.int64)   # stands in for device pointers: the call must stop before using them
    a = one.ctypes.data
    assert N.lib().mcvTriangulateTracksDevice(a, 1, a, a, a, 1, a, a, None, None) == -1
    assert "no HIP device" in native.last_error()


def test_track_problem_shapes():
    cams, idx, obs, off, truth = S.track_problem(50, 5, lengths=(2, 0, 7), n_cameras=16, sigma=1e-3, wrong_frac=0.2,
                                                 dup_frac=0.3)
    assert cams.shape == (16, 14) and off[0] == 0 and off[-1] == len(idx) == len(obs) and truth.shape == (50, 3)
    assert np.array_equal(np.diff(off), np.array([2, 0, 7] * 17)[:50])
    assert idx.min() >= 0 and idx.max() < 16
    again = S.track_problem(50, 5, lengths=(2, 0, 7), n_cameras=16, sigma=1e-3, wrong_frac=0.2, dup_frac=0.3)
    assert all(np.array_equal(a, b) for a, b in zip((cams, idx, obs, off, truth), again))
    same = (idx[1:] == idx[:-1]) & np.all(obs[1:] == obs[:-1], axis=1)
    assert same.any() and (np.abs(obs) > 1.0).any()
    for c in cams:   # lookAt: orthonormal frames
        f, u, r = c[3:6], c[6:9], c[9:12]
        assert abs(f @ f - 1) < 1e-12 and abs(f @ u) < 1e-12 and abs(r @ u) < 1e-12


def test_host_twin_csr_and_dedupe_under_sanitizers(tmp_path):
    """tests/asan/triangulate_asan_main.cpp: a stand-alone program (its own main, nothing preloaded,
    nothing loaded into Python) over triangulate_ref.h, built with -fsanitize=address,undefined: empty
    tracks, single-ray tracks and a track at the cap, rays given and unprojected."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "triangulate_asan"
    src = N.ROOT / "tests" / "asan" / "triangulate_asan_main.cpp"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", f"-I{N.ROOT / 'minicv_amd' / 'csrc'}", str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "triangulate_asan ok" in r.stdout and "ERROR" not in r.stderr
