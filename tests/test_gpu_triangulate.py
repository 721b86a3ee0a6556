"""Track triangulation on the GPU: cvIntersectRays, cvTriangulateTracks and mcvTriangulateTracksDevice
against the host twin and the pure-Python reference (_triangulate_ref.ref_intersection), bit for bit:
points, pair counts, cost and visible. The cases and their reference answers are shared with
tests/test_triangulate.py and computed once."""
import ctypes as C
import time
from collections import Counter

import numpy as np
import pytest

import _triangulate_ref as R
from minicv_amd import camera as CM
from minicv_amd import native as N
from minicv_amd import synthetic as S

pytestmark = pytest.mark.gpu

CUT = N.TRI_SHORT_MAX


def device_call(p, stats=True, offsets=None, idx=None, null_cost=False, null_visible=False):
    """mcvTriangulateTracksDevice on torch tensors (at least one element each: an empty tensor has no
    storage). -> (return value, untouched, (points, counts, cost, visible))."""
    import torch
    off = p.offsets if offsets is None else np.ascontiguousarray(offsets, np.int32)
    idx = p.idx if idx is None else np.ascontiguousarray(idx, np.int32)
    T = off.size - 1

    def dev(a, shape):
        return torch.from_numpy(np.ascontiguousarray(a if a.size else np.zeros(shape, a.dtype))).cuda()
    cams, di, do, doff = dev(p.cams, (1, 14)), dev(idx, 1), dev(p.obs, (1, 2)), dev(off, 1)
    pts, cnt, cost, vis = (torch.from_numpy(a).cuda() for a in R.sentinels(max(T, 1)))
    torch.cuda.synchronize()
    k = N.lib().mcvTriangulateTracksDevice(cams.data_ptr(), p.cams.shape[0], di.data_ptr(), do.data_ptr(),
                                           doff.data_ptr(), T, pts.data_ptr(), cnt.data_ptr(),
                                           cost.data_ptr() if stats and not null_cost else None,
                                           vis.data_ptr() if stats and not null_visible else None)
    out = tuple(a.cpu().numpy() for a in (pts, cnt, cost, vis))
    untouched = np.all(out[0] == 7.0) and np.all(out[1] == -7) and np.all(out[2] == 7.0) and np.all(out[3] == -7)
    return k, untouched, out


def check_case(native, gpu, name):
    """All three exports == the reference == the host twin on one shared case."""
    p = R.problem(name)
    assert p.enough_points(), "the case hides failures: fewer than half of its tracks have a point"
    want = int((p.counts > 0).sum())
    k, hp, hc, hcost, hvis = R.host_tracks(p)
    assert k == want
    R.assert_same((hp, hc, hcost, hvis), p, "host twin")
    k, _, out = R.call_export("cvIntersectRays", p)
    assert k == want, native.last_error()
    R.assert_same(tuple(a[:p.T] for a in out[:2]), p, "cvIntersectRays")
    k, _, out = R.call_export("cvTriangulateTracks", p)
    assert k == want, native.last_error()
    R.assert_same(tuple(a[:p.T] for a in out), p, "cvTriangulateTracks")
    assert np.array_equal(R.bits(out[0][:p.T]), R.bits(hp)) and np.array_equal(R.bits(out[2][:p.T]), R.bits(hcost))
    k, _, out = device_call(p)
    assert k == want, native.last_error()
    R.assert_same(tuple(a[:p.T] for a in out), p, "mcvTriangulateTracksDevice")
    return p


# ---- empty and minimal tracks

@pytest.mark.parametrize("name", ["empty_and_minimal", "all_tracks_empty"])
def test_empty_and_minimal_tracks(native, gpu, name):
    p = check_case(native, gpu, name)
    small = p.lengths() < 2
    assert small.any() and np.all(p.counts[small] == 0) and np.all(np.isnan(p.points[small]))
    k, _, out = R.call_export("cvTriangulateTracks", p)
    assert np.all(out[1][:p.T][small] == 0) and np.all(np.isnan(out[0][:p.T][small]))
    assert np.all(np.isinf(out[2][:p.T][small])) and np.all(out[3][:p.T][small] == 0)
    if name == "all_tracks_empty":
        assert k == 0 and p.rays.shape[0] == 0


def test_empty_and_minimal_tracks_T0(native, gpu):
    p = R.problem("empty_and_minimal")
    for name in ("cvIntersectRays", "cvTriangulateTracks"):
        k, untouched, _ = R.call_export(name, p, offsets=[0])
        assert k == 0 and untouched and native.last_error() == ""
    k, untouched, _ = device_call(p, offsets=[0])
    assert k == 0 and untouched
    pts, cnt = CM.triangulateTracks(p.cams, [], np.zeros((0, 2)), [0])
    assert pts.shape == (0, 3) and cnt.shape == (0,)


# ---- wave edges

@pytest.mark.parametrize("T", [1, 63, 64, 65, 257])
def test_wave_edges(native, gpu, T):
    p = check_case(native, gpu, f"wave_edges_T{T}")
    assert p.T == T


# ---- track-length edges

@pytest.mark.parametrize("name", ["length_cutoff", "length_R63", "length_R64", "length_R65", "length_R130",
                                  "length_R600"])
def test_track_length_edges(native, gpu, name):
    p = check_case(native, gpu, name)
    st = (C.c_longlong * 8)()
    k, _, _ = R.call_export("cvIntersectRays", p)
    assert N.lib().mcvTestTriangulateStats(st) == 0
    nlong = int((p.lengths() > CUT).sum())
    assert st[5] == nlong and st[4] == p.T - nlong and nlong >= 1
    if name == "length_cutoff":
        assert set(p.lengths().tolist()) == {CUT - 1, CUT, CUT + 1} and st[4] >= 2
    if name == "length_R600":   # several pair tiles, and kept rays beyond the ones held in LDS
        assert p.counts[0] > 100000


# ---- duplicates

def test_duplicates(native, gpu):
    p = check_case(native, gpu, "duplicates")
    assert p.counters["duplicate"] >= 12
    assert p.lengths()[3] == 5 and p.counts[3] == 0        # all duplicates: one ray is left, no pair
    assert p.lengths()[4] > CUT and p.counts[4] > 0        # the long-track kernel's dedupe
    # first / last / adjacent repeats leave the pairs of the four distinct rays
    assert all(0 < p.counts[t] <= 6 for t in (0, 1, 2))


# ---- angle threshold

def test_angle_threshold(native, gpu):
    p = check_case(native, gpu, "angle_threshold")
    two = p.counts[:48]
    assert 8 <= int((two == 1).sum()) <= 40 and set(two.tolist()) == {0, 1}   # both sides of 2 deg are hit
    assert p.counters["accepted_near_threshold"] >= 8 and p.counters["angle"] >= 8
    assert p.counts[48] == 0 and p.counts[49] == 0         # parallel rays; rays from one origin


# ---- rays behind the origin

def test_rays_behind_the_origin(native, gpu):
    p = check_case(native, gpu, "rays_behind_origin")
    assert p.counters["behind"] >= 6
    assert np.all(p.counts[:6] >= 1) and np.all(p.counts[:6] < 3)


# ---- non-finite midpoints

def test_non_finite_midpoints(native, gpu):
    p = check_case(native, gpu, "nonfinite_midpoints")
    assert p.counters["nonfinite"] >= 2
    assert p.counts[0] == 0 and np.all(np.isnan(p.points[0]))


# ---- statistics

def test_statistics(native, gpu):
    p = check_case(native, gpu, "statistics")
    assert (np.abs(p.obs) > 1.0).any()                                   # observations outside the image
    has = p.counts > 0
    assert (p.visible[has] < p.lengths()[has]).any() and (p.visible[has] > 0).any()
    behind = slice(p.T - 5, p.T)                                         # the camera that looks away
    assert np.all(p.visible[behind] == 2) and np.all(p.counts[behind] == 1)
    # cost / visible are optional, one at a time and both
    k, _, out = R.call_export("cvTriangulateTracks", p, stats=False)
    R.assert_same(tuple(a[:p.T] for a in out[:2]), p, "no statistics")
    assert np.all(out[2] == 7.0) and np.all(out[3] == -7)
    for null in ("cost", "vis"):
        k, _, out = R.call_export("cvTriangulateTracks", p, null=null)
        assert k == int(has.sum()), native.last_error()
        got = [a[:p.T] for a in out]
        assert np.all(out[2 if null == "cost" else 3] == (7.0 if null == "cost" else -7))
        got[2 if null == "cost" else 3] = None
        R.assert_same(tuple(got), p, f"null {null}")
    for kw in ({"stats": False}, {"null_cost": True}, {"null_visible": True}):
        k, _, out = device_call(p, **kw)
        assert k == int(has.sum()), native.last_error()
        got = [a[:p.T] for a in out]
        if kw.get("stats") is False or kw.get("null_cost"):
            assert np.all(out[2] == 7.0)
            got[2] = None
        if kw.get("stats") is False or kw.get("null_visible"):
            assert np.all(out[3] == -7)
            got[3] = None
        R.assert_same(tuple(got), p, f"device {kw}")
    pts, cnt, cost, vis = CM.triangulateTracks(p.cams, p.idx, p.obs, p.offsets, stats=True)
    R.assert_same((pts, cnt, cost, vis), p, "camera.triangulateTracks")
    pts, cnt = CM.intersectRays(p.rays, p.offsets)
    R.assert_same((pts, cnt), p, "camera.intersectRays")
    t = int(np.nonzero(has)[0][0])
    one = CM.intersection(p.rays[p.offsets[t]:p.offsets[t + 1]])
    assert np.array_equal(R.bits(one), R.bits(p.points[t]))
    assert CM.intersection(p.rays[:1]) is None


# ---- validation

def _bad_calls(p):
    off = p.offsets.copy()
    off[0] = 1
    yield "bad_offsets_start", {"offsets": off}, "offsets[0]", True
    off = p.offsets.copy()
    off[3] = off[2] - 1
    yield "bad_offsets_decrease", {"offsets": off}, "decrease at track 2", True
    idx = p.idx.copy()
    idx[7] = p.cams.shape[0]
    yield "camera_idx_high", {"idx": idx}, "cameraIdx[7]", False
    idx = p.idx.copy()
    idx[0] = -1
    yield "camera_idx_negative", {"idx": idx}, "cameraIdx[0]", False
    yield "track_4097", {"offsets": [0, 2, 2 + N.MAX_TRACK_LEN + 1]}, "track 1 has 4097 rays", True


@pytest.mark.parametrize("which", ["bad_offsets_start", "bad_offsets_decrease", "camera_idx_high",
                                   "camera_idx_negative", "track_4097"])
def test_validation(native, gpu, which):
    """A refused call has a message and leaves every output as it was, on all three exports."""
    p = R.problem("length_cutoff")
    (kw, word, ray_form), = [(a, b, c) for n, a, b, c in _bad_calls(p) if n == which]
    if ray_form:
        k, untouched, _ = R.call_export("cvIntersectRays", p, **kw)
        assert k == -1 and untouched and word in native.last_error()
    k, untouched, _ = R.call_export("cvTriangulateTracks", p, **kw)
    assert k == -1 and untouched and word in native.last_error()
    if which == "track_4097":   # the device call reads what the offsets name: give it that many observations
        n = 2 + N.MAX_TRACK_LEN + 1
        q = R.Problem.__new__(R.Problem)
        q.cams, q.idx, q.obs, q.offsets = p.cams, np.zeros(n, np.int32), np.zeros((n, 2)), p.offsets
        k, untouched, _ = device_call(q, **kw)
    else:
        k, untouched, _ = device_call(p, **kw)
    assert k == -1 and untouched and word in native.last_error()
    # and the next good call is unaffected
    k, _, out = device_call(p)
    R.assert_same(tuple(a[:p.T] for a in out), p, "after a refused call")


# ---- launch counts

def test_launch_counts(native, gpu):
    """Launches, synchronisations, copies and memsets depend on the export and on whether statistics
    are asked for, not on T (the numbers are DESIGN §7i's)."""
    st = (C.c_longlong * 8)()

    def counts(call):
        call()
        assert N.lib().mcvTestTriangulateStats(st) == 0
        return list(st)[:4], list(st)[4:6]
    seen = {}
    for T in (64, 4096):
        cams, idx, obs, off, _ = S.track_problem(T, 90 + T, lengths=(2, 3, 5, CUT + 4, 8))
        p = R.Problem.__new__(R.Problem)
        p.cams, p.idx, p.obs, p.offsets, p.T = cams, idx, np.ascontiguousarray(obs), off, T
        p.rays = np.zeros((len(idx), 6))
        p.rays[:, 3] = 1.0
        for form, call in (("rays", lambda: R.call_export("cvIntersectRays", p)),
                           ("tracks", lambda: R.call_export("cvTriangulateTracks", p, stats=False)),
                           ("tracks+stats", lambda: R.call_export("cvTriangulateTracks", p)),
                           ("device", lambda: device_call(p, stats=False)),
                           ("device+stats", lambda: device_call(p))):
            c, classes = counts(call)
            nlong = int((np.diff(off) > CUT).sum())
            assert classes == [T - nlong, nlong] and nlong > 0
            assert seen.setdefault(form, c) == c, (form, T, c, seen[form])
    assert seen == {"rays": [2, 1, 5, 1], "tracks": [3, 1, 7, 1], "tracks+stats": [4, 1, 9, 1],
                    "device": [5, 2, 3, 1], "device+stats": [6, 2, 3, 1]}


# ---- device export

def test_device_export(native, gpu):
    """mcvTriangulateTracksDevice on torch tensors == the host-pointer call, on a case with both track
    classes, noise, wrong observations and duplicates."""
    cams, idx, obs, off, _ = S.track_problem(700, 95, lengths=(2, 3, 4, 6, 9, 12, CUT, CUT + 1, 40), n_cameras=64,
                                             sigma=1e-3, wrong_frac=0.1, dup_frac=0.05)
    p = R.Problem.__new__(R.Problem)
    p.cams, p.idx, p.obs, p.offsets, p.T = cams, idx, np.ascontiguousarray(obs), off, 700
    p.rays = np.zeros((1, 6))
    k1, _, a = R.call_export("cvTriangulateTracks", p)
    k2, _, b = device_call(p)
    k3, hp, hc, hcost, hvis = R.host_tracks(p)
    assert k1 == k2 == k3 > 350, native.last_error()
    for x, y, z in zip(a, b, (hp, hc, hcost, hvis)):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)) and np.array_equal(x.view(np.uint8), z.view(np.uint8))


# ---- scale: the second trips of the grid-stride kernels and of the long-track queue

def test_scale(native, gpu):
    """n > kTriGrid x 256 observations (mcv_tri_unproject and mcv_tri_check_cameras stride) and more
    long tracks than the 8 kTriGrid blocks of mcv_tri_long: all three exports and the device export
    equal the host twin bit for bit, and the pure-Python reference on a seeded sample of 256 tracks."""
    p = R.scale()
    assert p.n > N.TRI_GRID * 256 and p.nLong > 8 * N.TRI_GRID and p.T > 8 * N.TRI_GRID
    assert p.ref.enough_points(), "the sample hides failures: fewer than half of its tracks have a point"
    k, hp, hc, hcost, hvis = R.host_tracks(p)
    twin = (hp, hc, hcost, hvis)
    assert k == int((hc > 0).sum()) > p.T // 2
    p.assert_sample(twin, "host twin")
    st = (C.c_longlong * 8)()
    for name, call in (("cvIntersectRays", lambda: R.call_export("cvIntersectRays", p)),
                       ("cvTriangulateTracks", lambda: R.call_export("cvTriangulateTracks", p)),
                       ("mcvTriangulateTracksDevice", lambda: device_call(p))):
        t0 = time.perf_counter()
        kk, _, out = call()
        print(f"scale: {name} {time.perf_counter() - t0:.3f} s")
        assert kk == k, (name, kk, k, native.last_error())
        assert N.lib().mcvTestTriangulateStats(st) == 0 and list(st)[4:6] == [p.T - p.nLong, p.nLong]
        got = out[:2] if name == "cvIntersectRays" else out
        R.assert_bits(got, twin, name)
        p.assert_sample(got, name)


def test_validation_at_scale(native, gpu):
    """A bad cameraIdx beyond the first trip of mcv_tri_check_cameras, and at the last observation:
    the exports refuse, name the first bad index, write nothing, and the next good call is unaffected."""
    p = R.scale()
    first, last = N.TRI_GRID * 256 + 3, p.n - 1
    assert first < last
    for bad, named in (((first, last), first), ((last,), last)):
        idx = p.idx.copy()
        idx[list(bad)] = p.cams.shape[0]
        k, untouched, _ = R.call_export("cvTriangulateTracks", p, idx=idx)
        assert k == -1 and untouched and f"cameraIdx[{named}]" in native.last_error(), native.last_error()
        k, untouched, _ = device_call(p, idx=idx)
        assert k == -1 and untouched and f"cameraIdx[{named}]" in native.last_error(), native.last_error()
    k, hp, hc, hcost, hvis = R.host_tracks(p)
    kk, _, out = device_call(p)
    assert kk == k, native.last_error()
    R.assert_bits(out, (hp, hc, hcost, hvis), "after a refused call")


# ---- every subject above has its test, and none of them is switched off

def test_every_subject_has_its_test():
    subjects = ("test_empty_and_minimal_tracks", "test_empty_and_minimal_tracks_T0", "test_wave_edges",
                "test_track_length_edges", "test_duplicates", "test_angle_threshold", "test_rays_behind_the_origin",
                "test_non_finite_midpoints", "test_statistics", "test_validation", "test_launch_counts",
                "test_device_export", "test_reference_conditions", "test_scale", "test_validation_at_scale")
    for name in subjects:
        f = globals().get(name)
        assert callable(f), f"{name} is missing"
        marks = {m.name for m in getattr(f, "pytestmark", [])}
        assert not marks & {"skip", "skipif", "xfail"}, f"{name} is switched off"


# ---- the conditions that keep these tests from hiding failures, on the reference alone

def test_reference_conditions():
    total = Counter()
    for name in R.CASES:
        p = R.problem(name)
        assert p.enough_points(), name
        total.update(p.counters)
    for branch in ("angle", "behind", "duplicate", "nonfinite"):
        assert total[branch] >= 1, branch
    assert total["accepted_near_threshold"] >= 1
