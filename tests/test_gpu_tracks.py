"""Track building on the GPU: cvBuildTracks against the host twin and the pure-Python reference on the
shared case list (tests/_tracks_ref.py), the order independence of the device union, the launch
counts of DESIGN §7l, and the chain buildTracks -> trackObservations -> triangulateTracks end to end.
Every comparison of tracks is an equality."""
import ctypes as C
import time

import numpy as np
import pytest

import _tracks_ref as R
from minicv_amd import camera as CM
from minicv_amd import native as N

pytestmark = pytest.mark.gpu

# kernel launches, stream synchronisations, copies, memsets of a call: with and without
# trackOfFeature (its copy back is the one difference)
COUNTS_FULL = [N.TRK_LAUNCHES, 2, 7, 1]
COUNTS_NO_MAP = [N.TRK_LAUNCHES, 2, 6, 1]


def stats():
    st = (C.c_longlong * 8)()
    assert N.lib().mcvTestTracksStats(st) == 0
    return list(st)


@pytest.mark.parametrize("name", list(R.CASES))
def test_parity(native, gpu, name):
    c, want = R.case(name), R.expected(name)
    T, twin, _ = R.run("mcvHostBuildTracks", c)
    assert T == want.T
    R.assert_same(twin, want, "host twin")
    T, got, _ = R.run("cvBuildTracks", c)
    assert T == want.T, native.last_error()
    R.assert_same(got, want, "cvBuildTracks")
    R.assert_same(got, twin, "cvBuildTracks against the twin")
    T, got, _ = R.run("cvBuildTracks", c, want_tof=False, want_dropped=False)
    assert T == want.T, native.last_error()
    R.assert_same(got, want, "without trackOfFeature and dropped", tof=False, dropped=False)


def test_both_sort_paths_are_taken(native, gpu):
    """The cut: a component of kTrkShortMax nodes is sorted by one lane, one node more by a workgroup."""
    cut = N.TRK_SHORT_MAX
    for L, nlong in ((cut, 0), (cut + 1, 1), (4096, 1), (4097, 0)):
        T, _, _ = R.run("cvBuildTracks", R.case(f"path_L{L}"))
        st = stats()
        assert T == (1 if L <= 4096 else 0) and st[4:7] == [1 if L <= 4096 else 0, nlong, L - 1], (L, st)
    R.run("cvBuildTracks", R.case("random_scene"))
    st = stats()
    assert st[4] > 1000 and st[6] == int(R.case("random_scene").mask.astype(bool).sum())


@pytest.mark.parametrize("name", ["random_scene", "path_L600", "path_L4096", "duplicate_edges",
                                  "joined_by_the_last_edge", "same_image_and_self_loop", "masked_half",
                                  "min_length_3"])
def test_order_independence(native, gpu, name):
    """The race-order property of the hook: whatever order the edges come in (and the hardware takes
    them in), a component's root is its smallest node, so no output bit changes."""
    want = R.expected(name)
    for seed in (1, 2, 3):
        T, got, _ = R.run("cvBuildTracks", R.case(name).permuted(seed))
        assert T == want.T, native.last_error()
        R.assert_same(got, want, f"{name} permuted {seed}")


def test_scale(native, gpu):
    """The second trips (tests/_tracks_ref.py scale_scene): 2.1 M nodes are more than kTrkScanChunk scan
    blocks, so mcv_trk_scan carries from chunk to chunk (32 candidates, all dropped as conflicts, have their
    roots past the first chunk; no kept track can: the carry of the second scan shows in offsets[T] and T);
    candidates, kept edges, slots and nodes are each more than kTrkGrid x 256, so every grid-stride kernel
    strides; more long candidates than kTrkGrid blocks of mcv_trk_long. Against the by-construction answer
    and the twin; one permuted re-run, the same bits."""
    c, want = R.case("scale"), R.expected("scale")
    assert -(-c.nodes // N.TRK_SCAN_ITEMS) > N.TRK_SCAN_CHUNK and c.nodes > N.TRK_GRID * 256
    T, twin, _ = R.run("mcvHostBuildTracks", c)
    assert T == want.T
    R.assert_same(twin, want, "host twin")
    t0 = time.perf_counter()
    T, got, _ = R.run("cvBuildTracks", c)
    print(f"scale: cvBuildTracks {time.perf_counter() - t0:.3f} s with the buffers of run(), T = {T}")
    assert T == want.T, native.last_error()
    st = stats()
    R.assert_same(got, want, "cvBuildTracks")
    R.assert_same(got, twin, "cvBuildTracks against the twin")
    assert got.dropped.tolist() == [1, R.SCALE_CONFLICTS, 0]
    assert st[:4] == COUNTS_FULL, st
    assert st[4] == want.T + R.SCALE_CONFLICTS and st[4] > N.TRK_GRID * 256 and st[5] > N.TRK_GRID, st
    assert st[6] == int(c.mask.astype(bool).sum()) > N.TRK_GRID * 256 and len(want.cameraIdx) > N.TRK_GRID * 256
    T, got, _ = R.run("cvBuildTracks", c.permuted(1))
    assert T == want.T, native.last_error()
    R.assert_same(got, want, "scale permuted")


def test_contended(native, gpu):
    """One 100,000-node component with 300k edges in random order (dropped as oversize) beside 1,000
    bystanders: the bounded loops of the hook end without the fail word under contended CAS, and the
    outputs are the by-construction ones whatever the edge order. One call per permutation."""
    c, want = R.case("contended"), R.expected("contended")
    assert want.T == 1000 and want.dropped.tolist() == [1, 0, 0]
    for k, p in enumerate((c, c.permuted(1), c.permuted(2))):
        t0 = time.perf_counter()
        T, got, _ = R.run("cvBuildTracks", p)
        print(f"contended: cvBuildTracks {time.perf_counter() - t0:.3f} s, order {k}")
        assert T == want.T, native.last_error()   # a fail word is a refusal: T = -1 with its message
        R.assert_same(got, want, f"contended, order {k}")
        assert stats()[4:6] == [1000, 0]


def test_launch_counts(native, gpu):
    """Launches, synchronisations, copies and memsets do not depend on B, the nodes, the edges or T."""
    seen = {}
    for name in ("one_edge", "random_scene", "path_L4097", "zigzag_long"):
        for form, kw, want in (("full", {}, COUNTS_FULL), ("no map", {"want_tof": False}, COUNTS_NO_MAP)):
            T, _, _ = R.run("cvBuildTracks", R.case(name), **kw)
            assert T == R.expected(name).T, native.last_error()
            assert stats()[:4] == want, (name, form, stats())
            seen[form] = want
    assert seen == {"full": [13, 2, 7, 1], "no map": [13, 2, 6, 1]}
    # a call without a kept match touches no node: the result is known on the host
    for name in ("B0", "all_masked", "empty_problems"):
        T, _, _ = R.run("cvBuildTracks", R.case(name))
        assert T == 0 and stats() == [0] * 8


def test_capacities_on_the_device(native, gpu):
    c, want = R.case("random_scene"), R.expected("random_scene")
    T, got, _ = R.run("cvBuildTracks", c, maxTracks=want.T, maxObs=len(want.cameraIdx))
    assert T == want.T, native.last_error()
    R.assert_same(got, want, "exact capacities")
    T, _, untouched = R.run("cvBuildTracks", c, maxTracks=want.T - 1)
    assert T == -1 and untouched and "do not fit maxTracks" in native.last_error()
    T, _, untouched = R.run("cvBuildTracks", c, maxObs=len(want.cameraIdx) - 1)
    assert T == -1 and untouched and "do not fit maxObs" in native.last_error()
    T, got, _ = R.run("cvBuildTracks", c)   # and the next good call is unaffected
    R.assert_same(got, want, "after a refused call")


def test_end_to_end(native, gpu):
    """12 cameras on a ring, 300 world points, noise-free project1 features in a per-image shuffled
    order, matches of neighbouring cameras from the shared point ids: buildTracks -> trackObservations ->
    triangulateTracks puts every track with a point within 1e-9 of its world point (exact observations
    at scale ~10: rounding of a few ulps amplified by at most 1 / sin 2 deg through the closest-point
    solve, as in test_triangulate.py), and trackOfFeature maps every used feature to its point's track."""
    rng = np.random.default_rng(5)
    nCam, nPts = 12, 300
    world = rng.uniform(-1.0, 1.0, (nPts, 3))
    cams = [CM.lookAt((8 * np.cos(a), 8 * np.sin(a), 1.5), (0, 0, 0), (0, 0, 1), (2.0, 2.0))
            for a in 2 * np.pi * np.arange(nCam) / nCam]
    ids, feats = [], []
    for cam in cams:
        xy, vis = CM.project1(cam, world)
        order = rng.permutation(np.nonzero(vis)[0])
        ids.append(order)              # ids[i][f] = the world point of feature f of image i
        feats.append(xy[order])
    assert all(len(v) > 250 for v in ids)
    imagePairs, pairs, offsets = [], [], [0]
    for i in range(nCam):
        j = (i + 1) % nCam
        slot = np.full(nPts, -1)
        slot[ids[j]] = np.arange(len(ids[j]))
        for f, p in enumerate(ids[i]):
            if slot[p] >= 0:
                pairs.append((f, slot[p]))
        imagePairs.append((i, j))
        offsets.append(len(pairs))
    toff, cam, feat, tof, dropped = CM.buildTracks([len(v) for v in ids], imagePairs, pairs, offsets)
    T = len(toff) - 1
    assert T > 250 and dropped.tolist() == [0, 0, 0]
    obs = CM.trackObservations(feats, cam, feat)
    pts, cnt = CM.triangulateTracks(cams, cam, obs, toff)
    point_of_track = np.array([ids[cam[toff[t]]][feat[toff[t]]] for t in range(T)])
    for t in range(T):   # a track is one world point seen once per camera
        sl = slice(toff[t], toff[t + 1])
        assert all(ids[c][f] == point_of_track[t] for c, f in zip(cam[sl], feat[sl]))
    has = cnt > 0
    assert has.sum() > 250
    assert np.max(np.abs(pts[has] - world[point_of_track[has]])) < 1e-9
    base = np.concatenate([[0], np.cumsum([len(v) for v in ids])])
    track_of_point = np.full(nPts, -1)
    track_of_point[point_of_track] = np.arange(T)
    used = np.zeros(base[-1], bool)
    for i in range(nCam):   # every feature of a point that made a track maps to that track, all others to -1
        want = track_of_point[ids[i]]
        assert np.array_equal(tof[base[i]:base[i + 1]], want)
        used[base[i]:base[i + 1]] = want >= 0
    assert used.sum() == len(cam)
