"""Bundle adjustment on the GPU: cvBundleAdjust equals the host twin bit for bit (cameras,
points, every summary field) on the named cases of tests/_ba_cases.py, which cover every edge of the
kernels' shapes; what a permutation of the tracks may and may not change; the launch, synchronisation
and copy counts; and the chain buildTracks -> trackObservations -> triangulateTracks -> bundleAdjust."""
import ctypes as C
import math
import time

import numpy as np
import pytest

import _ba_cases as B
from minicv_amd import camera as CM
from minicv_amd import native as N

pytestmark = pytest.mark.gpu


def stats():
    st = (C.c_longlong * 8)()
    assert N.lib().mcvTestBundleAdjustStats(st) == 0
    return dict(zip(("launches", "syncs", "copies", "memsets", "linearizations", "trials", "chunks", "segments"), st))


def both(c):
    rt, ct, pt, st = B.run("mcvHostBundleAdjust", c)
    rg, cg, pg, sg = B.run("cvBundleAdjust", c)
    assert rt >= 0 and rg >= 0, N.last_error()
    return (rt, ct, pt, st), (rg, cg, pg, sg)


def assert_equal(twin, got, what):
    (rt, ct, pt, st), (rg, cg, pg, sg) = twin, got
    assert rg == rt, what
    for f in st:
        if isinstance(st[f], float):
            assert B.same_bits([sg[f]], [st[f]]), (what, f, sg[f], st[f])
        else:
            assert sg[f] == st[f], (what, f, sg, st)
    assert B.same_bits(cg, ct), what
    assert B.same_bits(pg, pt), what


@pytest.mark.parametrize("name", list(B.CASES))
def test_export_equals_twin(native, gpu, name):
    """T = 63 / 64 / 65; tracks of 2, 63, 64, 65, 130 and 600 observations (the lane and the wave
    form); cameras with kBaSeg - 1, kBaSeg, kBaSeg + 1, 2 kBaSeg + 3 observations and with none; all and
    no cameras fixed; Huber on and off; rejected steps; every termination code; 255, 256, 257 and 513
    cameras (the second and third trip of the one-workgroup chains over the cameras, the second and third
    block of the per-camera kernels), one of them without an observation, one more fixed,
    the last camera of 257 and of 513 (alone in its trip) free and observed."""
    c = B.case(name)
    twin, got = both(c)
    assert_equal(twin, got, name)
    sm = got[3]
    if name.startswith("cameras_"):
        nCam = int(name.split("_")[1])
        empty, alsoFixed = B.camera_ring_special(nCam)
        assert len(c.cams) == nCam and (nCam <= 257 or min(empty, alsoFixed) >= 256)
        if nCam > 256:   # the last trip of the chains over the cameras holds one camera, and it moves
            assert nCam % 256 == 1 and not B.same_bits(got[1][nCam - 1], c.cams[nCam - 1])
        assert B.same_bits(got[1][[0, 1, alsoFixed, empty]], c.cams[[0, 1, alsoFixed, empty]])
        assert sm["accepted"] > 0 and sm["cgIterations"] > 0 and sm["usedObservations"] == len(c.idx)
    if name in B.TERMINATION:
        assert sm["termination"] == B.TERMINATION[name]
    if name == "rejected":
        assert sm["rejected"] > 0 and sm["accepted"] > 0
    if name == "track_lengths":
        assert np.diff(c.off).tolist()[:6] == [2, 63, 64, 65, 130, 600] and sm["usedTracks"] == 12
    if name == "segment_edges":
        S = N.BA_SEG
        assert np.bincount(c.idx, minlength=6).tolist()[:4] == [S - 1, S, S + 1, 2 * S + 3]
        assert sm["usedObservations"] == len(c.idx) and stats()["segments"] == 1 + 1 + 2 + 3 + 1
    if name == "all_fixed":
        assert B.same_bits(got[1], c.cams) and sm["cgIterations"] == 0 and sm["accepted"] > 0
    if name == "exclusions":
        for t in (3, 7, 12):
            assert B.same_bits(got[2][t], c.pts[t])
        assert B.same_bits(got[1][:2], c.cams[:2])
    if sm["accepted"] > 0:
        assert sm["finalCost"] < sm["initialCost"]


@pytest.mark.parametrize("name", ["exclusions", "track_lengths", "all_fixed", "cameras_257"])
def test_track_permutation(native, gpu, name):
    """The per-point sums follow the track's own order and the per-camera sums the ascending observation
    index, so permuting the tracks regroups only the camera-side sums and the total cost. What must
    stay equal, bit for bit: the used counts; the points of excluded tracks and the cameras that stay
    constant (inputs handed back); and, with every camera fixed, every point and the iteration counts
    (a point's step is Vinv h of its own track alone; the cost only decides acceptance, checked through
    the equal counts). Everything else stays equal to the twin of the permuted call, and moves by
    rounding only (1e-9)."""
    c = B.case(name)
    base = B.run("cvBundleAdjust", c)
    for seed in (1, 2):
        p, order = B.permuted(c, seed)
        twin, got = both(p)
        assert_equal(twin, got, (name, seed))
        _, cg, pg, sg = got
        assert (sg["usedObservations"], sg["usedTracks"]) == (base[3]["usedObservations"], base[3]["usedTracks"])
        want = base[2][order]
        excluded = np.array([B.same_bits(c.pts[t], base[2][t]) for t in order])
        assert B.same_bits(pg[excluded], want[excluded])
        fixed = c.fixed.astype(bool)
        assert B.same_bits(cg[fixed], c.cams[fixed])
        if name == "all_fixed":
            assert B.same_bits(pg, want) and B.same_bits(cg, base[1])
            assert [sg[f] for f in ("iterations", "accepted", "rejected")] == [base[3][f] for f in ("iterations", "accepted", "rejected")]
        else:
            ok = np.isfinite(want).all(axis=1)
            assert np.abs(pg[ok] - want[ok]).max() < 1e-9 and np.abs(cg - base[1]).max() < 1e-9


def test_scale(native, gpu):
    """More observations than kBaGrid x 256 threads (mcv_ba_used_obs strides), more long tracks than the
    4 kBaLongBlocks waves of the long-track kernels, T >= 1024, several segments per camera: cameras,
    points and every summary field equal the twin's bit for bit, and both costs are numpy's own
    evaluation of the model within 1e-12 (against its pairwise sum and against math.fsum of its terms)."""
    c = B.case("scale")
    n, T, L = len(c.idx), len(c.off) - 1, np.diff(c.off)
    assert n > N.BA_GRID * 256 and int((L > N.BA_SHORT_MAX).sum()) > 4 * N.BA_LONG_BLOCKS and T >= 1024
    assert c.cfg["maxCgIterations"] == N.BA_CG_CHUNK and c.cfg["maxIterations"] == 2 and c.cfg["huberDelta"] > 0
    t0 = time.perf_counter()
    got = B.run("cvBundleAdjust", c)
    t1 = time.perf_counter()
    twin = B.run("mcvHostBundleAdjust", c)
    print(f"scale: cvBundleAdjust {t1 - t0:.3f} s, the twin {time.perf_counter() - t1:.3f} s")
    assert got[0] >= 0 and twin[0] >= 0, N.last_error()
    st = stats()
    assert_equal(twin, got, "scale")
    sm = got[3]
    assert sm["usedTracks"] == T and sm["usedObservations"] == n and sm["iterations"] == 2
    assert st["segments"] == int(np.sum(-(-np.bincount(c.idx, minlength=len(c.cams)) // N.BA_SEG))) > 3 * len(c.cams)
    used = np.ones(n, bool)
    for what, cams, pts in (("initialCost", c.cams, c.pts), ("finalCost", got[1], got[2])):
        terms = B.cost_terms_v(cams, pts, c.idx, c.obs, c.off, used, c.cfg["huberDelta"])
        pairwise, exact = float(terms.sum()), math.fsum(terms)
        print(f"scale: {what} {sm[what]!r}, relative to numpy's sum {abs(sm[what] - pairwise) / pairwise:.3e}, "
              f"to fsum {abs(sm[what] - exact) / exact:.3e}")
        assert abs(sm[what] - pairwise) <= 1e-12 * pairwise and abs(sm[what] - exact) <= 1e-12 * exact
    assert sm["finalCost"] < sm["initialCost"] and sm["accepted"] > 0


def test_fixed_costs(native, gpu):
    """Launches, synchronisations and copies per LM iteration and per chunk of PCG iterations do not
    depend on T, the observations or nCameras: the counts at (T, nCameras) = (65, 3) and (4000, 40) follow
    one formula, and are equal when the linearisations, trials and chunks are."""
    L = N.BA_LAUNCHES
    seen = []
    for T, nCam, lens in ((65, 3, None), (4000, 40, 5)):
        c = B.scene(60 + nCam, nCam, T, lengths=None if lens is None else [lens] * T, functionTolerance=0.0,
                    maxIterations=3, maxCgIterations=N.BA_CG_CHUNK)
        ret, _, _, sm = B.run("cvBundleAdjust", c)
        st = stats()
        assert ret == 3 == st["trials"] and st["chunks"] == 3, (sm, st, N.last_error())
        lin, tr, ch = st["linearizations"], st["trials"], st["chunks"]
        assert st["launches"] == L["setup"] + L["cost"] + L["linearize"] * lin + (L["system"] + L["trial"]) * tr + \
            L["cg_iter"] * N.BA_CG_CHUNK * ch
        assert st["syncs"] == 2 + ch + tr + 1           # the used counts, the first cost, ..., the results
        assert st["copies"] == 12 + 2 + ch + tr + 2     # 12 uploads, the two records above, ..., two results
        assert st["memsets"] == 2 + tr
        seen.append((lin, tr, ch, st["launches"], st["syncs"], st["copies"], st["memsets"]))
    assert seen[0] == seen[1], seen


def test_end_to_end(native, gpu):
    """The ring of 12 cameras of test_gpu_tracks.py, built afresh, with noise on the features and on
    the cameras handed to the triangulation: buildTracks -> trackObservations -> triangulateTracks ->
    bundleAdjust ends below the cost at the triangulated points."""
    rng = np.random.default_rng(5)
    nCam, nPts = 12, 300
    world = rng.uniform(-1.0, 1.0, (nPts, 3))
    cams = [CM.lookAt((8 * np.cos(a), 8 * np.sin(a), 1.5), (0, 0, 0), (0, 0, 1), (2.0, 2.0))
            for a in 2 * np.pi * np.arange(nCam) / nCam]
    ids, feats = [], []
    for cam in cams:
        xy, vis = CM.project1(cam, world)
        order = rng.permutation(np.nonzero(vis)[0])
        ids.append(order)
        feats.append(xy[order] + rng.normal(0, 5e-4, (len(order), 2)))
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
    toff, cam, feat, _, dropped = CM.buildTracks([len(v) for v in ids], imagePairs, pairs, offsets)
    T = len(toff) - 1
    assert T > 250 and dropped.tolist() == [0, 0, 0]
    obs = CM.trackObservations(feats, cam, feat)
    start = CM.cameras_array(cams)
    for j in range(2, nCam):   # the cameras of a PnP or two-view solve: a little off
        start[j] = B.retract(start[j], np.concatenate([rng.normal(0, 2e-3, 3), rng.normal(0, 5e-3, 3)]))
    pts, cnt = CM.triangulateTracks(start, cam, obs, toff)
    fixed = np.zeros(nCam, np.uint8)
    fixed[:2] = 1
    outC, outP, sm = CM.bundleAdjust(start, cam, obs, toff, pts, fixed)
    used = B.used_set(start, pts, cam, obs, toff)
    assert sm["usedObservations"] == used.sum() and sm["usedTracks"] >= (cnt > 0).sum() - 5 > 250
    at_triangulated = B.cost(start, pts, cam, obs, toff, used)
    assert abs(sm["initialCost"] - at_triangulated) <= 1e-12 * at_triangulated
    assert sm["accepted"] > 0 and sm["finalCost"] < 0.5 * at_triangulated
    assert abs(sm["finalCost"] - B.cost(outC, outP, cam, obs, toff, used)) <= 1e-12 * sm["finalCost"]
    assert B.same_bits(outC[:2], start[:2]) and B.same_bits(outP[cnt == 0], pts[cnt == 0])
    point_of_track = np.array([ids[cam[toff[t]]][feat[toff[t]]] for t in range(T)])
    has = cnt > 0
    before = np.linalg.norm(pts[has] - world[point_of_track[has]], axis=1).mean()
    after = np.linalg.norm(outP[has] - world[point_of_track[has]], axis=1).mean()
    assert after < before
