"""Track building on the CPU: the host twin (mcvHostBuildTracks, tracks_ref.h) against the independent
pure-Python reference on the shared case list, the order independence of the definition, every
refusal of the ABI, the declarations, and the twin under AddressSanitizer + UBSan in a stand-alone
program. Everything is integer arithmetic: every comparison is an equality. No kernel is launched."""
import shutil
import subprocess

import numpy as np
import pytest

import _tracks_ref as R
from minicv_amd import camera as CM
from minicv_amd import native as N

EXPORTS = ("cvBuildTracks", "mcvHostBuildTracks", "mcvTestTracksStats")
BOTH = ("cvBuildTracks", "mcvHostBuildTracks")


@pytest.mark.parametrize("name", list(R.CASES))
def test_twin_equals_reference(native, name):
    c, want = R.case(name), R.expected(name)
    T, got, _ = R.run("mcvHostBuildTracks", c)
    assert T == want.T, native.last_error()
    R.assert_same(got, want, name)
    # the invariants of the definition, on the reference itself
    assert np.all(np.diff(want.trackOffsets) >= c.minLength) and np.all(np.diff(want.trackOffsets) <= R.MAX_LEN)
    for t in range(want.T):
        cams = want.cameraIdx[want.trackOffsets[t]:want.trackOffsets[t + 1]]
        assert np.all(np.diff(cams) > 0)   # ascending by image, one node per image


def test_random_scene_has_every_drop_class():
    """Seed 11 of _tracks_ref.random_scene: 33194 matches; the reference finds 978 tracks with 7902
    observations and drops 1 oversize component, 200 conflicts and 706 short ones (minLength 3)."""
    assert R.RANDOM_SEED == 11
    c, want = R.case("random_scene"), R.expected("random_scene")
    assert c.counts.tolist() == [500] * 64 and len(c.problems) == 200 and int(c.offsets[-1]) == 33194
    assert 0.08 < 1.0 - c.mask.mean() < 0.12
    assert (want.T, len(want.cameraIdx)) == (978, 7902) and want.dropped.tolist() == [1, 200, 706]


def test_case_list_covers_the_cuts():
    """The path lengths straddle the short / long cut of the kernels and the cap."""
    cut = N.TRK_SHORT_MAX
    assert {cut - 1, cut, cut + 1, R.MAX_LEN, R.MAX_LEN + 1} <= set(R.PATH_LENGTHS)
    assert R.expected("path_L4096").T == 1 and R.expected("path_L4097").dropped.tolist() == [1, 0, 0]
    assert R.expected("zigzag_long").dropped.tolist() == [0, 1, 0]      # more nodes than images, over the cut
    assert R.expected("long_conflict").dropped.tolist() == [0, 1, 0]    # within nImages, over the cut
    assert R.expected("same_image_and_self_loop").dropped.tolist() == [0, 1, 1]
    for o in ("descending", "shuffled"):
        R.assert_same(R.expected(f"path_L600_{o}"), R.expected("path_L600"), o)


def test_scan_block_edges():
    """The scan cases put roots and last members on the edges of the kTrkScanItems-node scan blocks and
    of the eight-node runs of a thread, for every nNodes around one and two blocks."""
    S = N.TRK_SCAN_ITEMS
    assert R.SCAN_NODES == (S - 1, S, S + 1, 2 * S, 2 * S + 1) and {n % 8 for n in R.SCAN_NODES} == {0, 1, 7}
    base = lambda c: np.concatenate([[0], np.cumsum(c.counts)])
    roots = {name: (base(R.case(name))[R.expected(name).cameraIdx] + R.expected(name).featureIdx)
             [R.expected(name).trackOffsets[:-1]].tolist() for name in R.SCAN_CASES}
    for n in R.SCAN_NODES:
        assert R.case(f"scan_{n}_tail").nodes == n and roots[f"scan_{n}_tail"] == [n - 2]
        assert R.expected(f"scan_{n}_tail").trackOfFeature.tolist() == [-1] * (n - 2) + [0, 0]
        assert roots[f"scan_{n}_ends"][0] == 0 and R.expected(f"scan_{n}_ends").trackOfFeature[n - 1] == 0
    assert roots[f"scan_{2 * S}_ends"] == [0, S - 1] and roots[f"scan_{2 * S + 1}_root_S"] == [5, S]
    assert roots[f"scan_{S + 1}_tail"] == [S - 1]       # the root S - 1 with its partner S, nothing else
    assert all(R.expected(name).dropped.tolist() == [0, 0, 0] for name in R.SCAN_CASES)


def scale_sizes(c):
    """Of a scene: nodes, scan blocks, kept edges, matches."""
    kept = len(c.pairs) if c.mask is None else int(c.mask.astype(bool).sum())
    return c.nodes, -(-c.nodes // N.TRK_SCAN_ITEMS), kept, len(c.pairs)


def test_scale_scene_is_a_second_trip_case():
    """What makes `scale` a second-trip case, from the mirrored constants: more scan blocks than one
    chunk of mcv_trk_scan (the carry), more candidates, kept edges and slots than a grid of threads,
    more long candidates than blocks of mcv_trk_long; all three drop counters by construction."""
    c, want = R.case("scale"), R.expected("scale")
    nodes, nb, kept, matches = scale_sizes(c)
    sizes = np.diff(want.trackOffsets)
    assert nb > N.TRK_SCAN_CHUNK and kept > N.TRK_GRID * 256 and nodes > N.TRK_GRID * 256
    assert want.T + int(want.dropped[1]) > N.TRK_GRID * 256            # candidates: the tracks and the conflicts
    assert len(want.cameraIdx) > N.TRK_GRID * 256                      # slots
    assert int((sizes > N.TRK_SHORT_MAX).sum()) > N.TRK_GRID           # long candidates
    assert 0.09 < 1.0 - kept / matches < 0.11 and want.dropped.tolist() == [1, R.SCALE_CONFLICTS, 0]
    # candidates with their root in the scan blocks past the first chunk of kTrkScanChunk: the same-image pairs
    prob = np.repeat(np.arange(len(c.imagePairs)), np.diff(c.offsets))
    last = np.all(c.imagePairs[prob] == len(c.counts) - 1, axis=1) & c.mask.astype(bool)
    lo = (len(c.counts) - 1) * int(c.counts[0]) + c.pairs[last].min(axis=1)
    assert int((lo >= N.TRK_SCAN_CHUNK * N.TRK_SCAN_ITEMS).sum()) == 32           # (the oversize tree has same-image edges too)
    assert R.OVERSIZE == R.MAX_LEN + 904
    c, want = R.case("contended"), R.expected("contended")
    assert want.T == 1000 and want.dropped.tolist() == [1, 0, 0] and len(c.pairs) > 300000
    assert np.all(np.diff(want.trackOffsets) == 3)


def test_by_construction_equals_reference():
    """The by-construction answer of the large generator is the pure-Python reference's on its 1 / 40
    sub-scene (every class of component of the full scene, the oversize one at full size)."""
    c, want = R.case("scale_sub40"), R.expected("scale_sub40")
    assert c.nodes == 40 * (52500 // 40) and want.dropped[0] == 1 and want.dropped[1] > 0
    assert int((np.diff(want.trackOffsets) > N.TRK_SHORT_MAX).sum()) == 2100 // 40
    R.assert_same(want, R.reference(c), "by construction against reference()")


@pytest.mark.parametrize("name", list(R.LARGE))
def test_twin_on_the_large_scenes(native, name):
    c, want = R.case(name), R.expected(name)
    T, got, _ = R.run("mcvHostBuildTracks", c)
    assert T == want.T, native.last_error()
    R.assert_same(got, want, name)
    p = c.permuted(1)
    assert not np.array_equal(p.pairs, c.pairs) and len(p.pairs) == len(c.pairs)
    T, got, _ = R.run("mcvHostBuildTracks", p)
    assert T == want.T, native.last_error()
    R.assert_same(got, want, f"{name} permuted")


@pytest.mark.parametrize("name", ["random_scene", "path_L600", "duplicate_edges", "joined_by_the_last_edge",
                                  "same_image_and_self_loop", "masked_half", "min_length_3"])
def test_order_independence(native, name):
    want = R.expected(name)
    changed = False
    for seed in (1, 2, 3):
        p = R.case(name).permuted(seed)
        changed = changed or not np.array_equal(p.imagePairs, R.case(name).imagePairs) or \
            not np.array_equal(p.pairs, R.case(name).pairs)
        T, got, _ = R.run("mcvHostBuildTracks", p)
        assert T == want.T, native.last_error()
        R.assert_same(got, want, f"{name} permuted {seed}")
    assert changed, "every permutation was the identity"


def test_optional_outputs(native):
    c, want = R.case("min_length_3"), R.expected("min_length_3")
    for tof, dropped in ((False, True), (True, False), (False, False)):
        T, got, _ = R.run("mcvHostBuildTracks", c, want_tof=tof, want_dropped=dropped)
        assert T == want.T
        R.assert_same(got, want, "optional", tof=tof, dropped=dropped)


def _refusals():
    c = R.case("min_length_3")
    big = 1 << 30
    for p in ("counts", "imagePairs", "pairs", "offsets", "trackOffsets", "cameraIdx", "featureIdx"):
        yield f"null_{p}", {"null": (p,)}, "null"
    yield "negative_nImages", {"nImages": -1}, "negative nImages or B"
    yield "negative_B", {"B": -1}, "negative nImages or B"
    counts = c.counts.copy()
    counts[2] = -1
    yield "negative_count", {"counts": counts}, "featureCounts[2] = -1"
    off = c.offsets.copy()
    off[0] = 1
    yield "offsets_start", {"offsets": off}, "offsets[0] = 1"
    off = c.offsets.copy()
    off[3] = off[2] - 1
    yield "offsets_decrease", {"offsets": off}, "decrease at problem 2"
    for v in (-1, len(c.counts)):
        ip = c.imagePairs.copy()
        ip[1, 1] = v
        yield f"image_index_{v}", {"imagePairs": ip}, "imagePairs of problem 1"
    for col, v in ((0, -1), (0, 5), (1, -1), (1, 5)):
        pr = c.pairs.copy()
        pr[4, col] = v
        yield f"feature_index_{col}_{v}", {"pairs": pr}, "match 4"
    pr = c.pairs.copy()
    pr[0, 1] = 5
    mask = np.ones(len(pr), np.uint8)
    mask[0] = 0
    yield "feature_index_masked_out", {"pairs": pr, "mask": mask}, "match 0"
    for v in (1, 0, -3):
        yield f"minLength_{v}", {"minLength": v}, "below 2"
    yield "too_many_nodes", {"counts": [big, 1, 5, 5, 5, 5]}, "2^30 features"
    yield "too_many_matches", {"offsets": [0, big + 1], "B": 1}, "2^30 matches"
    yield "negative_maxTracks", {"maxTracks": -1}, "negative maxTracks or maxObs"
    yield "negative_maxObs", {"maxObs": -1}, "negative maxTracks or maxObs"


REFUSALS = {name: (kw, word) for name, kw, word in _refusals()}


@pytest.mark.parametrize("export", BOTH)
@pytest.mark.parametrize("which", list(REFUSALS))
def test_refusals(native, export, which):
    """Every check runs on the host before the device is touched: the same refusal with and without a
    GPU, with a message, and nothing written to any output."""
    kw, word = REFUSALS[which]
    T, _, untouched = R.run(export, R.case("min_length_3"), **kw)
    assert T == -1 and untouched
    assert word in native.last_error() and export in native.last_error()


def test_capacities(native):
    """A result that does not fit is refused whole; the documented capacities are always accepted."""
    for name in ("min_length_2", "zigzag_over_two_images", "random_scene", "one_edge", "B0", "no_images"):
        c, want = R.case(name), R.expected(name)
        mt, mo = R.capacities(c)
        assert mo == min(2 * int(c.offsets[-1]), c.nodes) and mt == mo // 2
        T, got, _ = R.run("mcvHostBuildTracks", c, maxTracks=mt, maxObs=mo)
        assert T == want.T
        # exactly enough is enough
        T, got, _ = R.run("mcvHostBuildTracks", c, maxTracks=want.T, maxObs=len(want.cameraIdx))
        assert T == want.T
        R.assert_same(got, want, name)
        if want.T:
            T, _, untouched = R.run("mcvHostBuildTracks", c, maxTracks=want.T - 1)
            assert T == -1 and untouched and "do not fit maxTracks" in native.last_error()
            T, _, untouched = R.run("mcvHostBuildTracks", c, maxObs=len(want.cameraIdx) - 1)
            assert T == -1 and untouched and "do not fit maxObs" in native.last_error()


def test_export_fails_loudly_without_gpu(native):
    if native.lib().mcvDeviceCount() > 0:
        return   # the valid calls are the GPU suite's subject
    for name in ("one_edge", "B0"):
        T, _, untouched = R.run("cvBuildTracks", R.case(name))
        assert T == -1 and untouched and "no HIP device" in native.last_error()
    c = R.case("one_edge")
    with pytest.raises(N.NativeError, match="no HIP device"):
        CM.buildTracks(c.counts, c.imagePairs, c.pairs, c.offsets)


def test_declarations(native):
    txt = (N.ROOT / "include" / "minicv_native.h").read_text()
    for name in EXPORTS:
        assert name in N.SIGNATURES and getattr(native.lib(), name) is not None
        assert f"MCV_API int {name}(" in txt
    assert "#define MCV_ABI_VERSION 3" in txt and native.lib().mcvAbiVersion() == 3
    assert "maxObs >= min(2 offsets[B], base[nImages])" in txt and "maxTracks >= maxObs / 2" in txt
    ktxt = (N.ROOT / "minicv_amd" / "csrc" / "kernels.h").read_text()
    assert f"kTrkShortMax = {N.TRK_SHORT_MAX};" in ktxt and f"kTrkLaunches = {N.TRK_LAUNCHES};" in ktxt
    assert f"kTrkGrid = {N.TRK_GRID};" in ktxt and f"kTrkScanItems = {N.TRK_SCAN_ITEMS};" in ktxt
    assert f"kTrkScanChunk = {N.TRK_SCAN_CHUNK};" in ktxt
    import minicv_amd
    assert minicv_amd.buildTracks is CM.buildTracks and minicv_amd.trackObservations is CM.trackObservations
    assert native.lib().mcvTestTracksStats(None) == -1


def test_python_wrapper_and_observations(native):
    """camera._build_tracks marshals as the raw call does (here through the twin), and trackObservations
    gathers per-image coordinates by (cameraIdx, featureIdx)."""
    c, want = R.case("random_scene"), R.expected("random_scene")
    toff, cam, feat, tof, dropped = CM._build_tracks("mcvHostBuildTracks", c.counts, c.imagePairs, c.pairs,
                                                     c.offsets, c.mask, c.minLength)
    R.assert_same(R.Result(len(toff) - 1, toff, cam, feat, tof, dropped), want, "wrapper")
    pts = [np.stack([1000.0 * i + np.arange(n), -np.arange(n, dtype=np.float64)], axis=1)
           for i, n in enumerate(c.counts)]
    obs = CM.trackObservations(pts, cam, feat)
    assert obs.shape == (len(cam), 2) and obs.dtype == np.float64
    assert np.array_equal(obs[:, 0], 1000.0 * cam + feat) and np.array_equal(obs[:, 1], -feat.astype(np.float64))
    assert CM.trackObservations(pts, [], []).shape == (0, 2)
    e = CM._build_tracks("mcvHostBuildTracks", [], np.zeros((0, 2), np.int32), np.zeros((0, 2), np.int32), [0])
    assert e[0].tolist() == [0] and e[1].size == 0 and e[3].size == 0 and e[4].tolist() == [0, 0, 0]


def test_host_twin_under_sanitizers(tmp_path):
    """tests/asan/tracks_asan_main.cpp: a stand-alone program (its own main, nothing preloaded, nothing
    loaded into Python) over tracks_ref.h, built with -fsanitize=address,undefined and run over the
    shared cases; its results equal the reference's."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe, inp = tmp_path / "tracks_asan", tmp_path / "cases.txt"
    src = N.ROOT / "tests" / "asan" / "tracks_asan_main.cpp"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{N.ROOT / 'minicv_amd' / 'csrc'}", str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    names = list(R.CASES)
    with open(inp, "w") as f:
        for name in names:
            c = R.case(name)
            nums = [len(c.counts), *c.counts.tolist(), len(c.problems), *c.imagePairs.reshape(-1).tolist(),
                    *c.offsets.tolist(), *c.pairs.reshape(-1).tolist(), int(c.mask is not None),
                    *([] if c.mask is None else c.mask.tolist()), c.minLength]
            f.write(" ".join(map(str, nums)) + "\n")
    r = subprocess.run([str(exe), str(inp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.split("\n")
    assert f"tracks_asan ok: {len(names)} cases" in lines[5 * len(names)] and "ERROR" not in r.stderr
    for k, name in enumerate(names):
        want = R.expected(name)
        head, *arrays = ([int(v) for v in ln.split()] for ln in lines[5 * k:5 * k + 5])
        assert head == [want.T, len(want.cameraIdx), *want.dropped.tolist()], name
        for got, field in zip(arrays, ("trackOffsets", "cameraIdx", "featureIdx", "trackOfFeature")):
            assert got == getattr(want, field).tolist(), (name, field)
