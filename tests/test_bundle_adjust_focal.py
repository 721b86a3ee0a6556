"""Bundle adjustment with focal groups on the host: the declarations, the refusals, and the
twin mcvHostBundleAdjustFocal against an independent numpy restatement of the model: the focal Jacobian
blocks by central differences, one damped step against numpy's dense solve with the focal columns,
convergence from focal lengths 5 % off, the constant groups, a rejected non-positive focal length, and
the twin under sanitizers as a stand-alone program. No GPU."""
import ctypes as C
import re
import shutil
import subprocess
from dataclasses import replace

import numpy as np
import pytest

import _ba_cases as B
import _ba_focal_cases as F
from minicv_amd import native as N

EXPORTS = ["cvBundleAdjustFocal", "mcvHostBundleAdjustFocal", "mcvHostBaFocalStep", "mcvTestBundleAdjustFocalStats"]


def contiguous(c):
    return replace(c, cams=np.ascontiguousarray(c.cams, np.float64), idx=np.ascontiguousarray(c.idx, np.int32),
                   obs=np.ascontiguousarray(c.obs, np.float64), off=np.ascontiguousarray(c.off, np.int32),
                   pts=np.ascontiguousarray(c.pts, np.float64),
                   fixed=None if c.fixed is None else np.ascontiguousarray(c.fixed, np.uint8))


def twin(f, **cfg):
    ret, cams, pts, sm = F.run("mcvHostBundleAdjustFocal", f, f.config(**cfg) if cfg else None)
    assert ret == sm["iterations"] and ret >= 0, N.last_error()
    return cams, pts, sm


def linearize(c):
    """mcvHostBaLinearize: the blocks the focal lengths do not change."""
    n = len(c.idx)
    used, A, Bm, r, w = np.zeros(n, np.uint8), np.zeros((n, 2, 6)), np.zeros((n, 2, 3)), np.zeros((n, 2)), np.zeros(n)
    cfg = c.config()
    k = N.lib().mcvHostBaLinearize(c.cams.ctypes.data, len(c.cams), None if c.fixed is None else c.fixed.ctypes.data,
                                   c.idx.ctypes.data, c.obs.ctypes.data, c.off.ctypes.data, len(c.off) - 1,
                                   c.pts.ctypes.data, C.addressof(cfg), used.ctypes.data, A.ctypes.data, Bm.ctypes.data,
                                   r.ctypes.data, w.ctypes.data)
    assert k == used.sum(), N.last_error()
    return used.astype(bool), A, Bm, r, w


def test_declared_listed_exported(native):
    header = (N.ROOT / "include" / "minicv_native.h").read_text()
    for name in EXPORTS:
        assert re.search(rf"MCV_API int {name}\(", header), name
        assert name in N.SIGNATURES and hasattr(native.lib(), name), name
    assert "mcvBaFocalConfig" in header and "mcvBaFocalSummary" in header
    assert C.sizeof(N.BaFocalConfig) == 48 and C.sizeof(N.BaFocalSummary) == 56
    assert N.BaFocalConfig.base.offset == 0 and N.BaFocalConfig.focalMode.offset == 40
    assert N.BaFocalSummary.base.offset == 0 and N.BaFocalSummary.freeFocalGroups.offset == 48
    d = N.BaFocalConfig.default()
    assert (d.base.maxIterations, d.base.maxCgIterations, d.base.cgTolerance, d.base.initialLambda,
            d.base.functionTolerance, d.base.huberDelta, d.focalMode) == (50, 64, 0.1, 1e-3, 1e-6, 0.0, 1)
    ktxt = (N.ROOT / "minicv_amd" / "csrc" / "kernels.h").read_text()
    L = N.BA_FOCAL_LAUNCHES
    assert f"kBafLaunchesLinearize = {L['linearize']}, kBafLaunchesSystem = {L['system']}" in ktxt
    assert f"kBafLaunchesCgIter = {L['cg_iter']}, kBafLaunchesTrial = {L['trial'] - L['cost']} + kBaLaunchesCost" in ktxt
    assert "kBafLaunchesSetup = kBaLaunchesSetup + 1" in ktxt and L["setup"] == N.BA_LAUNCHES["setup"] + 1


def _refusals():
    c = contiguous(B.scene(40, 3, 5, lengths=[3, 2, 3, 2, 3]))
    g = lambda *v: np.array(v, np.int32)
    neg, zero, other = c.cams.copy(), c.cams.copy(), c.cams.copy()
    neg[1, 12] = -1.5
    zero[2, 13] = 0.0
    other[2, 13] = np.nextafter(other[2, 13], 2.0)
    return {
        "focalMode 3": (F.Focal(c, 3), "focalMode"),
        "focalMode -1": (F.Focal(c, -1), "focalMode"),
        "group high": (F.Focal(c, 1, g(0, 3, 1)), "outside"),
        "group negative": (F.Focal(c, 2, g(0, 1, -1)), "outside"),
        "group high, mode 0": (F.Focal(c, 0, g(0, 3, 1)), "outside"),
        "unequal in a group": (F.Focal(replace(c, cams=other), 1, g(2, 2, 2)), "differs"),
        "unequal in a group, mode 0": (F.Focal(replace(c, cams=other), 0, g(0, 1, 1)), "differs"),
        "negative focal": (F.Focal(replace(c, cams=neg), 1), "positive"),
        "zero focal": (F.Focal(replace(c, cams=zero), 2), "positive"),
        "negative focal beside a fixed group": (F.Focal(replace(c, cams=neg), 2, None, np.array([1, 0, 1], np.uint8)),
                                                "positive"),
    }


@pytest.mark.parametrize("export", ["cvBundleAdjustFocal", "mcvHostBundleAdjustFocal"])
def test_refusals_write_nothing(native, export):
    """The four refusals of the focal arguments run on the host before the device is touched, so the
    export refuses without a GPU too; a non-positive focal length of a group marked fixed is no refusal."""
    for what, (f, msg) in _refusals().items():
        ret, cams, pts, sm = F.run(export, f)
        assert ret == -1 and msg in N.last_error() and export in N.last_error(), (what, ret, N.last_error())
        assert (cams == F.SENTINEL).all() and (pts == F.SENTINEL).all(), what
        assert sm["termination"] == -9 and sm["freeFocalGroups"] == -9, what
    f, _ = _refusals()["negative focal"]
    ok = replace(f, fixedFocal=np.array([0, 1, 0], np.uint8))
    ret, cams, _, sm = F.run("mcvHostBundleAdjustFocal", ok)
    assert ret >= 0 and sm["freeFocalGroups"] == 2 and B.same_bits(cams[1, 12:14], f.case.cams[1, 12:14]), N.last_error()
    # cvBundleAdjust's own refusals still hold
    bad = replace(f.case, cams=B.scene(40, 3, 5, lengths=[3, 2, 3, 2, 3]).cams, cfg=dict(cgTolerance=0.0))
    ret, cams, pts, sm = F.run(export, F.Focal(bad, 1))
    assert ret == -1 and "cgTolerance" in N.last_error() and (cams == F.SENTINEL).all()


@pytest.mark.parametrize("export", ["cvBundleAdjustFocal", "mcvHostBundleAdjustFocal"])
def test_empty_calls_copy_the_inputs(native, export):
    c = contiguous(B.scene(41, 3, 4))
    empty = replace(c, idx=np.zeros(0, np.int32), obs=np.zeros((0, 2)), off=np.zeros(1, np.int32), pts=np.zeros((0, 3)))
    ret, cams, pts, sm = F.run(export, F.Focal(empty, 1))
    assert ret == 0 and B.same_bits(cams, c.cams) and sm["termination"] == 5 and sm["freeFocalGroups"] == 0, N.last_error()


@pytest.mark.parametrize("name", list(B.CASES))
def test_mode_zero_equals_bundle_adjust(native, name):
    """focalMode 0 is mcvHostBundleAdjust bit for bit, summary included, with null groups and with one group."""
    c = B.case(name)
    want = B.run("mcvHostBundleAdjust", c)
    for group in (None, np.zeros(len(c.cams), np.int32)):
        got = F.run("mcvHostBundleAdjustFocal", F.Focal(c, 0, group))
        assert got[0] == want[0] and B.same_bits(got[1], want[1]) and B.same_bits(got[2], want[2]), name
        assert got[3] == dict(want[3], freeFocalGroups=0), name


@pytest.mark.parametrize("mode", [1, 2])
def test_focal_blocks_against_central_differences(native, mode):
    """The focal block of every observation against central differences (h = 1e-6) of the numpy model in
    the group's parameters (s at 0 for mode 1, (dfx, dfy) for mode 2): within 1e-7 of the block's
    largest entry, test_bundle_adjust.py's step and bound for A and B (the residual is linear in both
    parameterisations, so only eps / h remains)."""
    c = contiguous(B.scene(50, 4, 12, nFixed=1, dCam=(0.05, 0.1), dPts=0.1))
    f = F.Focal(c, mode, np.array([0, 0, 2, 2], np.int32), np.array([0, 0, 0, 1], np.uint8))
    it, u, _, _, _ = F.step(f, 1e-3)
    assert it > 0, N.last_error()
    trk = np.repeat(np.arange(len(c.off) - 1), np.diff(c.off))
    h = 1e-6
    for k in range(len(c.idx)):
        j, i = c.idx[k], trk[k]

        def res(params):
            cam = F.with_focal(c.cams[j:j + 1], np.asarray(params, float).reshape(1, 2), mode)[0]
            pcv = B.rot(cam) @ (c.pts[i] - cam[0:3])
            return cam[12:14] * pcv[:2] / pcv[2] - c.obs[k]
        if j >= 2:
            assert (u[k] == 0).all()      # cameras 2 and 3 share a group that camera 3 marks fixed
            continue
        num = np.empty((2, 2))
        for a in range(2):
            d = np.zeros(2)
            d[a] = h
            num[:, a] = (res(d) - res(-d)) / (2 * h)
        if mode == 1:                      # the column of s; the second parameter does not exist
            assert np.abs(u[k] - num[:, 0]).max() <= 1e-7 * np.abs(num[:, 0]).max(), k
        else:
            assert np.abs(np.diag(u[k]) - num).max() <= 1e-7 * np.abs(num).max(), k


@pytest.mark.parametrize("mode,shared", [(1, True), (1, False), (2, True), (2, False)])
def test_one_step_against_numpy(native, mode, shared):
    """test_bundle_adjust.py's 4-camera scene (1 pose-fixed, 40 points, noise 1e-3) with every focal length
    5 % off: the dense J from the hooks' blocks with the focal columns of every group (1 or 4 groups, 1 or 2
    columns each) between the cameras' and the points', numpy's solve of the damped normal equations at
    lambda = 1e-3 (condition number asserted <= 1e8, the existing test's cap), and the twin's step with
    cgTolerance 1e-14: 1e-6 relative in the 2-norm, the existing test's bound.
    Measured: condition numbers 4.4e5 (one group, either mode), 4.6e5 (mode 1, null), 4.8e5 (mode 2, null);
    relative differences 1.1e-13, 2.2e-13, 3.4e-13 after 20 / 21, 34 and 44 CG iterations."""
    c = contiguous(F.off_focal(B.scene(51, 4, 40, nFixed=1, noise=1e-3, cgTolerance=1e-14, maxCgIterations=200)))
    nC, T, n, lam = len(c.cams), len(c.off) - 1, len(c.idx), 1e-3
    group = np.zeros(nC, np.int32) if shared else np.arange(nC, dtype=np.int32)
    f = F.Focal(c, mode, group if shared else None)
    used, A, Bm, r, _ = linearize(c)
    it, u, dC, dF, dP = F.step(f, lam)
    assert used.all() and 0 < it <= 200, N.last_error()
    free = [j for j in range(nC) if not c.fixed[j]]
    col = {j: 6 * m for m, j in enumerate(free)}
    nG, fd = int(group.max()) + 1, mode
    o1 = 6 * len(free)
    o2 = o1 + fd * nG
    trk = np.repeat(np.arange(T), np.diff(c.off))
    J = np.zeros((2 * n, o2 + 3 * T))
    for k in range(n):
        j = c.idx[k]
        if j in col:
            J[2 * k:2 * k + 2, col[j]:col[j] + 6] = A[k]
        if mode == 1:
            J[2 * k:2 * k + 2, o1 + group[j]] = u[k]
        else:
            J[2 * k, o1 + 2 * group[j]], J[2 * k + 1, o1 + 2 * group[j] + 1] = u[k]
        J[2 * k:2 * k + 2, o2 + 3 * trk[k]:o2 + 3 * trk[k] + 3] = Bm[k]
    H = J.T @ J
    d = np.diag(H).copy()
    H[np.diag_indices_from(H)] = d + lam * np.clip(d, 1e-6, 1e32)
    cond = np.linalg.cond(H)
    print("condition number", cond)
    assert cond <= 1e8
    want = np.linalg.solve(H, -J.T @ r.reshape(-1))
    for g in range(nG):       # every camera of a group reports the group's step
        assert len(np.unique(B.bits(dF[group == g]), axis=0)) == 1
    if mode == 1:
        assert (dF[:, 1] == 0).all()
    gf = np.concatenate([dF[np.nonzero(group == g)[0][0], :fd] for g in range(nG)])
    got = np.concatenate([dC[free].reshape(-1), gf, dP.reshape(-1)])
    rel = np.linalg.norm(got - want) / np.linalg.norm(want)
    print("relative difference of the step", rel, "after", it, "CG iterations")
    assert rel <= 1e-6


def test_convergence_from_wrong_focal(native):
    """The noise-free ring of test_convergence_noise_free with every focal length 5 % off, two cameras
    pose-fixed: with one group for all cameras and with null groups, in both modes, the cost falls to
    rounding level and focal lengths, cameras and points return to the truth, within the existing test's
    bounds (final cost <= 1e-16 x initial, 1e-6 on the parameters). Measured: final costs 1.2e-30 to
    1.4e-30 from 0.136; focal lengths within 1.8e-15, cameras 8.9e-15, points 1.1e-15.
    mcvHostBundleAdjust on the same scene cannot absorb the focal error: it ends at 1.2e-4, 8.5e25 times
    the worst focal run; asserted with a decade of margin (8.5e24)."""
    c = F.convergence_scene()
    nC = len(c.cams)
    used = B.used_set(c.cams, c.pts, c.idx, c.obs, c.off)
    c0 = B.cost(c.cams, c.pts, c.idx, c.obs, c.off, used)
    _, _, _, plain = B.run("mcvHostBundleAdjust", c)
    worst = 0.0
    for mode in (1, 2):
        for group in (np.zeros(nC, np.int32), None):
            cams, pts, sm = twin(F.Focal(c, mode, group))
            print(mode, "one group" if group is not None else "null groups", sm,
                  np.abs(cams[:, 12:14] - c.truth[0][:, 12:14]).max(), np.abs(cams - c.truth[0]).max(),
                  np.abs(pts - c.truth[1]).max())
            assert sm["usedObservations"] == used.sum() == len(c.idx) and abs(sm["initialCost"] - c0) <= 1e-12 * c0
            assert sm["freeFocalGroups"] == (1 if group is not None else nC)
            assert sm["finalCost"] <= 1e-16 * sm["initialCost"]
            assert B.cost(cams, pts, c.idx, c.obs, c.off, used) <= 1e-16 * c0    # numpy's own evaluation of the outputs
            assert np.abs(cams - c.truth[0]).max() <= 1e-6 and np.abs(pts - c.truth[1]).max() <= 1e-6
            assert B.same_bits(cams[:2, :12], c.cams[:2, :12])                   # pose-fixed, focal refined
            assert sm["iterations"] == sm["accepted"] + sm["rejected"] <= 50 and sm["termination"] in (2, 3, 4)
            worst = max(worst, sm["finalCost"])
    print("mcvHostBundleAdjust", plain["finalCost"], "ratio", plain["finalCost"] / worst)
    assert plain["finalCost"] >= 8.5e24 * worst


def test_constant_groups(native):
    """A group marked fixed, a group without a used observation and focalMode 0 hand back their focal bits;
    a free group whose cameras are all pose-fixed still moves."""
    c = F.off_focal(B.scene(1, 6, 40, noise=1e-3, maxIterations=6), 1.03)     # cameras 0 and 1 pose-fixed
    group = np.array([0, 0, 2, 2, 4, 4], np.int32)
    for mode in (1, 2):
        cams, _, sm = twin(F.Focal(c, mode, group, np.array([0, 0, 0, 1, 0, 0], np.uint8)))
        moved = ~(B.bits(cams[:, 12:14]) == B.bits(c.cams[:, 12:14])).all(axis=1)
        assert moved.tolist() == [True, True, False, False, True, True] and sm["freeFocalGroups"] == 2
        assert B.same_bits(cams[:2, :12], c.cams[:2, :12]) and B.same_bits(cams[0, 12:14], cams[1, 12:14])
        assert not B.same_bits(cams[2:, :12], c.cams[2:, :12])      # their poses move all the same
    cams, _, sm = twin(F.Focal(c, 0, group))
    assert B.same_bits(cams[:, 12:14], c.cams[:, 12:14]) and sm["freeFocalGroups"] == 0
    e = F.off_focal(B.case("segment_edges"), 1.03)        # camera 5 has no observation
    assert np.bincount(e.idx, minlength=6)[5] == 0
    for mode in (1, 2):
        cams, _, sm = twin(F.Focal(e, mode, np.array([0, 0, 0, 0, 0, 5], np.int32)))
        moved = ~(B.bits(cams[:, 12:14]) == B.bits(e.cams[:, 12:14])).all(axis=1)
        assert moved.tolist() == [True] * 5 + [False] and sm["freeFocalGroups"] == 1


@pytest.mark.parametrize("mode", [1, 2])
def test_non_positive_focal_trial_is_rejected(native, mode):
    """Mirrored observations (obs -> -obs) with every pose fixed: the best focal length is the negative of
    the true one, and the first step at lambda = 1e-6 goes there. That trial lowers the cost (numpy's own
    evaluation) with every point still in front of its camera, so only the focal rule rejects it; the run
    goes on with larger lambda and ends with positive focal lengths and a lower cost."""
    c = B.scene(70, 4, 30, nFixed=4, dPts=0.0)
    c = contiguous(replace(c, obs=-c.obs, cfg=dict(initialLambda=1e-6, maxIterations=40)))
    f = F.Focal(c, mode, np.zeros(4, np.int32))
    it, _, dC, dF, dP = F.step(f, 1e-6)
    assert it > 0 and (dC == 0).all(), N.last_error()
    trial = F.with_focal(c.cams, dF, mode)
    assert (trial[:, 12:14] < 0).all()
    used = B.used_set(c.cams, c.pts, c.idx, c.obs, c.off)
    r, pc = B.residuals(trial, c.pts + dP, c.idx, c.obs, c.off)
    before = B.cost(c.cams, c.pts, c.idx, c.obs, c.off, used)
    assert used.all() and (pc[:, 2] > 0).all() and float((r * r).sum()) < before
    _, _, first = twin(f, maxIterations=1)
    assert first["rejected"] == 1 and first["accepted"] == 0 and first["finalCost"] == first["initialCost"]
    cams, pts, sm = twin(f)
    print(sm, cams[0, 12:14])
    assert sm["rejected"] > 0 and sm["accepted"] > 0 and sm["finalCost"] < sm["initialCost"]
    assert (cams[:, 12:14] > 0).all() and np.isfinite(cams).all()


def _hex(a):
    return " ".join(float(v).hex() for v in np.asarray(a, np.float64).reshape(-1))


def test_host_twin_under_sanitizers(tmp_path):
    """tests/asan/bundle_adjust_focal_asan_main.cpp: a stand-alone program (its own main, nothing preloaded,
    nothing loaded into Python) over ba_ref.h, built with -fsanitize=address,undefined and run over
    shared cases; its results equal the library's twin bit for bit."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe, inp = tmp_path / "bundle_adjust_focal_asan", tmp_path / "cases.txt"
    src = N.ROOT / "tests" / "asan" / "bundle_adjust_focal_asan_main.cpp"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", f"-I{N.ROOT / 'minicv_amd' / 'csrc'}", str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    names = ["T65_m1_null", "track_lengths_m1_two", "track_lengths_m2_null", "segments_m1_shared_empty",
             "segments_m2_fixed_group", "cameras_257_m2_pair", "cameras_258_m1_null", "huber_on_m1", "rejected_m2",
             "term_lambda", "term_nothing", "term_zero_cost"]
    with open(inp, "w") as out:
        for name in names:
            f = F.focal_case(name)
            c, cfg = f.case, f.config()
            out.write(f"{len(c.cams)} {len(c.off) - 1} {len(c.idx)} {0 if c.fixed is None else 1} "
                      f"{0 if f.group is None else 1} {0 if f.fixedFocal is None else 1} {f.mode}\n")
            out.write(f"{cfg.base.maxIterations} {cfg.base.maxCgIterations} " +
                      _hex([cfg.base.cgTolerance, cfg.base.initialLambda, cfg.base.functionTolerance,
                            cfg.base.huberDelta]) + "\n")
            out.write(_hex(c.cams) + "\n")
            for a in (c.fixed, f.group, f.fixedFocal):
                if a is not None:
                    out.write(" ".join(str(int(v)) for v in a) + "\n")
            out.write(" ".join(str(int(v)) for v in c.idx) + "\n" + _hex(c.obs) + "\n")
            out.write(" ".join(str(int(v)) for v in c.off) + "\n" + _hex(c.pts) + "\n")
    r = subprocess.run([str(exe), str(inp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.split("\n")
    assert f"bundle_adjust_focal_asan ok: {len(names)} cases" in lines[4 * len(names)] and "ERROR" not in r.stderr
    for k, name in enumerate(names):
        f = F.focal_case(name)
        _, cams, pts, sm = F.twin_of(name)
        head = [int(v) for v in lines[4 * k].split()]
        assert head[:8] == [sm[q] for q in ("iterations", "accepted", "rejected", "cgIterations", "usedObservations",
                                            "usedTracks", "termination", "freeFocalGroups")], name
        assert head[8] == (len(f.case.cams) if f.group is None else len(np.unique(f.group))), name
        words = [np.array([int(v, 16) for v in lines[4 * k + m].split()], np.uint64) for m in (1, 2, 3)]
        assert np.array_equal(words[0], B.bits([sm["initialCost"], sm["finalCost"]])), name
        assert np.array_equal(words[1], B.bits(cams).reshape(-1)) and np.array_equal(words[2], B.bits(pts).reshape(-1)), name
