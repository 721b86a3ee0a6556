"""Bundle adjustment on the host: the declarations, the refusals, and the twin
mcvHostBundleAdjust against an independent numpy restatement of the model (tests/_ba_cases.py):
Jacobians by central differences, one damped step against numpy's dense solve, convergence on a
noise-free scene, the Huber loss, the exclusions, a case with rejected steps, and the twin under
sanitizers as a stand-alone program. No GPU."""
import ctypes as C
import re
import shutil
import subprocess
from dataclasses import replace

import numpy as np
import pytest

import _ba_cases as B
from minicv_amd import native as N

EXPORTS = ["cvBundleAdjust", "mcvHostBundleAdjust", "mcvHostBaLinearize", "mcvHostBaStep", "mcvTestBundleAdjustStats"]


def twin(c, **cfg):
    ret, cams, pts, sm = B.run("mcvHostBundleAdjust", replace(c, cfg=dict(c.cfg, **cfg)) if cfg else c)
    assert ret == sm["iterations"] and ret >= 0, N.last_error()
    return cams, pts, sm


def linearize(c):
    n = len(c.idx)
    used, A, Bm, r, w = np.zeros(n, np.uint8), np.zeros((n, 2, 6)), np.zeros((n, 2, 3)), np.zeros((n, 2)), np.zeros(n)
    cfg = c.config()
    k = N.lib().mcvHostBaLinearize(c.cams.ctypes.data, len(c.cams), None if c.fixed is None else c.fixed.ctypes.data,
                                   c.idx.ctypes.data, c.obs.ctypes.data, c.off.ctypes.data, len(c.off) - 1,
                                   c.pts.ctypes.data, C.addressof(cfg), used.ctypes.data, A.ctypes.data, Bm.ctypes.data,
                                   r.ctypes.data, w.ctypes.data)
    assert k == used.sum(), N.last_error()
    return used.astype(bool), A, Bm, r, w


def contiguous(c):
    return replace(c, cams=np.ascontiguousarray(c.cams, np.float64), idx=np.ascontiguousarray(c.idx, np.int32),
                   obs=np.ascontiguousarray(c.obs, np.float64), off=np.ascontiguousarray(c.off, np.int32),
                   pts=np.ascontiguousarray(c.pts, np.float64),
                   fixed=None if c.fixed is None else np.ascontiguousarray(c.fixed, np.uint8))


def test_declared_listed_exported(native):
    header = (N.ROOT / "include" / "minicv_native.h").read_text()
    for name in EXPORTS:
        assert re.search(rf"MCV_API int {name}\(", header), name
        assert name in N.SIGNATURES and hasattr(native.lib(), name), name
    assert "mcvBaConfig" in header and "mcvBaSummary" in header
    assert C.sizeof(N.BaConfig) == 40 and C.sizeof(N.BaSummary) == 48
    d = N.BaConfig.default()
    assert (d.maxIterations, d.maxCgIterations, d.cgTolerance, d.initialLambda, d.functionTolerance, d.huberDelta) == \
        (50, 64, 0.1, 1e-3, 1e-6, 0.0)


def _refusals():
    c = contiguous(B.scene(40, 3, 5, lengths=[3, 2, 3, 2, 3]))
    big = np.concatenate([[0], np.full(5, N.MAX_TRACK_LEN + 1)]).astype(np.int32)
    cams_nan = c.cams.copy()
    cams_nan[1, 4] = np.inf
    bad_idx = c.idx.copy()
    bad_idx[4] = 3
    neg_idx = c.idx.copy()
    neg_idx[0] = -1
    off1, offd = c.off.copy(), c.off.copy()
    off1[0] = 1
    offd[2] = offd[1] - 1
    return {
        "offsets[0]": (replace(c, off=off1), "not 0"),
        "offsets decrease": (replace(c, off=offd), "decrease"),
        "track over the cap": (replace(c, off=big), "MCV_MAX_TRACK_LEN"),
        # 16 385 tracks of 4096: over 2^26 observations; refused from the offsets alone, nothing else is read
        "too many observations": (replace(c, off=(np.arange(16386, dtype=np.int64) * N.MAX_TRACK_LEN).astype(np.int32)),
                                  "over 2^26"),
        "camera index high": (replace(c, idx=bad_idx), "outside"),
        "camera index negative": (replace(c, idx=neg_idx), "outside"),
        "non-finite camera": (replace(c, cams=cams_nan), "non-finite"),
        "cgTolerance": (replace(c, cfg=dict(cgTolerance=0.0)), "cgTolerance"),
        "cgTolerance nan": (replace(c, cfg=dict(cgTolerance=float("nan"))), "cgTolerance"),
        "initialLambda": (replace(c, cfg=dict(initialLambda=-1.0)), "initialLambda"),
        "initialLambda inf": (replace(c, cfg=dict(initialLambda=float("inf"))), "initialLambda"),
        "functionTolerance": (replace(c, cfg=dict(functionTolerance=-1e-3)), "functionTolerance"),
        "maxIterations": (replace(c, cfg=dict(maxIterations=-1)), "maxIterations"),
        "maxCgIterations": (replace(c, cfg=dict(maxCgIterations=-2)), "maxCgIterations"),
        "huberDelta nan": (replace(c, cfg=dict(huberDelta=float("nan"))), "huberDelta"),
    }


@pytest.mark.parametrize("export", ["cvBundleAdjust", "mcvHostBundleAdjust"])
def test_refusals_write_nothing(native, export):
    """Every check runs on the host before the device is touched, so the export refuses without a GPU too."""
    for what, (c, msg) in _refusals().items():
        ret, cams, pts, sm = B.run(export, c)
        assert ret == -1 and msg in N.last_error(), (what, ret, N.last_error())
        assert (cams == B.SENTINEL).all() and (pts == B.SENTINEL).all() and sm["termination"] == -9, what
    c = contiguous(B.scene(40, 3, 5))
    L, cfg, sm = native.lib(), c.config(), N.BaSummary()
    outC, outP = np.full_like(c.cams, B.SENTINEL), np.full_like(c.pts, B.SENTINEL)
    args = [c.cams.ctypes.data, 3, None, c.idx.ctypes.data, c.obs.ctypes.data, c.off.ctypes.data, 5, c.pts.ctypes.data,
            C.addressof(cfg), outC.ctypes.data, outP.ctypes.data, C.addressof(sm)]
    for null in (0, 3, 4, 5, 7, 9, 10):   # cameras, cameraIdx, observations, offsets, points, outCameras, outPoints
        a = list(args)
        a[null] = None
        assert getattr(L, export)(*a) == -1 and "null" in N.last_error(), null
    for pos, val in ((1, -1), (6, -1)):   # nCameras, T
        a = list(args)
        a[pos] = val
        assert getattr(L, export)(*a) == -1 and "negative" in N.last_error(), pos
    assert (outC == B.SENTINEL).all() and (outP == B.SENTINEL).all()
    if export == "cvBundleAdjust" and L.mcvDeviceCount() <= 0:
        assert getattr(L, export)(*args) == -1 and (outC == B.SENTINEL).all() and (outP == B.SENTINEL).all()


@pytest.mark.parametrize("export", ["cvBundleAdjust", "mcvHostBundleAdjust"])
def test_empty_calls_copy_the_inputs(native, export):
    c = contiguous(B.scene(41, 3, 4))
    empty = replace(c, idx=np.zeros(0, np.int32), obs=np.zeros((0, 2)), off=np.zeros(1, np.int32), pts=np.zeros((0, 3)))
    ret, cams, pts, sm = B.run(export, empty)
    assert ret == 0 and B.same_bits(cams, c.cams) and sm["termination"] == 5 and sm["usedTracks"] == 0, N.last_error()
    notracks = replace(c, idx=np.zeros(0, np.int32), obs=np.zeros((0, 2)), off=np.zeros(5, np.int32))
    ret, cams, pts, sm = B.run(export, notracks)   # four tracks without an observation
    assert ret == 0 and B.same_bits(cams, c.cams) and B.same_bits(pts, c.pts) and sm["termination"] == 5


def test_nothing_used_copies_the_inputs(native):
    c = B.case("term_nothing")
    cams, pts, sm = twin(c)
    assert sm["iterations"] == 0 and sm["termination"] == 5 and sm["usedObservations"] == 0
    assert B.same_bits(cams, c.cams) and B.same_bits(pts, c.pts)


def test_jacobians_against_central_differences(native):
    """A_k and B_k against central differences (h = 1e-6) of the numpy model through the Cayley
    retraction: within 1e-7 of each block's largest entry (depths >= 1 and |focal| <= 2 keep the h^2
    and eps / h terms near 1e-10)."""
    c = contiguous(B.scene(50, 4, 12, nFixed=1, dCam=(0.05, 0.1), dPts=0.1))
    used, A, Bm, r, w = linearize(c)
    _, pc = B.residuals(c.cams, c.pts, c.idx, c.obs, c.off)
    assert used.all() and pc[:, 2].min() >= 1.0 and np.abs(c.cams[:, 12:14]).max() <= 2.0 and (w == 1.0).all()
    r0, _ = B.residuals(c.cams, c.pts, c.idx, c.obs, c.off)
    assert np.abs(r - r0).max() <= 1e-14
    trk = np.repeat(np.arange(len(c.off) - 1), np.diff(c.off))
    h = 1e-6
    for k in range(len(c.idx)):
        j, i = c.idx[k], trk[k]

        def res(cam, X):
            pcv = B.rot(cam) @ (X - cam[0:3])
            return cam[12:14] * pcv[:2] / pcv[2] - c.obs[k]
        numA, numB = np.empty((2, 6)), np.empty((2, 3))
        for a in range(6):
            d = np.zeros(6)
            d[a] = h
            numA[:, a] = (res(B.retract(c.cams[j], d), c.pts[i]) - res(B.retract(c.cams[j], -d), c.pts[i])) / (2 * h)
        for a in range(3):
            d = np.zeros(3)
            d[a] = h
            numB[:, a] = (res(c.cams[j], c.pts[i] + d) - res(c.cams[j], c.pts[i] - d)) / (2 * h)
        if c.fixed[j]:
            assert (A[k] == 0).all()          # a fixed camera's block is zero
        else:
            assert np.abs(A[k] - numA).max() <= 1e-7 * np.abs(numA).max(), k
        assert np.abs(Bm[k] - numB).max() <= 1e-7 * np.abs(numB).max(), k


def _one_step_scenes():
    return {"4_cameras": (lambda: B.scene(51, 4, 40, nFixed=1, noise=1e-3, cgTolerance=1e-14, maxCgIterations=60), 60),
            "257_cameras": (lambda: B.camera_ring(257, seed=52, perCam=6, cgTolerance=1e-14, maxCgIterations=400), 400)}


def test_one_step_against_numpy(native):
    _one_step("4_cameras")


def test_one_step_against_numpy_257_cameras(native):
    _one_step("257_cameras")


def _one_step(which):
    """4 cameras (1 fixed), 40 points, and 257 cameras (3 fixed, one without an observation: not a
    column of J; camera 256 free and observed), about 300 points, where the twin's chains over the cameras (r.z, p.q, the cost) take a
    second trip of 256: the dense J from the hook's blocks, numpy's solve of the damped normal equations
    at lambda = 1e-3 (condition number asserted <= 1e8), and the twin's step with cgTolerance 1e-14 and
    60 (400) CG iterations: 1e-6 relative in the 2-norm (cond x eps with a hundredfold margin)."""
    make, maxCg = _one_step_scenes()[which]
    c = contiguous(make())
    lam = 1e-3
    used, A, Bm, r, _ = linearize(c)
    assert used.all()
    nC, T, n = len(c.cams), len(c.off) - 1, len(c.idx)
    seen = np.bincount(c.idx, minlength=nC) > 0
    free = [j for j in range(nC) if not c.fixed[j] and seen[j]]
    if which == "257_cameras":
        assert nC == 257 > 256 and 250 <= T <= 350 and len(free) == nC - 4 and not seen[254] and c.fixed[255]
        assert 256 in free   # the second trip of the chains holds a free, observed camera: its terms are not zero
        assert np.bincount(c.idx, minlength=nC)[seen].min() >= 6
    col = {j: 6 * m for m, j in enumerate(free)}
    trk = np.repeat(np.arange(T), np.diff(c.off))
    J = np.zeros((2 * n, 6 * len(free) + 3 * T))
    for k in range(n):
        if c.idx[k] in col:
            J[2 * k:2 * k + 2, col[c.idx[k]]:col[c.idx[k]] + 6] = A[k]
        J[2 * k:2 * k + 2, 6 * len(free) + 3 * trk[k]:6 * len(free) + 3 * trk[k] + 3] = Bm[k]
    H = J.T @ J
    d = np.diag(H).copy()
    H[np.diag_indices_from(H)] = d + lam * np.clip(d, 1e-6, 1e32)
    cond = np.linalg.cond(H)
    print("condition number", cond)
    assert cond <= 1e8
    want = np.linalg.solve(H, -J.T @ r.reshape(-1))
    dC, dP, cfg = np.zeros((nC, 6)), np.zeros((T, 3)), c.config()
    it = N.lib().mcvHostBaStep(c.cams.ctypes.data, nC, c.fixed.ctypes.data, c.idx.ctypes.data, c.obs.ctypes.data,
                               c.off.ctypes.data, T, c.pts.ctypes.data, C.addressof(cfg), lam, dC.ctypes.data,
                               dP.ctypes.data)
    assert 0 < it <= maxCg, N.last_error()
    rest = np.setdiff1d(np.arange(nC), free)
    assert (dC[rest] == 0).all()          # fixed cameras and the one nothing sees
    got = np.concatenate([dC[free].reshape(-1), dP.reshape(-1)])
    rel = np.linalg.norm(got - want) / np.linalg.norm(want)
    print("relative difference of the step", rel, "after", it, "CG iterations")
    assert rel <= 1e-6


def test_constants_pinned():
    """The mirrors of the sizes the scale cases are derived from, read from the headers' text."""
    ktxt = (N.ROOT / "minicv_amd" / "csrc" / "kernels.h").read_text()
    ttxt = (N.ROOT / "minicv_amd" / "csrc" / "ba_terms.h").read_text()
    assert f"kBaGrid = {N.BA_GRID};" in ktxt and f"kBaLongBlocks = {N.BA_LONG_BLOCKS};" in ktxt
    assert f"kBaSeg = {N.BA_SEG};" in ttxt and f"kBaShortMax = {N.BA_SHORT_MAX};" in ttxt
    assert f"kBaCgChunk = {N.BA_CG_CHUNK};" in ttxt


def test_vectorised_model_equals_loop_model():
    """residuals_v against residuals on existing cases: not 0 ulp. pc's three products are summed left
    to right there and by numpy's matrix product in the loop form, so pc differs by at most 2 ulp of its
    largest entry and a residual of a used observation (below 1) by at most 2^-52; the used sets are equal."""
    for name in ("track_lengths", "segment_edges", "huber_on", "exclusions"):
        c = B.case(name)
        r, pc = B.residuals(c.cams, c.pts, c.idx, c.obs, c.off)
        rv, pcv = B.residuals_v(c.cams, c.pts, c.idx, c.obs, c.off)
        used = ok = B.used_set(c.cams, c.pts, c.idx, c.obs, c.off)
        assert np.array_equal(used, B.used_set_v(c.cams, c.pts, c.idx, c.obs, c.off)) and ok.sum() >= len(ok) - 8
        assert np.abs(pc[ok] - pcv[ok]).max() <= 2 * np.spacing(np.abs(pc[ok]).max())
        assert np.abs(r[ok]).max() < 1 and np.abs(r[ok] - rv[ok]).max() <= 2.0 ** -52
        a, b = B.cost(c.cams, c.pts, c.idx, c.obs, c.off, used, 0.01), B.cost_v(c.cams, c.pts, c.idx, c.obs, c.off, used, 0.01)
        assert abs(a - b) <= 1e-13 * a


@pytest.mark.parametrize("nCam", [255, 256, 257, 513])
def test_camera_rings(native, nCam):
    """The cases with more cameras than one trip of 256: every camera has at least 3 observations but
    the one with none; the twin's costs against numpy's own evaluation (test_end_to_end's 1e-12)."""
    c = B.case(f"cameras_{nCam}")
    empty, alsoFixed = B.camera_ring_special(nCam)
    per = np.bincount(c.idx, minlength=nCam)
    assert len(c.cams) == nCam and per[empty] == 0 and per[np.arange(nCam) != empty].min() >= 3
    assert np.nonzero(c.fixed)[0].tolist() == [0, 1, alsoFixed] and per[alsoFixed] >= 3
    if nCam > 257:
        assert empty >= 256 and alsoFixed >= 256
    if nCam > 256:   # the last camera, alone in its trip of the chains over the cameras, is free and observed
        assert nCam % 256 == 1 and not c.fixed[nCam - 1] and per[nCam - 1] >= 3
    L = np.diff(c.off)
    assert 350 <= len(L) <= 450 and L.min() >= 4 and L.max() <= 9 and c.cfg["maxIterations"] == 3
    cams, pts, sm = twin(c)
    used = B.used_set_v(c.cams, c.pts, c.idx, c.obs, c.off)
    assert used.all() and sm["usedObservations"] == len(c.idx) and sm["usedTracks"] == len(L)
    c0, c1 = B.cost_v(c.cams, c.pts, c.idx, c.obs, c.off, used), B.cost_v(cams, pts, c.idx, c.obs, c.off, used)
    assert abs(sm["initialCost"] - c0) <= 1e-12 * c0 and abs(sm["finalCost"] - c1) <= 1e-12 * c1
    assert sm["accepted"] > 0 and sm["finalCost"] < 0.1 * sm["initialCost"] and sm["cgIterations"] > 0
    keep = [0, 1, alsoFixed, empty]
    assert B.same_bits(cams[keep], c.cams[keep])
    moved = np.setdiff1d(np.arange(nCam), keep)
    assert (B.bits(cams[moved]) != B.bits(c.cams[moved])).any(axis=1).all()


def scale_segments(c):
    return int(np.sum(-(-np.bincount(c.idx, minlength=len(c.cams)) // N.BA_SEG)))


def test_scale_case(native):
    """What makes `scale` a second-trip case, from the mirrored constants, and the twin on it against
    the vectorised numpy model."""
    c = B.case("scale")
    n, T, L = len(c.idx), len(c.off) - 1, np.diff(c.off)
    nLong = int((L > N.BA_SHORT_MAX).sum())
    assert n > N.BA_GRID * 256 and nLong > 4 * N.BA_LONG_BLOCKS and T >= 1024
    assert set(L.tolist()) == {3, N.BA_SHORT_MAX + 1} and len(c.cams) == 70
    per = np.bincount(c.idx, minlength=70)
    assert per.min() > 3 * N.BA_SEG and scale_segments(c) > 3 * 70
    trk = np.repeat(np.arange(T), L)
    assert len(np.unique(trk.astype(np.int64) * 70 + c.idx)) == n      # distinct cameras within a track
    cams, pts, sm = twin(c)
    used = B.used_set_v(c.cams, c.pts, c.idx, c.obs, c.off)
    assert used.all() and sm["usedTracks"] == T and sm["usedObservations"] == n
    delta = c.cfg["huberDelta"]
    r, _ = B.residuals_v(c.cams, c.pts, c.idx, c.obs, c.off)
    assert 0.2 < (np.sqrt((r * r).sum(axis=1)) > delta).mean() < 1.0   # both branches of the loss are taken
    c0, c1 = B.cost_v(c.cams, c.pts, c.idx, c.obs, c.off, used, delta), B.cost_v(cams, pts, c.idx, c.obs, c.off, used, delta)
    print("scale: twin against numpy, relative", abs(sm["initialCost"] - c0) / c0, abs(sm["finalCost"] - c1) / c1)
    assert abs(sm["initialCost"] - c0) <= 1e-12 * c0 and abs(sm["finalCost"] - c1) <= 1e-12 * c1
    assert sm["finalCost"] < sm["initialCost"] and sm["iterations"] == 2


def test_convergence_noise_free(native):
    c = B.case("converge")
    cams, pts, sm = twin(c)
    used = B.used_set(c.cams, c.pts, c.idx, c.obs, c.off)
    assert sm["usedObservations"] == used.sum() == len(c.idx) and sm["usedTracks"] == len(c.off) - 1
    c0 = B.cost(c.cams, c.pts, c.idx, c.obs, c.off, used)
    assert abs(sm["initialCost"] - c0) <= 1e-12 * c0
    print("initial", sm["initialCost"], "final", sm["finalCost"], sm)
    assert sm["finalCost"] <= 1e-16 * sm["initialCost"]
    assert B.cost(cams, pts, c.idx, c.obs, c.off, used) <= 1e-16 * c0     # numpy's own evaluation of the outputs
    assert np.abs(cams - c.truth[0]).max() <= 1e-6 and np.abs(pts - c.truth[1]).max() <= 1e-6
    assert sm["iterations"] == sm["accepted"] + sm["rejected"] <= 50 and sm["termination"] in (2, 3, 4)
    assert B.same_bits(cams[:2], c.cams[:2])                               # the two fixed cameras
    # the cost never rises over the accepted steps: the run cut after k trials is a prefix of the full run.
    # numpy's cost of the same outputs differs by the rounding of the residuals: each of the 2 n components
    # carries at most eps = 8 x 2^-52 (a handful of roundings of values below 1), so
    # |d cost| <= sum 2 |r| eps + eps^2 <= 2 eps sqrt(2 n cost) + 2 n eps^2
    costs, acc, eps, n2 = [sm["initialCost"]], 0, 8 * 2.0 ** -52, 2 * len(c.idx)
    for k in range(1, 14):
        ck, pk, sk = twin(c, maxIterations=k)
        assert sk["iterations"] == k and sk["accepted"] >= acc
        assert sk["finalCost"] < costs[-1] if sk["accepted"] > acc else sk["finalCost"] == costs[-1]
        mid = B.cost(ck, pk, c.idx, c.obs, c.off, used)
        assert abs(mid - sk["finalCost"]) <= 2 * eps * np.sqrt(n2 * sk["finalCost"]) + n2 * eps * eps
        costs.append(sk["finalCost"])
        acc = sk["accepted"]


def test_huber(native):
    on, off = B.case("huber_on"), B.case("huber_off")
    _, bad = B._with_outliers(B.scene(2, 6, 60, noise=1e-3, dCam=(0.005, 0.01), dPts=0.02), 3)
    assert 0.05 < bad.mean() < 0.2 and B.same_bits(on.obs, off.obs)
    delta = on.cfg["huberDelta"]
    used = B.used_set(on.cams, on.pts, on.idx, on.obs, on.off)
    err = {}
    for name, c, d in (("on", on, delta), ("off", off, 0.0)):
        cams, pts, sm = twin(c)
        want = B.cost(cams, pts, c.idx, c.obs, c.off, used, d)
        print(name, sm, "numpy cost", want)
        assert abs(sm["finalCost"] - want) <= 1e-12 * want
        assert sm["finalCost"] < sm["initialCost"]
        trk = np.repeat(np.arange(len(c.off) - 1), np.diff(c.off))
        clean = np.setdiff1d(np.arange(len(c.off) - 1), trk[bad])       # tracks without an outlier
        assert len(clean) >= 5
        err[name] = np.linalg.norm(pts[clean] - c.truth[1][clean], axis=1).mean()
    print("mean error of the inlier points", err)
    assert err["on"] < err["off"]


def test_exclusions_come_back_bit_for_bit(native):
    c = B.case("exclusions")
    used = B.used_set(c.cams, c.pts, c.idx, c.obs, c.off)
    cams, pts, sm = twin(c)
    T = len(c.off) - 1
    assert sm["usedTracks"] == T - 3 and sm["usedObservations"] == used.sum() == len(c.idx) - 8   # 5 + 2 + 1 observations
    for t in (3, 7, 12):
        assert not used[c.off[t]:c.off[t + 1]].any() and B.same_bits(pts[t], c.pts[t]), t
    assert B.same_bits(cams[:2], c.cams[:2]) and not B.same_bits(cams[2:], c.cams[2:])
    moved = np.setdiff1d(np.arange(T), [3, 7, 12])
    assert (B.bits(pts[moved]) != B.bits(c.pts[moved])).any(axis=1).all()
    assert sm["finalCost"] < sm["initialCost"]
    assert abs(sm["finalCost"] - B.cost(cams, pts, c.idx, c.obs, c.off, used)) <= 1e-12 * sm["finalCost"]


def test_rejected_steps(native):
    """A strong perturbation with initialLambda 1e-9: trials are rejected (lambda x 10, no new
    linearisation) before the run converges all the same."""
    c = B.case("rejected")
    cams, pts, sm = twin(c)
    print(sm)
    assert sm["rejected"] > 0 and sm["accepted"] > sm["rejected"] // 2 and sm["termination"] == 1
    assert sm["finalCost"] < 1e-4 * sm["initialCost"]
    assert np.abs(pts - c.truth[1]).max() < 0.05


def test_termination_codes(native):
    for name, code in B.TERMINATION.items():
        _, _, sm = twin(B.case(name))
        assert sm["termination"] == code, (name, sm)


def _hex(a):
    return " ".join(float(v).hex() for v in np.asarray(a, np.float64).reshape(-1))


def test_host_twin_under_sanitizers(tmp_path):
    """tests/asan/bundle_adjust_asan_main.cpp: a stand-alone program (its own main, nothing preloaded,
    nothing loaded into Python) over ba_ref.h, built with -fsanitize=address,undefined and run over
    shared cases; its results equal the library's twin bit for bit."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe, inp = tmp_path / "bundle_adjust_asan", tmp_path / "cases.txt"
    src = N.ROOT / "tests" / "asan" / "bundle_adjust_asan_main.cpp"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", f"-I{N.ROOT / 'minicv_amd' / 'csrc'}", str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    names = ["exclusions", "rejected", "track_lengths", "segment_edges", "huber_on", "all_fixed", "term_lambda",
             "term_nothing", "term_zero_cost"]
    with open(inp, "w") as f:
        for name in names:
            c, cfg = B.case(name), B.case(name).config()
            f.write(f"{len(c.cams)} {len(c.off) - 1} {len(c.idx)} {0 if c.fixed is None else 1}\n")
            f.write(f"{cfg.maxIterations} {cfg.maxCgIterations} " +
                    _hex([cfg.cgTolerance, cfg.initialLambda, cfg.functionTolerance, cfg.huberDelta]) + "\n")
            f.write(_hex(c.cams) + "\n")
            if c.fixed is not None:
                f.write(" ".join(str(int(v)) for v in c.fixed) + "\n")
            f.write(" ".join(str(int(v)) for v in c.idx) + "\n" + _hex(c.obs) + "\n")
            f.write(" ".join(str(int(v)) for v in c.off) + "\n" + _hex(c.pts) + "\n")
    r = subprocess.run([str(exe), str(inp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.split("\n")
    assert f"bundle_adjust_asan ok: {len(names)} cases" in lines[4 * len(names)] and "ERROR" not in r.stderr
    for k, name in enumerate(names):
        c = B.case(name)
        cams, pts, sm = twin(c)
        head = [int(v) for v in lines[4 * k].split()]
        assert head[:7] == [sm[f] for f in ("iterations", "accepted", "rejected", "cgIterations", "usedObservations",
                                            "usedTracks", "termination")], name
        if name == "segment_edges":
            assert head[7] == 1 + 1 + 2 + 3 + 1      # kBaSeg - 1, kBaSeg, kBaSeg + 1, 2 kBaSeg + 3, 700, none
        words = [np.array([int(v, 16) for v in lines[4 * k + m].split()], np.uint64) for m in (1, 2, 3)]
        assert np.array_equal(words[0], B.bits([sm["initialCost"], sm["finalCost"]])), name
        assert np.array_equal(words[1], B.bits(cams).reshape(-1)) and np.array_equal(words[2], B.bits(pts).reshape(-1)), name
