"""A host thread that switches devices between calls: every host driver keeps its buffers, streams and
events in a workspace per (thread, device, slot) (mcv_runtime.h, thread_device_ws), so a call on device 0,
the same call with device 1 current and the call on device 0 again return the same bytes and, where the
driver counts them, the same launches, synchronisations, copies and memsets.

Needs two visible GPUs; with one the cases skip at run time. Host-pointer exports only, on the smallest
shapes that still take every kernel of the call. Every comparison is on bytes; none has a tolerance."""
import ctypes as C

import numpy as np
import pytest

import _ba_cases as A
import _matcher_cases as M
import _scaled_batch as B
import _tracks_ref as T
import _triangulate_ref as R
from minicv_amd import native as N, opencv

pytestmark = pytest.mark.gpu

S = M.S   # the generators the matcher cases are built from


def switching(run):
    """run() with device 0 current, with device 1 current and with device 0 again; all three equal."""
    import torch
    if N.lib().mcvDeviceCount() < 2:
        pytest.skip("needs two visible GPUs: the calling thread cannot switch devices with one")
    home = torch.cuda.current_device()
    out = []
    try:
        for dev in (0, 1, 0):
            torch.cuda.set_device(dev)
            assert torch.cuda.current_device() == dev
            out.append(run())
    finally:
        torch.cuda.set_device(home)
    assert out[0] == out[1], "the call on device 1 differs from the call on device 0"
    assert out[0] == out[2], "the call back on device 0 differs from the first"
    return out[0]


def raw(*arrays):
    return tuple(np.ascontiguousarray(a).tobytes() for a in arrays)


def stats(export):
    st = (C.c_longlong * 8)()
    assert getattr(N.lib(), export)(st) == 0
    return tuple(st)


# ---- triangulation: 3 tracks, one longer than TRI_SHORT_MAX (the workgroup-per-track kernel)

def tri_problem():
    p = R.Problem(*S.track_problem(3, 71, lengths=(2, 5, N.TRI_SHORT_MAX + 1), n_cameras=32)[:4])
    assert p.lengths().tolist() == [2, 5, 17] and p.enough_points()
    return p


@pytest.mark.parametrize("export", ["cvIntersectRays", "cvTriangulateTracks"])
def test_triangulate(gpu, export):
    p = tri_problem()

    def run():
        k, _, out = R.call_export(export, p)
        assert k == int((p.counts > 0).sum()), N.last_error()
        R.assert_same(tuple(a[:p.T] for a in (out[:2] if export == "cvIntersectRays" else out)), p, export)
        return raw(*out), k, stats("mcvTestTriangulateStats")
    _, _, st = switching(run)
    assert st[4] == 2 and st[5] == 1   # two short tracks, one long


# ---- track building: one component above TRK_SHORT_MAX (a workgroup sorts it) and three small ones

def test_build_tracks(gpu):
    L = N.TRK_SHORT_MAX + 8
    chain = [(k, k + 1, [(0, 0)], None) for k in range(L - 1)]
    small = [(0, 1, [(1, 1)], None), (2, 3, [(1, 1)], None), (3, 4, [(1, 1)], None), (6, 7, [(1, 1)], None)]
    c = T.Case([2] * L, chain + small)
    want = T.reference(c)
    assert want.T == 4 and np.diff(want.trackOffsets).max() == L

    def run():
        k, got, _ = T.run("cvBuildTracks", c)
        assert k == want.T, N.last_error()
        T.assert_same(got, want, "cvBuildTracks")
        return raw(got.trackOffsets, got.cameraIdx, got.featureIdx, got.trackOfFeature, got.dropped), stats(
            "mcvTestTracksStats")
    _, st = switching(run)
    assert st[5] == 1   # the long component took the workgroup sort


# ---- findScaled: 2 problems of 8 observations, each by its own call and both in one batch

def scaled_batch():
    return B.build((8, 8), None, 500)


def test_find_scaled_pose(gpu):
    b = scaled_batch()
    got = switching(lambda: raw(*B.single_results(b)))
    assert np.isfinite(np.frombuffer(got[0])).all()


def test_find_scaled_pose_batch(gpu):
    b = scaled_batch()

    def run():
        k, costs, scales, ev, _ = B.call("cvFindScaledPoseBatch", b)
        assert k == b.P, N.last_error()
        return raw(costs, scales, ev), stats("mcvTestScaledBatchStats")
    got, _ = switching(run)
    assert got == raw(*B.single_results(b))


# ---- bundle adjustment: 2 cameras, 8 tracks, 2 iterations

def test_bundle_adjust(gpu):
    c = A.scene(41, 2, 8, noise=1e-3, nFixed=1, maxIterations=2)
    ret, hc, hp, hsm = A.run("mcvHostBundleAdjust", c)
    assert ret == 2 and hsm["accepted"] >= 1, (ret, hsm)

    def run():
        k, cams, pts, sm = A.run("cvBundleAdjust", c)
        assert k == ret and sm == hsm, (k, sm, N.last_error())
        return raw(cams, pts), stats("mcvTestBundleAdjustStats")
    got, _ = switching(run)
    assert got == raw(hc, hp)


# ---- the matchers: 33 queries x 65 train rows (a partial query tile, three train tiles)

NQ, NT = 33, 65


def matcher_inputs(kind):
    if kind == "hamming":
        q, t, _ = S.hamming_problem(NQ, NT, seed=81)
        return opencv.matchHamming, q, t
    if kind == "l2u8":
        q, t, _ = S.sift_u8_problem(NQ, NT, seed=82)
        return opencv.matchL2U8, q, t
    q, t, _ = S.l2_problem(NQ, NT, dim=int(kind[3:]), seed=83)   # l2_<dim>
    return opencv.matchL2, q, t


@pytest.mark.parametrize("kind", ["hamming", "l2_32", "l2_130", "l2u8"])
def test_matchers(gpu, oracle, kind):
    fn, q, t = matcher_inputs(kind)
    got = switching(lambda: raw(*fn(q, t)))
    if kind == "hamming":
        ref = oracle.match_hamming(q, t)
    else:
        i1, d1, i2, d2 = oracle.match_l2(q.astype(np.float32), t.astype(np.float32))
        ref = (i1, d1.astype(np.float32), i2, d2.astype(np.float32))
    assert got == raw(*ref)


def test_match_l2_multi(gpu):
    """Two query shards: slot 0 on the calling thread's device, slot 1 on the other one, so the call from
    device 0 and the call from device 1 use all four (device, slot) workspaces."""
    fn, q, t = matcher_inputs("l2_32")
    got = switching(lambda: raw(*fn(q, t, deviceCount=2)))
    assert got == switching(lambda: raw(*fn(q, t)))


# ---- the pipeline: 64 x 64 byte descriptors, homography, fixed iterations

def test_match_and_find_model(gpu):
    pa, da, pb, db, _ = S.feature_pair_problem(64, 64, seed=91)
    fa, fb = opencv.Features(pa, da), opencv.Features(pb, db)
    p = opencv.RansacParams(threshold=3.0, max_iters=256, fixed_iters=True, seed=7)

    def run():
        cnt, H, pairs, mask = opencv.matchAndFindModel(fa, fb, ratio=0.8, params=p)
        return raw(H, pairs, mask), cnt
    _, cnt = switching(run)
    assert cnt >= 4
