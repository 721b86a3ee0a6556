"""CPU tests of the uint8 L2 matcher's surface (cvMatchL2U8 and the *Norm pipeline exports): the
reference the GPU tests use is itself tied to the oracle, the header / ctypes table / library agree,
and bad arguments are rejected with a message before any device is needed. No kernel runs here."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from minicv_amd import native as N
from minicv_amd import opencv, synthetic as S

import _l2u8_ref as R

ROOT = Path(__file__).resolve().parent.parent
NEW_EXPORTS = ["cvMatchL2U8", "cvMatchL2U8Multi", "mcvMatchL2U8Device", "cvMatchFeaturesNorm",
               "cvMatchAndFindModelNorm"]


@pytest.mark.parametrize("high", [256, 2])
@pytest.mark.parametrize("nq,nt,dim", [(200, 777, 128), (129, 300, 128), (64, 200, 17), (50, 100, 512),
                                       (100, 100, 1)])
def test_int64_restatement_equals_oracle(oracle, nq, nt, dim, high):
    """The yardstick of the GPU tests: the int64 numpy restatement equals the oracle's L2 matcher on the
    bytes as float32 — indices (values in [0, 2): most queries tie, the lowest index wins), second
    places, and (float)sqrt(d^2) bit for bit."""
    q, t = R.random_u8(nq, nt, dim, seed=nq + nt + dim + high, high=high)
    ref = R.match_l2_u8(q, t)
    ri, rd, ri2, rd2 = oracle.match_l2(q.astype(np.float32), t.astype(np.float32))
    R.assert_same(ref, (ri, rd, ri2, rd2))
    if high == 2 and dim <= 17:
        assert (ref[1] == ref[3]).any()          # exact ties did occur


@pytest.mark.parametrize("nt", [0, 1])
def test_restatement_few_train_rows(oracle, nt):
    q, t = R.random_u8(7, nt, 128, seed=nt)
    ref = R.match_l2_u8(q, t)
    assert (ref[2] == -1).all() and np.isinf(ref[3]).all()
    if nt:
        R.assert_same(ref, oracle.match_l2(q.astype(np.float32), t.astype(np.float32)))
    else:
        assert (ref[0] == -1).all() and np.isinf(ref[1]).all()


def test_sqrt_in_double_equals_sqrt_in_float():
    """(float)sqrt((double)d2) == sqrtf((float)d2) for every d2 the matcher can produce on a sample and
    at the ends of its range (d2 <= 512 * 255^2 < 2^25: exact in fp32 only below 2^24)."""
    d2 = np.unique(np.r_[0:70000, 2 ** 24 - 3:2 ** 24 + 3, 512 * 255 * 255 - 5:512 * 255 * 255 + 1,
                         np.random.default_rng(0).integers(0, 512 * 255 * 255 + 1, size=200000)])
    a = np.sqrt(d2.astype(np.float64)).astype(np.float32)
    exact32 = d2 < 2 ** 24
    b = np.sqrt(d2[exact32].astype(np.float32))
    np.testing.assert_array_equal(a[exact32], b)


def test_header_declares_and_library_resolves(native):
    txt = (ROOT / "include" / "minicv_native.h").read_text()
    names = set(re.findall(r"MCV_API\s+[\w\s\*]+?\b(\w+)\s*\(", txt))
    for n in NEW_EXPORTS:
        assert n in names, n
        assert n in N.SIGNATURES, n
        assert getattr(native.lib(), n) is not None
    for macro, val in (("MCV_NORM_AUTO", N.NORM_AUTO), ("MCV_NORM_L2", N.NORM_L2),
                       ("MCV_NORM_HAMMING", N.NORM_HAMMING)):
        m = re.search(rf"#define\s+{macro}\s+(\d+)", txt)
        assert m and int(m.group(1)) == val
    assert (N.NORM_AUTO, N.NORM_L2, N.NORM_HAMMING) == (0, 4, 6)      # OpenCV's NormTypes
    assert native.lib().mcvAbiVersion() == 3
    assert C.sizeof(N.MatchConfig) == 16


def _call_u8(L, name, q, t, dim, outs, device_count=None):
    args = [q.ctypes.data, q.shape[0], t.ctypes.data, t.shape[0], dim]
    if device_count is not None:
        args.append(device_count)
    return getattr(L, name)(*args, *outs)


@pytest.mark.parametrize("dim", [0, 513, -1])
def test_dim_out_of_range_rejected(native, dim):
    L = native.lib()
    q = np.zeros((4, 600), np.uint8)
    o = [np.zeros(4, np.int32), np.zeros(4, np.float32), np.zeros(4, np.int32), np.zeros(4, np.float32)]
    ptrs = [x.ctypes.data for x in o]
    assert _call_u8(L, "cvMatchL2U8", q, q, dim, ptrs) == -1
    assert f"dim {dim} outside [1, 512]" in native.last_error()
    assert _call_u8(L, "cvMatchL2U8Multi", q, q, dim, ptrs, device_count=2) == -1
    assert "outside [1, 512]" in native.last_error()
    assert L.mcvMatchL2U8Device(q.ctypes.data, 4, q.ctypes.data, 4, dim, *ptrs, None) == -1
    assert "outside [1, 512]" in native.last_error()


def test_null_outputs_and_sizes_rejected(native):
    L = native.lib()
    q = np.zeros((4, 128), np.uint8)
    o = [np.zeros(4, np.int32), np.zeros(4, np.float32)]
    assert L.cvMatchL2U8(q.ctypes.data, 4, q.ctypes.data, 4, 128, None, o[1].ctypes.data, None, None) == -1
    assert "bad argument" in native.last_error()
    assert L.cvMatchL2U8(q.ctypes.data, 4, q.ctypes.data, 4, 128, o[0].ctypes.data, None, None, None) == -1
    assert "bad argument" in native.last_error()
    assert L.cvMatchL2U8(None, 4, q.ctypes.data, 4, 128, o[0].ctypes.data, o[1].ctypes.data, None, None) == -1
    assert "bad argument" in native.last_error()
    assert L.mcvMatchL2U8Device(q.ctypes.data, 4, q.ctypes.data, 4, 128, None, None, None, None, None) == -1
    assert "bad argument" in native.last_error()
    assert L.cvMatchL2U8(q.ctypes.data, -1, q.ctypes.data, 4, 128, o[0].ctypes.data, o[1].ctypes.data, None,
                         None) == -1
    # beyond the stated row limit (2^24): rejected before anything is read
    big = (1 << 24) + 1
    assert L.cvMatchL2U8(q.ctypes.data, 4, q.ctypes.data, big, 128, o[0].ctypes.data, o[1].ctypes.data, None,
                         None) == -1
    assert "nt" in native.last_error() and str(1 << 24) in native.last_error()
    assert L.cvMatchL2U8Multi(q.ctypes.data, 4, q.ctypes.data, 4, 128, 0, o[0].ctypes.data, o[1].ctypes.data, None,
                              None) == -1
    assert "deviceCount" in native.last_error()


def _features(kind):
    pa, da, pb, db, _ = S.feature_pair_problem(40, 50, seed=3, kind=kind)
    return opencv.Features(pa, da), opencv.Features(pb, db)


@pytest.mark.parametrize("norm", [1, 2, 5, 7, -4, 100])
def test_unknown_norm_rejected(native, norm):
    A, B = _features("sift_u8")
    with pytest.raises(N.NativeError, match=f"norm {norm} is none of"):
        opencv.matchFeatures(A, B, norm=norm)
    with pytest.raises(N.NativeError, match=f"norm {norm} is none of"):
        opencv.matchAndFindModel(A, B, norm=norm)


def test_hamming_on_float_rejected(native):
    A, B = _features("l2")
    with pytest.raises(N.NativeError, match="MCV_NORM_HAMMING needs uint8"):
        opencv.matchFeatures(A, B, norm=N.NORM_HAMMING)
    with pytest.raises(N.NativeError, match="MCV_NORM_HAMMING needs uint8"):
        opencv.matchAndFindModel(A, B, norm=N.NORM_HAMMING)


def test_valid_arguments_need_a_device(native):
    """No CPU fallback: without a GPU a valid call fails with the no-device message; with one it runs
    and gives the reference's answer."""
    q, t, _ = S.sift_u8_problem(40, 60, seed=1)
    A, B = _features("sift_u8")
    if native.lib().mcvDeviceCount() > 0:
        R.assert_same(opencv.matchL2U8(q, t), R.match_l2_u8(q, t))
        opencv.matchFeatures(A, B, norm=N.NORM_L2)
        return
    with pytest.raises(N.NativeError, match="no HIP device"):
        opencv.matchL2U8(q, t)
    with pytest.raises(N.NativeError, match="no HIP device"):
        opencv.matchL2U8(q, t, deviceCount=3)
    for norm in (N.NORM_AUTO, N.NORM_L2, N.NORM_HAMMING):
        with pytest.raises(N.NativeError, match="no HIP device"):
            opencv.matchFeatures(A, B, norm=norm)
    with pytest.raises(N.NativeError, match="no HIP device"):
        opencv.matchAndFindModel(A, B, norm=N.NORM_L2)


def test_sift_u8_problem_shape_and_ties():
    q, t, planted = S.sift_u8_problem(500, 800, seed=4)
    assert q.dtype == np.uint8 and t.dtype == np.uint8 and q.shape == (500, 128) and t.shape == (800, 128)
    assert len(np.unique(t, axis=0)) < len(t)                 # duplicated train rows
    idx, d, idx2, d2 = R.match_l2_u8(q, t)
    assert (d == d2).any()                                    # hence exact ties for some queries
    ok = planted >= 0
    assert np.mean((t[idx[ok]] == t[planted[ok]]).all(axis=1)) > 0.99
    q2, t2, _ = S.sift_u8_problem(500, 800, seed=4)
    np.testing.assert_array_equal(q, q2)
    np.testing.assert_array_equal(t, t2)
    pa, da, pb, db, pl = S.feature_pair_problem(30, 40, seed=2, kind="sift_u8")
    assert da.dtype == np.uint8 and da.shape == (30, 128) and db.shape == (40, 128)
