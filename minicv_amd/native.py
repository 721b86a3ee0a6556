"""ctypes binding of libMiniCVNative.so — the same entry points the F# `module OpenCV.Native`
binds with [<DllImport("MiniCVNative")>] (/root/reference/src/MiniCV/OpenCV.fs:339-382), plus the
new hot-path exports declared in include/minicv_native.h.

The library is the product: there is no Python or CPU fallback. If it is missing, importing the
binding raises. Build it with `python -m minicv_amd.build` (or __graft_entry__.build()).
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
LIB_PATH = Path(os.environ.get("MINICV_NATIVE_LIB",
                               ROOT / "libs" / "Native" / "MiniCV" / "linux" / "AMD64" / "libMiniCVNative.so"))


class V2d(C.Structure):
    _fields_ = [("X", C.c_double), ("Y", C.c_double)]


class V3d(C.Structure):
    _fields_ = [("X", C.c_double), ("Y", C.c_double), ("Z", C.c_double)]


class M33d(C.Structure):
    _fields_ = [("M", C.c_double * 9)]


class Camera(C.Structure):
    """mcvCamera: the MiniCV Camera record (src/MiniCV/Camera.fs:7-14), field order kept."""
    _fields_ = [("location", V3d), ("forward", V3d), ("up", V3d), ("right", V3d), ("focal", V2d)]


class Ray3d(C.Structure):
    """mcvRay3d: Aardvark's Ray3d (origin, direction), 48 bytes."""
    _fields_ = [("origin", V3d), ("direction", V3d)]


class BaConfig(C.Structure):
    """mcvBaConfig; BaConfig.default() holds the library's defaults."""
    _fields_ = [("maxIterations", C.c_int), ("maxCgIterations", C.c_int), ("cgTolerance", C.c_double),
                ("initialLambda", C.c_double), ("functionTolerance", C.c_double), ("huberDelta", C.c_double)]

    @classmethod
    def default(cls, **kw) -> "BaConfig":
        c = cls(50, 64, 0.1, 1e-3, 1e-6, 0.0)
        for k, v in kw.items():
            if k not in dict(cls._fields_):
                raise TypeError(f"BaConfig has no field {k}")
            setattr(c, k, v)
        return c


class BaSummary(C.Structure):
    """mcvBaSummary."""
    _fields_ = [("initialCost", C.c_double), ("finalCost", C.c_double), ("iterations", C.c_int),
                ("accepted", C.c_int), ("rejected", C.c_int), ("cgIterations", C.c_int),
                ("usedObservations", C.c_int), ("usedTracks", C.c_int), ("termination", C.c_int)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class BaFocalConfig(C.Structure):
    """mcvBaFocalConfig: mcvBaConfig and focalMode (0 constant, 1 one scale per group, 2 fx and fy)."""
    _fields_ = [("base", BaConfig), ("focalMode", C.c_int), ("pad", C.c_int)]

    @classmethod
    def default(cls, focalMode: int = 1, **kw) -> "BaFocalConfig":
        return cls(BaConfig.default(**kw), focalMode, 0)


class BaFocalSummary(C.Structure):
    """mcvBaFocalSummary."""
    _fields_ = [("base", BaSummary), ("freeFocalGroups", C.c_int), ("pad", C.c_int)]

    def as_dict(self) -> dict:
        return dict(self.base.as_dict(), freeFocalGroups=self.freeFocalGroups)


class RecoverPoseConfig(C.Structure):
    """MiniCVNative.cpp:39-46 / OpenCV.fs:16-36."""
    _fields_ = [("FocalLength", C.c_double), ("PrincipalPoint", V2d), ("Probability", C.c_double),
                ("InlierThreshold", C.c_double)]


class RansacConfig(C.Structure):
    _fields_ = [("threshold", C.c_double), ("confidence", C.c_double), ("maxIters", C.c_int),
                ("method", C.c_int), ("seed", C.c_uint64), ("deviceCount", C.c_int), ("flags", C.c_int),
                ("errorKind", C.c_int), ("pnpKind", C.c_int)]


class KeyPoint2d(C.Structure):
    """MiniCVNative.h:14-21 / OpenCV.fs:300-310 (28 bytes)."""
    _fields_ = [("X", C.c_float), ("Y", C.c_float), ("size", C.c_float), ("angle", C.c_float),
                ("response", C.c_float), ("octave", C.c_int), ("class_id", C.c_int)]


class DetectorResult(C.Structure):
    """MiniCVNative.h:23-29 / OpenCV.fs:329-337."""
    _fields_ = [("PointCount", C.c_int), ("DescriptorEntries", C.c_int), ("DescriptorElementType", C.c_int),
                ("Points", C.c_void_p), ("Descriptors", C.c_void_p)]


class SiftConfig(C.Structure):
    """SiftConfig (MiniCVNative.h:79-86, 40 bytes); SiftConfig.default() holds cv::SIFT's defaults with byte
    descriptors, which cvDetectFeatures also takes for a NULL config."""
    _fields_ = [("FeatureCount", C.c_int), ("OctaveLayers", C.c_int), ("ContrastThreshold", C.c_double),
                ("EdgeThreshold", C.c_double), ("Sigma", C.c_double), ("DescriptorType", C.c_int)]

    @classmethod
    def default(cls, **kw) -> "SiftConfig":
        c = cls(0, 3, 0.04, 10.0, 1.6, 0)
        for k, v in kw.items():
            if k not in dict(cls._fields_):
                raise TypeError(f"SiftConfig has no field {k}")
            setattr(c, k, v)
        return c


class mcvImage(C.Structure):
    """One image of cvDetectFeaturesBatch (24 bytes): data is height x width x channels bytes, reserved 0."""
    _fields_ = [("data", C.c_void_p), ("width", C.c_int), ("height", C.c_int), ("channels", C.c_int),
                ("reserved", C.c_int)]


class MatchConfig(C.Structure):
    _fields_ = [("ratio", C.c_float), ("crossCheck", C.c_int), ("maxDistance", C.c_float), ("model", C.c_int)]


class ReplayState(C.Structure):
    _fields_ = [("niters", C.c_int64), ("bestIndex", C.c_int64), ("bestCount", C.c_int32),
                ("stopped", C.c_int32)]


METHOD_LSQ = 0
METHOD_RANSAC = 8
METHOD_LMEDS = 4    # cv::LMEDS (findHomography / findFundamentalMat)
FLAG_FIXED_ITERS = 1
FLAG_NO_REFINE = 2
FLAG_FUSED_ERROR = 64   # bit 4 is retired (rejected by the library)
FLAG_CV_SAMPLER = 32    # OpenCV's own sample stream (cv::RNG(-1) + getSubset)
FLAG_SEVEN_POINT = 8
FLAG_FAST_MINIMAL = 16
FERR_SAMPSON = 0
FERR_EPIPOLAR = 1
MODEL_HOMOGRAPHY = 0
MODEL_FUNDAMENTAL = 1
MODEL_ESSENTIAL = 2
MODEL_PNP = 3
MODEL_AFFINE = 4        # estimateAffine2D: 3-point samples, 2x3 model
MODEL_SIMILARITY = 5    # estimateAffinePartial2D: 2-point samples, [a -b tx; b a ty]
A_SWEEP_K = 8           # hypotheses per wave of the packed affine sweep (kernels.h kVerifyAHypPerWave)
BATCH_TILE = 1024       # points per LDS tile of the batched sweep (kernels.h kBatchTile)
BATCH_SLOT_CAP = 1 << 21   # slots per hypothesis round of cvFindModelBatch (ransac_batch_host.cpp)
BATCH_E_TILE = 512         # double4 points per LDS tile of the batched essential sweep (kernels.h kBatchETile)
BATCH_E_HYP_CAP = 1 << 18  # hypotheses per round of the essential batches (ransac_batch_host.cpp)
BATCH_PNP_TILE = 512       # PnpPoint rows per LDS tile of the batched PnP sweep (kernels.h kBatchPnpTile)
BATCH_PNP_WIDTH = 64       # poses (lanes) per workgroup of that sweep (kernels.h kBatchPnpWidth)
BATCH_PNP_HYP_CAP = 1 << 18  # hypotheses per round of cvSolvePnPRansacBatch (ransac_batch_host.cpp)
MATCH_BATCH_ROWS_HAMMING = 64   # query rows per workgroup of the batched matcher (kernels.h)
MATCH_BATCH_ROWS_L2 = 128
MAX_TRACK_LEN = 4096            # rays per track of the triangulation exports (MCV_MAX_TRACK_LEN)
TRI_SHORT_MAX = 16              # longer tracks take the workgroup-per-track kernel (kernels.h kTriShortMax)
TRK_SHORT_MAX = 32              # larger components are sorted by a workgroup each (kernels.h kTrkShortMax)
TRK_LAUNCHES = 13               # kernel launches of a cvBuildTracks call (kernels.h kTrkLaunches)
TRK_SCAN_ITEMS = 2048           # nodes per block of the two scans of cvBuildTracks (kernels.h kTrkScanItems)
TRK_SCAN_CHUNK = 1024           # block sums per trip of mcv_trk_scan, which carries between trips (kernels.h kTrkScanChunk)
# blocks of the fixed grids that stride over a length (kernels.h kTrkGrid, kTriGrid, kBaGrid, kBaLongBlocks):
# the sizes past which a kernel takes a second trip, for the scale cases of the test suite
TRK_GRID = 2048                 # of 256 threads: nodes, edges, slots, candidates; blocks over the long queue
TRI_GRID = 2048                 # of 256 threads over the observations; 8 x as many blocks over the long queue
BA_GRID = 2048                  # of 256 threads over the observations
BA_LONG_BLOCKS = 1024           # of 4 waves, one long track per wave and trip
BA_SEG = 1024                   # entries per segment of a camera's list in cvBundleAdjust (ba_terms.h kBaSeg)
BA_SHORT_MAX = 64               # longer tracks take the wave-per-track kernels (ba_terms.h kBaShortMax)
BA_CG_CHUNK = 8                 # PCG iterations between two reads of the solve's record (ba_terms.h kBaCgChunk)
# kernel launches of cvBundleAdjust's stages (kernels.h kBaLaunches*): the call's total is
# SETUP + COST + LINEARIZE x linearisations + (SYSTEM + TRIAL) x trials + CG_ITER x BA_CG_CHUNK x chunks
BA_LAUNCHES = {"setup": 3, "cost": 2, "linearize": 4, "system": 4, "cg_iter": 5, "trial": 5}
# the same of cvBundleAdjustFocal with focalMode 1 or 2 (kernels.h kBafLaunches*); focalMode 0 has BA_LAUNCHES
BA_FOCAL_LAUNCHES = {"setup": 4, "cost": 2, "linearize": 6, "system": 5, "cg_iter": 6, "trial": 6}
FEATURE_AKAZE, FEATURE_ORB, FEATURE_BRISK, FEATURE_SIFT = 1, 2, 3, 4   # the reference's DetectorMode
SIFT_MAX_SIDE = 8192            # width and height cap of cvDetectFeatures (sift_math.h kSiftMaxSide)
SIFT_MAX_LAYERS = 6             # OctaveLayers 1 .. 6 (sift_math.h kSiftMaxLayers)
SIFT_MAX_SIGMA = 4.0            # sift_math.h kSiftMaxSigma
# kernel launches of a cvDetectFeatures call (kernels.h kSiftLaunches*), and its synchronisations,
# copies and memsets (kSiftSyncs, kSiftCopies, kSiftMemsets)
SIFT_LAUNCHES = {"fixed": 10, "per_blur": 2, "extrema": 1, "downsample": 1, "select": 1}
SIFT_SYNCS, SIFT_COPIES, SIFT_MEMSETS = 4, 7, 1


def sift_octaves(width: int, height: int) -> int:
    """nOctaves of a width x height image: round(log2(min(2 w, 2 h)) - 2), at least 0."""
    import math
    return max(int(round(math.log2(2 * min(width, height)) - 2.0)), 0)


def sift_launches(width: int, height: int, octave_layers: int = 3, feature_count: int = 0) -> int:
    """Kernel launches of one cvDetectFeatures call on a width x height image (0 without an octave)."""
    n, L = sift_octaves(width, height), SIFT_LAUNCHES
    if n == 0:
        return 0
    return (L["fixed"] + n * (L["per_blur"] * (octave_layers + 2) + L["extrema"]) + (n - 1) * L["downsample"]
            + (L["select"] if feature_count > 0 else 0))


# cvDetectFeaturesBatch: the caps (sift_math.h kSiftBatchMax*), the bytes of one row of the
# per-image table, the launches that do not depend on the octaves, the other three counts and the blocks
# of the grid-wide scans (sift_batch_plan.h)
SIFT_BATCH_MAX_IMAGES = 4096
SIFT_BATCH_MAX_CANDIDATES = 1 << 24
SIFT_BATCH_MAX_WORKSPACE_BYTES = 1 << 35
SIFT_BATCH_IMAGE_BYTES = 360
SIFT_BATCH_LAUNCHES_FIXED = 16
SIFT_BATCH_SYNCS, SIFT_BATCH_COPIES, SIFT_BATCH_MEMSETS = 4, 8, 1
SIFT_BATCH_SCAN_BLOCKS = 1024


def sift_batch_launches(sizes, octave_layers: int = 3, feature_count: int = 0) -> int:
    """Kernel launches of one cvDetectFeaturesBatch call on images of the (width, height) in `sizes`: the
    single call's formula for the largest nOctaves among them, with SIFT_BATCH_LAUNCHES_FIXED (0 when no
    image has an octave)."""
    n, L = max([sift_octaves(w, h) for w, h in sizes], default=0), SIFT_LAUNCHES
    if n == 0:
        return 0
    return (SIFT_BATCH_LAUNCHES_FIXED + n * (L["per_blur"] * (octave_layers + 2) + L["extrema"])
            + (n - 1) * L["downsample"] + (L["select"] if feature_count > 0 else 0))


SIN_MIN_ANGLE = float.fromhex("0x1.1de58c9f7dc27p-5")   # hyp_rays.h kSinMinAngle
E_SLOTS = 10
NORM_AUTO = 0       # by element type: uint8 -> Hamming, float32 -> L2 (cvMatchFeatures' rule)
NORM_L2 = 4         # OpenCV numbering; uint8 + L2 = the exact int8 matcher (byte SIFT)
NORM_HAMMING = 6

_P = C.c_void_p
_I = C.c_int
_I64 = C.c_int64
_U64 = C.c_uint64
_D = C.c_double
_F = C.c_float

# name -> (restype, argtypes). Pointers are passed as void* (numpy .ctypes.data / device ints).
SIGNATURES = {
    # existing reference exports (OpenCV.fs:343-382)
    "cvRecoverPose": (_I, [_P, _I, _P, _P, _P, _P, _P]),
    "cvRecoverPoses": (_I, [_P, _I, _P, _P, _P, _P, _P, _P]),
    "cvDetectFeatures": (_P, [_P, _I, _I, _I, _I, _P]),
    "cvFreeFeatures": (None, [_P]),
    "cvTest": (None, []),
    "cvFivePoint": (_I, [_P, _P, _P]),
    "cvSolvePnP": (_I, [_P, _P, _I, M33d, _P, _I, _P, _P]),
    "cvSolvePnPRansac": (_I, [_P, _P, _I, M33d, _P, _I, _I, _F, _D, _P, _P, _P, _P]),
    "cvRefinePnPLM": (None, [_P, _P, _I, M33d, _P, _P, _P]),
    "cvRefinePnPVVS": (None, [_P, _P, _I, M33d, _P, _P, _P]),
    "solveAp3p": (_I, [_P, _P] + [_D] * 19),
    "cvDetectQRCode": (_I, [_P, _I, _I, _I, _P, _P]),
    "cvDetectArucoMarkers": (_I, [_P, _I, _I, _I, _P, _P]),
    # new hot-path exports
    "cvFindHomography": (_I, [_P, _P, _I, _P, _P, _P]),
    "cvFindFundamentalMat": (_I, [_P, _P, _I, _P, _P, _P]),
    "cvFindEssentialMat": (_I, [_P, _P, _I, _D, V2d, _P, _P, _P]),
    "cvEstimateAffine2D": (_I, [_P, _P, _I, _P, _P, _P]),
    "cvEstimateAffinePartial2D": (_I, [_P, _P, _I, _P, _P, _P]),
    "cvFindModelBatch": (_I, [_I, _P, _P, _P, _I, _P, _P, _P, _P]),
    "cvFindEssentialMatBatch": (_I, [_P, _P, _P, _I, _P, _P, _P, _P, _P, _P]),
    "cvRecoverPoseBatch": (_I, [_P, _P, _P, _P, _I, _P, _P, _P, _P]),
    "cvSolvePnPRansacCfg": (_I, [_P, _P, _I, M33d, _P, _P, _P, _P, _P, _P]),
    "cvSolvePnPRansacBatch": (_I, [_P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P]),
    "cvRefinePnPBatch": (_I, [_P, _P, _P, _I, _P, _P, _P, _I, _P, _P, _P]),
    "cvSolvePnPRansacRefineBatch": (_I, [_P, _P, _P, _I, _P, _P, _P, _I, _P, _P, _P, _P]),
    "cvMatchFeatures": (_I, [_P, _P, _P, _P, _P, _I]),
    "cvMatchAndFindModel": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _P]),
    "cvMatchFeaturesNorm": (_I, [_P, _P, _P, _I, _P, _P, _I]),
    "cvMatchAndFindModelNorm": (_I, [_P, _P, _P, _I, _P, _P, _P, _P, _I, _P]),
    "cvMatchFeaturesBatch": (_I, [_P, _I, _P, _I, _P, _I, _P, _P, _I, _P]),
    "cvMatchAndFindModelBatch": (_I, [_P, _I, _P, _I, _P, _I, _P, _P, _I, _P, _P, _P, _P]),
    "cvMatchHamming": (_I, [_P, _I, _P, _I, _I, _P, _P, _P, _P]),
    "cvMatchL2": (_I, [_P, _I, _P, _I, _I, _P, _P, _P, _P]),
    "cvMatchHammingMulti": (_I, [_P, _I, _P, _I, _I, _I, _P, _P, _P, _P]),
    "cvMatchL2Multi": (_I, [_P, _I, _P, _I, _I, _I, _P, _P, _P, _P]),
    "cvMatchL2U8": (_I, [_P, _I, _P, _I, _I, _P, _P, _P, _P]),
    "cvMatchL2U8Multi": (_I, [_P, _I, _P, _I, _I, _I, _P, _P, _P, _P]),
    "cvFindScaledPose": (_I, [_D, _P, _P, _P, _I, _P, _P, _P, _P]),
    "cvFindScaledPoseCosts": (_I, [_P, _P, _P, _I, _P, _P, _P, _P]),
    "cvIntersectRays": (_I, [_P, _P, _I, _P, _P]),
    "cvTriangulateTracks": (_I, [_P, _I, _P, _P, _P, _I, _P, _P, _P, _P]),
    "cvBuildTracks": (_I, [_P, _I, _P, _I, _P, _P, _P, _I, _P, _I, _P, _P, _I, _P, _P]),
    "cvBundleAdjustFocal": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P]),
    "cvBundleAdjust": (_I, [_P, _I, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P]),
    "cvFindScaledPoseBatch": (_I, [_P, _P, _P, _P, _I, _P, _P, _P, _I, _P, _P, _P]),
    "cvFindScaledPoseBatchCosts": (_I, [_P, _P, _P, _P, _I, _P, _P, _P, _I, _P, _P]),
    "mcvGetLastError": (C.c_char_p, []),
    "mcvDeviceCount": (_I, []),
    "mcvVersion": (C.c_char_p, []),
    "mcvAbiVersion": (_I, []),
    "mcvCvSubsets": (_I64, [_I, _I, _P, _I, _I64, _P]),
    # device-level API
    "mcvRansacPlanCreate": (_P, [_I, _I, _I64]),
    "mcvRansacPlanDestroy": (None, [_P]),
    "mcvPackCorrespondences": (_I, [_P, _P, _I, _P, _P]),
    "mcvPackEssential": (_I, [_P, _P, _I, _D, V2d, _P, _P]),
    "mcvPackPnP": (_I, [_P, _P, _I, _P, _P]),
    "mcvRansacPlanSetCamera": (_I, [_P, _P, _P]),
    "mcvRansacEvaluate": (_I, [_P, _P, _I, _P, _I64, _I64, _P, _P, _P]),
    "mcvRansacFinalize": (_I, [_P, _P, _I, _P, _I64, _P, _P, _P]),
    "mcvReplayInit": (None, [_P, _I]),
    "mcvL2LastExactScans": (_I, []),
    "mcvL2LastGemmForm": (_I, []),
    "mcvL2LastScanChunks": (_I, []),
    "mcvHammingLastQueryTiles": (_I, []),
    "mcvReplayChunk": (_I, [_P, _P, _I64, _I64, _I, _I, _D, _I]),
    "mcvReplayChunkModels": (_I, [_P, _P, _I64, _I64, _I, _I, _I, _D, _I]),
    "mcvMatchHammingDevice": (_I, [_P, _I, _P, _I, _I, _P, _P, _P, _P, _P]),
    "mcvMatchHammingDeviceForm": (_I, [_P, _I, _P, _I, _I, _P, _P, _P, _P, _I, _P]),
    "mcvMatchL2Device": (_I, [_P, _I, _P, _I, _I, _P, _P, _P, _P, _P]),
    "mcvMatchL2U8Device": (_I, [_P, _I, _P, _I, _I, _P, _P, _P, _P, _P]),
    "mcvFindScaledPoseDevice": (_I, [_P, _P, _P, _I, _P, _P, _P, _P, _P]),
    "mcvTriangulateTracksDevice": (_I, [_P, _I, _P, _P, _P, _I, _P, _P, _P, _P]),
    "mcvProfileEnable": (None, [_I]),
    "mcvProfileReset": (None, []),
    "mcvProfileRead": (_I, [C.c_char_p, _P]),
    # test hooks
    "mcvHostHypothesis": (_I, [_I, _P, _I, _U64, _I64, _P, _P, _P]),
    "mcvHostPhilox": (None, [C.c_uint32] * 6 + [_P]),
    "mcvHostFingerprint": (_U64, [_P, C.c_size_t]),
    "mcvHostGlibcMath": (_I, [_I, _P, _P, _I, _P]),
    "mcvTestFingerprint": (_I, [_P, C.c_size_t, _P]),
    "mcvTestEigLogCap": (_I, [_I]),
    "mcvTestHStaging": (_I, [_I, _P]),
    "mcvHostEssential": (_I, [_P, _I, _U64, _I64, _P, _P]),
    "mcvHostEssentialFast": (_I, [_P, _I, _U64, _I64, _P, _P]),
    "mcvHostFivePoint": (_I, [_P, _P]),
    "mcvHostFivePointRef": (_I, [_P, _P]),
    "mcvHostF7": (_I, [_P, _I, _U64, _I64, _P, _P]),
    "mcvHostDecomposeEssential": (None, [_P, _P, _P, _P]),
    "mcvHostRealRoots": (_I, [_P, _I, _I, _P]),
    "mcvHostPnP": (_I, [_P, _I, _P, _U64, _I64, _P, _P, _P]),
    "mcvHostPnPFast": (_I, [_P, _I, _P, _U64, _I64, _P, _P, _P]),
    "mcvHostPnPEpnp": (_I, [_P, _I, _P, _U64, _I64, _P, _P, _P]),
    "mcvHostPnpCert": (_I, [_P, _I, _P, _P, _P, C.c_float, _I, _P, _P]),
    "mcvHostSampsonCert": (_I, [_P, _I, _P, C.c_float, _I, _P, _P]),
    "mcvHostSqpnp": (_I, [_P, _P, _I, _P, _P, _P]),
    "mcvTestPnpSweep": (_I, [_P, _I, _P, _P, _I, C.c_float, _I, _I, _P]),
    "mcvHostEpnp5": (None, [_P, _P, _P, _P, _P]),
    "mcvHostSolveAp3p": (_I, [_P, _P, _P, _D, _D, _D, _D, _P, _P]),
    "mcvTestPnpHypotheses": (_I, [_P, _I, _P, _U64, _I64, _I, _I, _P, _P]),
    "mcvHostRodrigues": (None, [_P, _P, _P]),
    "mcvHostRodriguesInv": (None, [_P, _P]),
    "mcvTestRcpExhaustive": (C.c_longlong, [_I, _P]),
    "mcvTestDivF64": (C.c_longlong, [_I, C.c_ulonglong, C.c_longlong, _P]),
    "mcvTestHomographySweep": (_I, [_P, _I, _P, _I, _F, _I, _P]),
    "mcvTestHMfmaWuv": (_I, [_P, _I, _P, _I, _P]),
    "mcvTestHMfma": (_I, [_I, _P]),
    "mcvTestHCellMode": (_I, [_I, _I, _I, _P]),
    "mcvTestHCellBound": (_I, [_P, _I, _P, _P, _I, _F, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    "mcvTestHCellRel": (_I, [_P, _I, _P, _P, _I, _F, _I, _I, _I, _P, _I, _I, _P, _P, _P, _P, _P]),
    "mcvTestHCellPre": (_I, [_I, _P]),
    "mcvTestHGenRow": (_I, [_I, _P]),
    "mcvTestHGenerate": (_I, [_P, _I, _U64, _P, _I64, _I, _I, _P, _P, _P]),
    "mcvHostHGenRow": (_I, [_P, _I, _U64, _P, _I64, _I, _I, _P, _P, _P, _P, _P, _P]),
    "mcvTestHStage0Slots": (_I, [_I]),
    "mcvHostHStagePlan": (_I, [_I, _I, _I, _I, _I, _I, _P]),
    "mcvTestHCellSecondPass": (_I, [_I]),
    "mcvTestHListPush": (_I, [_P, _I, _P, _P, _I, _F, _I, _I, _I, _I, _P, _P, _P]),
    "mcvTestHCellPreVerdicts": (_I, [_P, _I, _P, _P, _I, _F, _I, _I, _I, _I, _P, _P, _P, _P]),
    "mcvTestErrorRank": (_I, [_I, _P, _I, _P, _I, _I, _I, _P]),
    "mcvHostErrorRank": (_I, [_I, _P, _I, _P, _I, _I, _I, _P]),
    "mcvTestAffineSweep": (_I, [_P, _I, _P, _I, _F, _I, _P]),
    "mcvHostAffineRefine": (_I, [_I, _P, _I, _P, _P]),
    "mcvHostScaledCosts": (_I, [_P, _P, _P, _I, _P, _P, _P, _P]),
    "mcvHostIntersectRays": (_I, [_P, _P, _I, _P, _P]),
    "mcvHostTriangulateTracks": (_I, [_P, _I, _P, _P, _P, _I, _P, _P, _P, _P]),
    "mcvTestTriangulateStats": (_I, [_P]),
    "mcvHostFindScaledPoseBatch": (_I, [_P, _P, _P, _P, _I, _P, _P, _P, _I, _P, _P, _P]),
    "mcvTestScaledBatchStats": (_I, [_P]),
    "mcvHostBuildTracks": (_I, [_P, _I, _P, _I, _P, _P, _P, _I, _P, _I, _P, _P, _I, _P, _P]),
    "mcvTestTracksStats": (_I, [_P]),
    "mcvHostDetectFeatures": (_P, [_P, _I, _I, _I, _I, _P]),
    "mcvTestSiftStats": (_I, [_P]),
    "mcvTestSiftStage": (_I, [_I, _P, C.c_longlong, _P]),
    "cvDetectFeaturesBatch": (C.c_longlong, [_P, _I, _I, _P, _P]),
    "cvFreeFeaturesBatch": (None, [_P, _I]),
    "mcvTestSiftBatchStats": (_I, [_P]),
    "mcvTestSiftBatchPlan": (_I, [_P, _I, _I, _P, _P]),
    "mcvHostBundleAdjustFocal": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P]),
    "mcvHostBaFocalStep": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _I, _P, _P, _D, _P, _P, _P, _P]),
    "mcvTestBundleAdjustFocalStats": (_I, [_P]),
    "mcvHostBundleAdjust": (_I, [_P, _I, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P]),
    "mcvHostBaLinearize": (_I, [_P, _I, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P]),
    "mcvHostBaStep": (_I, [_P, _I, _P, _P, _P, _P, _I, _P, _P, _D, _P, _P]),
    "mcvTestBundleAdjustStats": (_I, [_P]),
    "mcvHostBatchLayout": (_I, [_P, _I, _I, _I, C.c_longlong, _P, _P]),
    "mcvHostBatchRound": (_I, [_P, _P, _P, _P, _P, _I, _P, _I, C.c_longlong, C.c_longlong, _P, _P, _P]),
    "mcvTestBatchCap": (C.c_longlong, [C.c_longlong]),
    "mcvTestBatchStats": (_I, [_P]),
    "mcvTestBatchSweep": (_I, [_I, _P, _P, _I, _P, _P, _F, _I, _P]),
    "mcvTestBatchSweepE": (_I, [_P, _P, _I, _P, _P, _P, _I, _P]),
    "mcvTestBatchSweepPnp": (_I, [_P, _P, _I, _P, _P, _P, _F, _P]),
    "mcvHostRefinePnPBatchLayout": (_I, [_P, _I, _P, _P, _P]),
    "mcvTestRefinePnPMasked": (_I, [_P, _P, _I, _P, _P, _P, _I, _P, _P]),
    "mcvHostMatchBatchLayout": (_I, [_P, _I, _P, _I, _I, _I, _P, _P, _P, _I]),
    "mcvTestMatchBatchStats": (_I, [_P]),
    "mcvTestMatchBatchKnn": (_I, [_P, _P, _I, _I, _P, _I, _I, _P, _P, _P, _P]),
}

_lib = None


def lib() -> C.CDLL:
    """Load libMiniCVNative.so (raises if it has not been built: no fallback)."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise RuntimeError(f"libMiniCVNative.so not found at {LIB_PATH}; run __graft_entry__.build()")
        # torch bundles its own libamdhip64.so.7 / libhsa-runtime64.so.1 (same SONAMEs as /opt/rocm's).
        # Whichever process-wide copy loads first serves both; if ours loaded first, torch would bring
        # a second HIP/HSA runtime whose device init fails. So let torch's copy load first when present.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(str(LIB_PATH))
        for name, (res, args) in SIGNATURES.items():
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def last_error() -> str:
    e = lib().mcvGetLastError()
    return e.decode() if e else ""


class NativeError(RuntimeError):
    pass


def check(ok: bool, what: str) -> None:
    if not ok:
        raise NativeError(f"{what}: {last_error()}")
