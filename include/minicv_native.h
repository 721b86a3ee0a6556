/*
 * minicv_native.h — C-ABI of the MI355X-native MiniCVNative drop-in.
 *
 * The managed host (F# `module OpenCV.Native`, /root/reference/src/MiniCV/OpenCV.fs:339-382)
 * binds `[<DllImport("MiniCVNative")>]` entry points. This header declares
 *   (1) the 13 existing exports of the reference library, byte-compatible signatures
 *       (definitions: /root/reference/src/MiniCVNative/MiniCVNative.cpp:48-548, ap3p.cpp:282);
 *   (2) the new hot-path exports (findHomography / findFundamentalMat RANSAC, brute-force
 *       Hamming / L2 matching), written in the conventions of the existing ones
 *       (AoS fp64 point arrays + separate N, caller-allocated byte mask, M33d& out, int return);
 *   (3) a device-level API (plain device pointers + hipStream_t passed as void*) used by
 *       bench.py / multi-GPU ranks that keep inputs resident in HBM.
 *
 * Conventions:
 *   V2d  = 2 x double (x, y)            <-> Aardvark V2d / cv::Point2d
 *   V3d  = 3 x double                   <-> Aardvark V3d / cv::Vec3d
 *   M33d = 9 x double, row-major        <-> Aardvark M33d / cv::Matx33d
 *   masks are caller-allocated uint8[N], values 0/1
 *   no exception crosses the boundary: failure = false / 0 / NULL; mcvGetLastError() says why.
 */
#ifndef MINICV_NATIVE_H
#define MINICV_NATIVE_H

#include <stdint.h>
#include <stdbool.h>
#include <stddef.h>

#if defined(_WIN32)
#define MCV_API __declspec(dllexport)
#else
#define MCV_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef struct { double X, Y; } mcvV2d;
typedef struct { double X, Y, Z; } mcvV3d;
typedef struct { double M[9]; } mcvM33d;       /* row-major */
typedef struct { float X, Y; } mcvV2f;
/* The reference's `bool` exports (MiniCVNative.cpp:48,93,165,384,439) return a 1-byte C++ bool,
 * while the F# P/Invoke side (OpenCV.fs:343-382, no MarshalAs) reads a 4-byte Win32 BOOL: only the
 * low byte is defined there. This library returns them as a 32-bit 0/1, so the upper bytes are
 * zero and both readings agree. */
typedef int32_t mcvBool;

/* ------------------------------------------------------------------------------------------
 * (1) Existing exports of the reference (same names, same argument meaning).
 * ---------------------------------------------------------------------------------------- */

/* RecoverPoseConfig — MiniCVNative.cpp:39-46, OpenCV.fs:16-36 (40 bytes). */
typedef struct {
    double FocalLength;
    mcvV2d PrincipalPoint;
    double Probability;
    double InlierThreshold;
} RecoverPoseConfig;

/* KeyPoint2d / DetectorResult — MiniCVNative.h:14-29, OpenCV.fs:300-337. */
typedef struct {
    mcvV2f pt;
    float size;
    float angle;
    float response;
    int octave;
    int class_id;
} KeyPoint2d;

typedef struct {
    int PointCount;
    int DescriptorEntries;
    int DescriptorElementType;   /* OpenCV depth code (0 = u8, 5 = f32) */
    KeyPoint2d* Points;
    uint8_t* Descriptors;        /* row-major [PointCount][dim] */
} DetectorResult;

typedef struct {
    int Id;
    mcvV2f P0, P1, P2, P3;
} ArucoMarkerInfo;

/* Essential-matrix RANSAC + pose — MiniCVNative.cpp:197-215 (on the GPU):
 * findEssentialMat(pa, pb, f, pp, RANSAC, Probability, InlierThreshold) -> ms = RANSAC mask ->
 * recoverPose(E, ..., mask) (cheirality over the inliers, distance 50). Returns the number of
 * inliers passing the cheirality test of the chosen (R, t); 0 on failure (ms untouched). */
MCV_API int  cvRecoverPose(const RecoverPoseConfig* config, const int N, const mcvV2d* pa, const mcvV2d* pb,
                           mcvM33d* rMat, mcvV3d* tVec, uint8_t* ms);
/* MiniCVNative.cpp:165-194: findEssentialMat -> ms -> decomposeEssentialMat(E) -> R1, R2, t.
 * false if N < 5 or no model (ms untouched then). */
MCV_API mcvBool cvRecoverPoses(const RecoverPoseConfig* config, const int N, const mcvV2d* pa, const mcvV2d* pb,
                            mcvM33d* rMat1, mcvM33d* rMat2, mcvV3d* tVec, uint8_t* ms);
/* Feature detection — MiniCVNative.cpp:221-365. mode is the reference's DetectorMode; only SIFT
 * (mode 4) runs here, on the GPU: AKAZE, ORB and BRISK return NULL with an error, as does
 * any other mode. config: NULL (the defaults {0, 3, 0.04, 10.0, 1.6, 0}) or a SiftConfig.
 *   data: height x width x channels bytes, row-major. channels 1: grey; 3 or 4: RGB(A), grey =
 *   (4899 R + 9617 G + 1868 B + 8192) >> 14; anything else: NULL. width and height: 1 .. 8192.
 *   OctaveLayers 1 .. 6, 0 < Sigma <= 4, ContrastThreshold >= 0, EdgeThreshold > 0, DescriptorType 0
 *   (uint8, the reference's default: rows for cvMatchFeaturesNorm(MCV_NORM_L2)) or 5 (float32).
 * Keypoints come out ascending by (octave, layer, row, column, orientation bin); FeatureCount > 0 keeps
 * that many of the largest response. The result (PointCount may be 0) is freed with cvFreeFeatures.
 * The keypoints and descriptors are SIFT as cv::SIFT arranges it, defined bit for bit by DESIGN §7n;
 * bit parity with cv::SIFT is not claimed. NULL on failure (mcvGetLastError). */
#define MCV_FEATURE_MODE_AKAZE 1
#define MCV_FEATURE_MODE_ORB   2
#define MCV_FEATURE_MODE_BRISK 3
#define MCV_FEATURE_MODE_SIFT  4
typedef struct {   /* MiniCVNative.h:79-86 (40 bytes) */
    int FeatureCount;
    int OctaveLayers;
    double ContrastThreshold;
    double EdgeThreshold;
    double Sigma;
    int DescriptorType;
} SiftConfig;
MCV_API DetectorResult* cvDetectFeatures(char* data, int width, int height, int channels, int mode, void* config);
MCV_API void cvFreeFeatures(DetectorResult* res);
/* Batched detection: nImages independent cvDetectFeatures(mode 4) calls under one
 * SiftConfig (NULL: the defaults), in one call whose kernel launches, stream synchronisations, copies
 * and memsets do not grow with nImages. The images may differ in width, height and channels.
 * results: the caller's array of nImages DetectorResult, filled by the call: results[i] holds exactly
 * what cvDetectFeatures(images[i].data, width, height, channels, 4, config) returns (FeatureCount
 * applies per image; an image without an octave or a keypoint gives PointCount 0 with non-NULL
 * members), so the array goes straight into cvMatchFeaturesBatch / cvMatchAndFindModelBatch. Free it
 * with cvFreeFeaturesBatch. Returns the total keypoint count (0 for nImages == 0), -1 on failure
 * (mcvGetLastError; every results[i] is then all zero). Every argument is checked on the host before
 * the device is touched, an image's checks are cvDetectFeatures' with the image index in the message,
 * and one bad image fails the whole call. Design constants, not measurements: at most 4096 images
 * (kSiftBatchMaxImages), at most 1 << 24 extremum candidates of all images together
 * (kSiftBatchMaxCandidates; an image alone is held to cvDetectFeatures' 1 << 22), and at most 1 << 35
 * bytes (kSiftBatchMaxWorkspaceBytes) of the buffers whose size the arguments fix (images, pyramids,
 * blur scratch, buckets, candidate list); past any of them the error says to split the batch. */
typedef struct {            /* 24 bytes */
    const uint8_t* data;    /* height x width x channels bytes, row-major */
    int width, height, channels;
    int reserved;           /* must be 0 */
} mcvImage;
MCV_API long long cvDetectFeaturesBatch(const mcvImage* images, int nImages, int mode, void* config,
                                        DetectorResult* results);
/* Frees the members of results[0 .. nImages) and zeroes the structs. NULL and all-zero entries are fine. */
MCV_API void cvFreeFeaturesBatch(DetectorResult* results, int nImages);
/* Debug export — MiniCVNative.cpp:504 (no-op). */
MCV_API void cvTest(void);
/* Five-point minimal solver — MiniCVNative.cpp:368-382 / fivepoint.cpp:233-339 (one GPU solve of
 * the reference's own path: SVD null space, solvePoly roots with |Im| <= 1e-10 in its order):
 * Es: caller-allocated 10 x M33d, unit-Frobenius-norm E with pb^T E pa = 0. Returns the count. */
MCV_API int  cvFivePoint(const mcvV2d* pa, const mcvV2d* pb, mcvM33d* Es);
/* PnP — MiniCVNative.cpp:48-163 (on the GPU). K passed by value as in the
 * reference; distortion = 4 doubles (k1, k2, p1, p2; MiniCVNative.cpp:78,120).
 * cvSolvePnPRansac (OpenCV 4.x solvePnPRansac): solverKind 2 / 5 (P3P / AP3P) sample 4 points
 * for AP3P, kinds 0 / 1 / 3 / 4 (ITERATIVE / EPNP / DLS / UPNP) sample 5 points for EPnP (other
 * values act as 0); N == model points -> one solve on all points. fp32 reprojection error of
 * projectPoints, inlier iff err <= reprojectionError^2, sequential-RANSAC semantics with seed 0;
 * final pose on the inliers: LM from the RANSAC pose (kind 0), EPnP (every other kind).
 * outInliers (caller: N ints) = RANSAC inlier indices.
 * cvSolvePnP: kinds 2 / 5 need N == 4 (AP3P, the 4th point picks the solution); 1 / 3 / 4:
 * EPnP on all points; 0 (ITERATIVE) and values outside 0..6: EPnP, then LM over all points;
 * 6 (SQPNP, N >= 3): OpenCV's sqpnp::PoseSolver on the undistorted normalised points (computeOmega's
 * sums on the GPU, the SQP search on the host; its assertion failures return false with the reason,
 * no solution in front of the camera returns false). */
MCV_API mcvBool cvSolvePnP(const mcvV2d* imgPoints, const mcvV3d* worldPoints, const int N, const mcvM33d K,
                        const double* distortionCoeffs, const int solverKind, mcvV3d* tVec, mcvV3d* rVec);
MCV_API mcvBool cvSolvePnPRansac(const mcvV2d* imgPoints, const mcvV3d* worldPoints, const int N, const mcvM33d K,
                              const double* distortionCoeffs, const int solverKind, const int iterationsCount,
                              const float reprojectionError, const double confidence, mcvV3d* tVec, mcvV3d* rVec,
                              int* inlierCount, int* outInliers);
/* In/out pose (t, r): 20 LM iterations over all points (solvePnPRefineLM) / 20 VVS iterations with
 * lambda 1 on the normalised image plane (solvePnPRefineVVS). */
MCV_API void cvRefinePnPLM(const mcvV2d* imgPoints, const mcvV3d* worldPoints, const int N, const mcvM33d K,
                           const double* distortionCoeffs, mcvV3d* tVec, mcvV3d* rVec);
MCV_API void cvRefinePnPVVS(const mcvV2d* imgPoints, const mcvV3d* worldPoints, const int N, const mcvM33d K,
                            const double* distortionCoeffs, mcvV3d* tVec, mcvV3d* rVec);
/* AP3P — ap3p.cpp:282-317, double arguments as the reference defines them and the F# P/Invoke
 * passes them (OpenCV.fs:373-374: F# `float` is System.Double). The reference's quartic path:
 * Ferrari (std::complex) + two Newton polish passes, every root with |cos| <= 1 in its order,
 * complex roots' real parts included. Rs/ts: caller arrays of 4; R as the reference returns it
 * (ap3p.cpp:245-250). Returns the count. */
MCV_API int  solveAp3p(mcvM33d* Rs, mcvV3d* ts, double mu0, double mv0, double X0, double Y0, double Z0,
                       double mu1, double mv1, double X1, double Y1, double Z1,
                       double mu2, double mv2, double X2, double Y2, double Z2,
                       double inv_fx, double inv_fy, double cx_fx, double cy_fy);
/* Fiducials — MiniCVNative.cpp:384-502 (out of scope: return false). */
MCV_API mcvBool cvDetectQRCode(char* data, int width, int height, int channels, int* positions, int* count);
MCV_API mcvBool cvDetectArucoMarkers(char* data, int width, int height, int channels, int* infoCount,
                                  ArucoMarkerInfo* infos);

/* ------------------------------------------------------------------------------------------
 * (2) New hot-path exports (replace the OpenCV calls a maintainer would otherwise add:
 *     cv::findHomography, cv::findFundamentalMat, cv::BFMatcher(NORM_HAMMING / NORM_L2)).
 * ---------------------------------------------------------------------------------------- */

/* method codes (OpenCV numbering) */
#define MCV_METHOD_LSQ     0   /* all points, no RANSAC (OpenCV method 0) */
#define MCV_METHOD_LMEDS   4   /* cv::LMEDS, least median of squares (cvFindHomography / cvFindFundamentalMat
                                  only): no inlier threshold. RANSACUpdateNumIters(confidence, 0.45, m,
                                  maxIters) hypotheses (maxIters with MCV_FLAG_FIXED_ITERS), each model's
                                  median error (rank N / 2 of its N fp32 errors), the first smallest median
                                  wins; inliers: err <= (float)sigma^2, sigma = max(2.5 * 1.4826 *
                                  (1 + 5 / (N - m)) * sqrt(median), 0.001). Errors are ordered by their fp32
                                  bit patterns as OpenCV's nth_element over the reinterpreted ints does; the
                                  one difference: every NaN sorts after +inf here (an x86 build's negative
                                  NaNs sort first). N == m takes the direct solve, as for RANSAC. */
#define MCV_METHOD_RANSAC  8   /* cv::RANSAC */

/* flags */
#define MCV_FLAG_FIXED_ITERS  1   /* evaluate exactly maxIters hypotheses (no adaptive stop) */
#define MCV_FLAG_NO_REFINE    2   /* return the best hypothesis' model (skip inlier refit + LM) */
#define MCV_FLAG_RETIRED_4    4   /* retired: meant "unfused error" in the round-1 header (now the default);
                                     rejected with an error so an old caller cannot silently get the
                                     opposite definition */
#define MCV_FLAG_SEVEN_POINT  8   /* fundamental only: OpenCV FM_RANSAC's minimal solver (run7Point: 7-point
                                     samples, up to 3 models each, model slots 3h .. 3h+2 in the device
                                     API) instead of the 8-point default; with errorKind EPIPOLAR it is
                                     cv::findFundamentalMat(FM_RANSAC). With MCV_METHOD_RANSAC it needs N >= 15
                                     (OpenCV switches to LMeDS below that: use MCV_METHOD_LMEDS, which takes
                                     7-point samples at any N >= 7) or N == 7 (one solve, first model). */
#define MCV_FLAG_CV_SAMPLER   32  /* OpenCV's own sample stream instead of the counter-based Philox one:
                                     cv::RNG((uint64)-1) per call, getSubset's duplicate rejection and
                                     checkSubset, 10000 attempts (RANSACPointSetRegistrator::run), generated
                                     on the host before the GPU evaluates the hypotheses; cfg->seed is then
                                     unused. The default of cvRecoverPose(s) / cvSolvePnPRansac and of the
                                     NULL-config defaults; sequential by definition: <= 2^24 hypotheses */
#define MCV_FLAG_FUSED_ERROR  64  /* opt-in: FMA-contracted inlier error (what a compiler contracting
                                     OpenCV's computeError produces, e.g. clang on arm64). Default:
                                     op-by-op, every operation rounded as written = OpenCV's x86-64
                                     (SSE baseline) build, the reference's Linux/AMD64 target. */
#define MCV_FLAG_FAST_MINIMAL 16  /* opt-in replacement minimal solvers. Essential: Gauss-Jordan null space,
                                     polynomial-product constraints, Illinois real roots (default: the
                                     reference's fivepoint.cpp solver). Homography / 8-point fundamental:
                                     minimal solve by 8x8 Gaussian
                                     elimination with h22 = 1 / f22 = 1 (no eigenvalue check for F).
                                     Default: OpenCV's own runKernel / run8Point, the 9x9 cv::eigen
                                     (JacobiImpl_) of LtL / A^T A. The two agree to ~1e-11 relative; the
                                     default costs ~50x more per hypothesis on the GPU. */

/* F error metric (cfg->errorKind, fundamental only) */
#define MCV_FERR_SAMPSON   0   /* first-order geometric (Sampson) distance^2 (north_star) */
#define MCV_FERR_EPIPOLAR  1   /* OpenCV FM_RANSAC: max of the two squared point-to-epipolar-line distances */

typedef struct {
    double threshold;     /* max reprojection / epipolar distance of an inlier (point units); not read by
                             MCV_METHOD_LMEDS, which derives its own */
    double confidence;    /* RANSAC / LMedS confidence in (0,1) */
    int    maxIters;      /* hypothesis budget */
    int    method;        /* MCV_METHOD_* (LMEDS: homography, fundamental, affine and similarity only) */
    uint64_t seed;        /* counter-based sampler key: hypothesis i depends only on (seed, i) */
    int    deviceCount;   /* 0/1: one GPU; >1 shard hypotheses over that many local GPUs (MCV_METHOD_LMEDS
                             always runs on the calling device: its budget is at most maxIters, and results
                             are defined as those of one device) */
    int    flags;         /* MCV_FLAG_* */
    int    errorKind;     /* MCV_FERR_* (fundamental only) */
    int    pnpKind;       /* PnP only: the reference's solverKind (0 ITERATIVE, 1 EPNP, 2 P3P, 3 DLS, 4 UPNP,
                             5 AP3P; others = 0). 2 / 5: AP3P on 4-point sets; else EPnP on 5-point sets.
                             Final pose on the inliers: LM from the RANSAC pose (0), EPnP (1-5). */
} RansacConfig;           /* 48 bytes */

/* findHomography. src/dst: N AoS fp64 points (converted to fp32 like OpenCV's convertTo(CV_32F)).
 * H: out, row-major, H[8] == 1. mask: caller-allocated uint8[N] (RANSAC / LMedS inliers of the best
 * hypothesis; all 1 for METHOD_LSQ / N == 4). Returns the inlier count (>= 4), 0 on failure.
 * cfg->method: MCV_METHOD_LSQ, MCV_METHOD_RANSAC or MCV_METHOD_LMEDS (refit + 10 LM iterations on the
 * inliers unless MCV_FLAG_NO_REFINE, for both robust methods). */
MCV_API int cvFindHomography(const mcvV2d* src, const mcvV2d* dst, const int N, const RansacConfig* cfg,
                             mcvM33d* H, uint8_t* mask);

/* findFundamentalMat, 8-point minimal sets. a/b: N AoS fp64 points. F: out, scaled so that F[8] = 1 when
 * |F[8]| > FLT_EPSILON (run8Point's normalisation), otherwise as solved.
 * mask: caller-allocated uint8[N]. Returns inlier count (>= 8; >= 7 with MCV_FLAG_SEVEN_POINT), 0 on failure.
 * cfg->method: MCV_METHOD_LSQ, MCV_METHOD_RANSAC or MCV_METHOD_LMEDS (F as solved by the winning sample). */
MCV_API int cvFindFundamentalMat(const mcvV2d* a, const mcvV2d* b, const int N, const RansacConfig* cfg,
                                 mcvM33d* F, uint8_t* mask);

/* estimateAffine2D (6-DoF, 3-point samples) and estimateAffinePartial2D (4-DoF similarity, 2-point
 * samples): from/to N AoS fp64 points (converted to fp32). A6: out, the 2x3 matrix row-major (the
 * similarity as [a -b tx; b a ty]). mask: caller-allocated uint8[N], may be NULL. cfg->method:
 * MCV_METHOD_RANSAC or MCV_METHOD_LMEDS; the winner is refined on its inliers by 10 Levenberg-Marquardt
 * iterations (no refit first) when it has more inliers than the sample size, unless MCV_FLAG_NO_REFINE.
 * N equal to the sample size: one solve on all points, mask all 1. cfg NULL: RANSAC, threshold 3,
 * maxIters 2000, confidence 0.99, OpenCV's sample stream. Error (fp32): a = F0 x + F1 y + F2 - X,
 * b = F3 x + F4 y + F5 - Y, a a + b b <= (float)threshold^2. Returns the inlier count, 0 on failure. */
MCV_API int cvEstimateAffine2D(const mcvV2d* from, const mcvV2d* to, const int N, const RansacConfig* cfg,
                               double* A6, uint8_t* mask);
MCV_API int cvEstimateAffinePartial2D(const mcvV2d* from, const mcvV2d* to, const int N, const RansacConfig* cfg,
                                      double* A6, uint8_t* mask);

/* B independent RANSAC problems of one model family in one call. Problem p owns correspondences
 * [offsets[p], offsets[p+1]) of a / b (offsets: B + 1 ints, offsets[0] == 0, non-decreasing).
 * model: 0 homography, 1 fundamental (8-point), 4 affine, 5 similarity (the MCV_MODEL_* values of section 4).
 * models[p]: the 3x3 model (affine family: the 2x3 matrix, then 0 0 1, as cvMatchAndFindModel writes it).
 * mask: uint8[offsets[B]], may be NULL. counts[p]: inlier count of problem p, 0 when it has no model.
 * Every problem returns exactly what the model's single export (cvFindHomography, cvFindFundamentalMat,
 * cvEstimateAffine2D, cvEstimateAffinePartial2D) returns for the same slice and cfg: the same count, mask
 * bytes and nine doubles, refined models included; a NULL cfg means that export's own defaults. A problem
 * on which the single call would return 0 gets count 0, a zero model and a zero mask slice, the others
 * are untouched, and mcvGetLastError() names the first failed problem's index and its message.
 * The kernel launches and stream synchronisations of a call do not grow with B (problems with exactly
 * the sample size take the single export's direct solve, one by one).
 * cfg: method MCV_METHOD_RANSAC; flags any of MCV_FLAG_CV_SAMPLER (one stream per problem), MCV_FLAG_FIXED_ITERS,
 * MCV_FLAG_NO_REFINE; both errorKinds for F; every problem uses cfg->seed. LSQ, LMedS, MCV_FLAG_FUSED_ERROR,
 * MCV_FLAG_FAST_MINIMAL, MCV_FLAG_SEVEN_POINT, deviceCount > 1, the retired bit 4 and other models fail the
 * whole call; every argument check runs before the device is touched.
 * Returns the number of problems with a model (0 for B == 0), -1 on a bad argument or a device failure. */
MCV_API int cvFindModelBatch(int model, const mcvV2d* a, const mcvV2d* b, const int* offsets, int B,
                             const RansacConfig* cfg, mcvM33d* models, uint8_t* mask, int* counts);

/* findEssentialMat (OpenCV focal/pp overload): a/b pixel points, normalised (x - pp) / focal in
 * fp64; five-point minimal sets (<= 10 models per hypothesis), Sampson error, inlier iff
 * err <= (float)(threshold / focal)^2. cfg NULL: threshold 1, confidence 0.999, maxIters 1000,
 * seed 0. E: out, unit Frobenius norm. mask: uint8[N]. Returns the inlier count, 0 on failure.
 * N == 5 runs one solve on all points (mask all 1) and succeeds only with a single solution. */
MCV_API int cvFindEssentialMat(const mcvV2d* a, const mcvV2d* b, const int N, double focal, mcvV2d pp,
                               const RansacConfig* cfg, mcvM33d* E, uint8_t* mask);

/* B independent cvFindEssentialMat problems in one call, in cvFindModelBatch's conventions: problem p owns
 * correspondences [offsets[p], offsets[p+1]) of a / b (offsets: B + 1 ints, offsets[0] == 0, non-decreasing).
 * focal[B], pp[B]: per problem. cfg: one for all (NULL: cvFindEssentialMat's defaults with its NULL cfg).
 * E[B], mask: uint8[offsets[B]] (may be NULL), counts[B].
 * Problem p returns exactly what cvFindEssentialMat returns for its slice with focal[p], pp[p] and cfg: the
 * same count, mask bytes and nine doubles. A problem on which the single call returns 0 (N < 5, no model,
 * N == 5 with several solutions, a focal that is zero or not finite) gets count 0, a zero E and a zero mask
 * slice; the others are untouched and mcvGetLastError() names the first failed problem's index and its
 * message. The kernel launches and stream synchronisations of a call do not grow with B (problems with
 * exactly 5 correspondences take the single export, one by one).
 * cfg: method MCV_METHOD_RANSAC; flags any of MCV_FLAG_CV_SAMPLER (one cv::RNG((uint64)-1) stream per
 * problem), MCV_FLAG_FIXED_ITERS, MCV_FLAG_NO_REFINE (accepted, no effect: E has no refine); every problem
 * uses cfg->seed. Other methods, MCV_FLAG_FUSED_ERROR, MCV_FLAG_FAST_MINIMAL, deviceCount > 1 and the retired
 * bit 4 fail the whole call; every argument check runs before the device is touched.
 * Returns the number of problems with a model (0 for B == 0), -1 on a bad argument or a device failure. */
MCV_API int cvFindEssentialMatBatch(const mcvV2d* a, const mcvV2d* b, const int* offsets, int B,
                                    const double* focal, const mcvV2d* pp, const RansacConfig* cfg,
                                    mcvM33d* E, uint8_t* mask, int* counts);
/* B independent cvRecoverPose problems in one call. configs[B]: per problem (focal, principal point,
 * probability, threshold); every problem runs OpenCV's sample stream with 1000 iterations, as cvRecoverPose
 * does. R[B], t[B], ms: uint8[offsets[B]] = the RANSAC masks, good[B] = cvRecoverPose's return.
 * Problem p returns exactly what cvRecoverPose returns for its slice with configs[p]: the same count, mask
 * bytes and doubles of R and t. A problem on which the single call fails gets good 0, zero R and t and a
 * zero mask slice, and mcvGetLastError() names the first such problem. One difference from the single call:
 * cvRecoverPose leaves ms all 1 when N == 5 gives several solutions; the batch zeroes that slice.
 * A Probability outside (0, 1) fails the whole call, as do null arguments and bad offsets.
 * Returns the number of problems with a pose (0 for B == 0), -1 on a bad argument or a device failure. */
MCV_API int cvRecoverPoseBatch(const RecoverPoseConfig* configs, const mcvV2d* pa, const mcvV2d* pb,
                               const int* offsets, int B, mcvM33d* R, mcvV3d* t, uint8_t* ms, int* good);

/* cvSolvePnPRansac with a full RansacConfig (threshold = reprojection error in pixels; seed, fixed iterations, fused error, NO_REFINE). */
MCV_API mcvBool cvSolvePnPRansacCfg(const mcvV2d* imgPoints, const mcvV3d* worldPoints, const int N, const mcvM33d K,
                                 const double* distortionCoeffs, const RansacConfig* cfg, mcvV3d* tVec, mcvV3d* rVec,
                                 int* inlierCount, int* outInliers);

/* B independent cvSolvePnPRansacCfg problems in one call, in cvFindModelBatch's conventions: problem p owns
 * correspondences [offsets[p], offsets[p+1]) of imgPoints / worldPoints (offsets: B + 1 ints, offsets[0] == 0,
 * non-decreasing). K[B]: per problem; distortionCoeffs: 4 per problem (k1, k2, p1, p2), or NULL: none.
 * cfg: one for all (NULL: cvSolvePnPRansacCfg's NULL defaults: 100 iterations, 8 px, 0.99, kind 0, OpenCV's
 * sample stream). tVecs[B], rVecs[B]; mask: uint8[offsets[B]], required: the RANSAC inliers of each problem's
 * best hypothesis (the single call's index list is its non-zero positions); counts[B]: the inlier counts.
 * Problem p returns exactly what cvSolvePnPRansacCfg returns for its slice with K[p], its coefficients and
 * cfg: the same success flag, inlier set and bits of rVec and tVec, refined poses included. A problem on
 * which the single call returns false or fails (N < 4, no hypothesis with at least 4 inliers, a direct solve
 * without a solution, fx or fy zero or not finite) gets count 0, a zero pose and a zero mask slice; the
 * others are untouched and mcvGetLastError() names the first failed problem's index and its message.
 * The kernel launches, stream synchronisations and copies of a call do not grow with B (problems with exactly
 * the sample size, N == 4 and N == 5 for the 5-point kinds, take the single export, one by one).
 * cfg: method MCV_METHOD_RANSAC; every pnpKind; flags any of MCV_FLAG_CV_SAMPLER (one cv::RNG((uint64)-1)
 * stream per problem), MCV_FLAG_FIXED_ITERS, MCV_FLAG_NO_REFINE; every problem uses cfg->seed. Other methods,
 * MCV_FLAG_FUSED_ERROR, MCV_FLAG_FAST_MINIMAL, deviceCount > 1, a confidence outside (0, 1) and the retired
 * bit 4 fail the whole call, as do null arguments, a negative B and bad offsets; every argument check runs
 * before the device is touched.
 * Returns the number of problems with a pose (0 for B == 0), -1 on a bad argument or a device failure. */
MCV_API int cvSolvePnPRansacBatch(const mcvV2d* imgPoints, const mcvV3d* worldPoints, const int* offsets, int B,
                                  const mcvM33d* K, const double* distortionCoeffs, const RansacConfig* cfg,
                                  mcvV3d* tVecs, mcvV3d* rVecs, uint8_t* mask, int* counts);

/* B independent cvRefinePnPLM / cvRefinePnPVVS calls in one: the refinement step of solvePnPInternal
 * (OpenCV.fs:1006-1013) for many cameras. Problem p owns rows [offsets[p], offsets[p+1]) as in
 * cvSolvePnPRansacBatch. refineKind: 0 = LM (cvRefinePnPLM), 1 = VVS (cvRefinePnPVVS). tVecs / rVecs [B]: in
 * the start pose, out the refined one. mask: uint8[offsets[B]] or NULL (all points); any non-zero byte selects
 * the row. distortionCoeffs: 4 per problem or NULL. refined: uint8[B] or NULL.
 * With n_p the selected rows of problem p: where the single call would refine (n_p >= 3, fx and fy finite and
 * non-zero), rVecs[p] / tVecs[p] come out as the bits cvRefinePnPLM / cvRefinePnPVVS write for the selected
 * rows gathered in index order (the arrays OpenCV.fs:1006-1007 builds) with K[p], problem p's coefficients and
 * the given start pose, and refined[p] = 1. Otherwise the pose is left untouched bit for bit, refined[p] = 0
 * and mcvGetLastError() names the first such problem's index and the single call's message.
 * The kernel launches, stream synchronisations and copies of a call do not grow with B: one pack, one compact
 * and one gather launch (neither with a NULL mask), then per lockstep step (at most 21 for LM, 20 for VVS) two
 * launches and one synchronisation.
 * Returns the number of problems refined (0 for B == 0), -1 on a bad argument (a null imgPoints, worldPoints,
 * offsets, K, tVecs or rVecs, a negative B, offsets[0] != 0, decreasing offsets, a problem over the family's
 * limit of 65535 x 512 rows, a refineKind other than 0 / 1) or a device failure; every argument check runs
 * before the device is touched and before any output is written. */
MCV_API int cvRefinePnPBatch(const mcvV2d* imgPoints, const mcvV3d* worldPoints, const int* offsets, int B,
                             const mcvM33d* K, const double* distortionCoeffs, const uint8_t* mask, int refineKind,
                             mcvV3d* tVecs, mcvV3d* rVecs, uint8_t* refined);

/* solvePnPRansacWithRefine (OpenCV.fs:1051) for many cameras: cvSolvePnPRansacBatch's arguments and contract,
 * then cvRefinePnPBatch(refineKind) of every problem with a pose on the mask the first step returned. Every
 * output equals the two calls in sequence; mask and counts stay the RANSAC inliers; a problem without a pose
 * stays a zero pose and is not refined. The points are uploaded and packed once, and the refine reads the
 * packed points and the mask where the RANSAC rounds left them on the device. Refuses what
 * cvSolvePnPRansacBatch refuses and a refineKind other than 0 / 1, before the device is touched.
 * Returns the number of problems with a pose, -1 on a bad argument or a device failure. */
MCV_API int cvSolvePnPRansacRefineBatch(const mcvV2d* imgPoints, const mcvV3d* worldPoints, const int* offsets,
                                        int B, const mcvM33d* K, const double* distortionCoeffs,
                                        const RansacConfig* cfg, int refineKind, mcvV3d* tVecs, mcvV3d* rVecs,
                                        uint8_t* mask, int* counts);

/* Device-resident match -> RANSAC hand-off. Inputs are the reference's
 * DetectorResult (MiniCVNative.h:23-29: KeyPoint2d[PointCount] + row-major descriptors,
 * DescriptorElementType 0 = uint8 -> Hamming, 5 = float32 -> L2). Matching a -> b (knn 2), then
 * on the GPU: Lowe ratio test (d1 < ratio d2; ratio <= 0: off), mutual-nearest check, max
 * distance (<= 0: off), order-preserving compaction, keypoint gather into the RANSAC layout. */
typedef struct {
    float ratio;
    int   crossCheck;
    float maxDistance;
    int   model;        /* MCV_MODEL_HOMOGRAPHY, MCV_MODEL_FUNDAMENTAL, MCV_MODEL_AFFINE or
                           MCV_MODEL_SIMILARITY (cvMatchAndFindModel) */
} MatchConfig;          /* 16 bytes */

/* Matches only: pairs[2k] = index in a, pairs[2k+1] = index in b (ascending in a), dist[k]
 * (Hamming distance or L2 distance; may be NULL). Returns the match count, -1 on failure
 * (maxPairs >= a->PointCount is always enough). */
MCV_API int cvMatchFeatures(const DetectorResult* a, const DetectorResult* b, const MatchConfig* cfg, int* pairs,
                            float* dist, int maxPairs);
/* Matches + RANSAC on the matched keypoints (cvFindHomography / cvFindFundamentalMat /
 * cvEstimateAffine2D / cvEstimateAffinePartial2D semantics, cfg->method RANSAC) without leaving the GPU.
 * M: model (affine family: the 2x3 matrix, third row 0 0 1); pairs as above; mask[k]: inlier flag of
 * match k; *matchCount: number of matches written. Returns the inlier count, 0 on failure. */
MCV_API int cvMatchAndFindModel(const DetectorResult* a, const DetectorResult* b, const MatchConfig* mcfg,
                                const RansacConfig* rcfg, mcvM33d* M, int* pairs, uint8_t* mask, int maxPairs,
                                int* matchCount);

/* The same two calls with the descriptor norm chosen by the caller (OpenCV's NormTypes numbering).
 * cvMatchFeatures / cvMatchAndFindModel are the MCV_NORM_AUTO forms. uint8 descriptors under
 * MCV_NORM_L2 (byte SIFT: cv::SIFT::create(..., CV_8U), the reference's default descriptor type) take
 * the exact int8 matcher of cvMatchL2U8, in both directions when crossCheck is set; dist is then the
 * L2 distance, and every output equals that of the float32 call on the same values. uint8 + AUTO or
 * HAMMING: Hamming. float32 + AUTO or L2: L2. float32 + HAMMING, or any other norm: failure. */
#define MCV_NORM_AUTO    0   /* by element type: u8 -> Hamming, f32 -> L2 (cvMatchFeatures' rule) */
#define MCV_NORM_L2      4   /* OpenCV numbering */
#define MCV_NORM_HAMMING 6
MCV_API int cvMatchFeaturesNorm(const DetectorResult* a, const DetectorResult* b, const MatchConfig* cfg, int norm,
                                int* pairs, float* dist, int maxPairs);
MCV_API int cvMatchAndFindModelNorm(const DetectorResult* a, const DetectorResult* b, const MatchConfig* mcfg,
                                    int norm, const RansacConfig* rcfg, mcvM33d* M, int* pairs, uint8_t* mask,
                                    int maxPairs, int* matchCount);

/* B matching problems over nImages images. Problem p matches images[imagePairs[2p]] (queries) to
 * images[imagePairs[2p+1]] (train). pairs / dist: CSR over the problems, problem p owns
 * [offsets[p], offsets[p+1]) (offsets: B + 1 ints, written by the call, offsets[0] == 0).
 * pairs[2k], pairs[2k+1]: feature indices inside the two images, ascending in the first.
 * dist may be NULL. Returns offsets[B], -1 on failure.
 * Problem p returns exactly what cvMatchFeaturesNorm(&images[i], &images[j], cfg, norm, ...) returns: the same
 * count, pairs and dist bits (cfg NULL: ratio 0.8, no cross-check, no max distance). An empty image on
 * either side gives an empty slice; i == j is legal. Descriptors: uint8 only, one element type and one
 * width for all images. MCV_NORM_AUTO / MCV_NORM_HAMMING: Hamming, 1 - 64 bytes per row, fewer than 2^22
 * features per image; MCV_NORM_L2: byte SIFT, dim 1 - 512, cvMatchL2U8's exact integer definition. float32
 * descriptors fail the whole call (use cvMatchFeaturesNorm per pair), as do a bad image index, mixed
 * widths or element types, null arguments, negative sizes, DescriptorEntries not a multiple of
 * PointCount, an unknown norm and a total above maxPairs (the sum of the query images' PointCount over
 * the problems is always enough); every argument check runs before the device is touched.
 * Every image's descriptors go to the device once per call and are padded / shifted / normed once, however
 * many pairs the image is in. The call's kernel launches (at most 6), stream synchronisations (at most 2)
 * and copies (at most 5: the host arrays are staged through pinned buffers) do not depend on B or nImages. */
MCV_API int cvMatchFeaturesBatch(const DetectorResult* images, int nImages, const int* imagePairs, int B,
                                 const MatchConfig* cfg, int norm, int* pairs, float* dist, int maxPairs,
                                 int* offsets);

/* The same, then cvFindModelBatch (mcfg->model) on the matched keypoints of every pair (coordinates float
 * widened to double; offsets and rcfg passed through unchanged): the counts, mask bytes and nine doubles
 * are those of that call. models[B], mask: uint8[maxPairs] indexed like pairs, counts[B]; all required.
 * A pair with fewer matches than the sample size gets count 0, a zero model and a zero mask slice, and
 * mcvGetLastError() names the first such pair. Accepts the models and configurations cvFindModelBatch
 * accepts; the rest fails the whole call before the device is touched.
 * Returns the number of pairs with a model, -1 on failure. */
MCV_API int cvMatchAndFindModelBatch(const DetectorResult* images, int nImages, const int* imagePairs, int B,
                                     const MatchConfig* mcfg, int norm, const RansacConfig* rcfg,
                                     int* pairs, int maxPairs, int* offsets, mcvM33d* models, uint8_t* mask,
                                     int* counts);

/* Brute-force Hamming matcher (BFMatcher NORM_HAMMING, knn k = 2). q: [nq][bytesPerDesc],
 * t: [nt][bytesPerDesc] row-major bytes; bytesPerDesc in [1, 64]; nt < 2^22.
 * Outputs per query: best train index / distance and second best (idx2/dist2 may be NULL;
 * -1 / INT_MAX when nt < 2). Ties -> lowest train index. Returns nq, or -1 on failure. */
MCV_API int cvMatchHamming(const uint8_t* q, const int nq, const uint8_t* t, const int nt, const int bytesPerDesc,
                           int* idx, int* dist, int* idx2, int* dist2);

/* Brute-force L2 matcher (BFMatcher NORM_L2, knn k = 2) on fp32 descriptors [n][dim].
 * dist = sqrt of the squared distance (fp32). Returns nq, or -1 on failure. */
MCV_API int cvMatchL2(const float* q, const int nq, const float* t, const int nt, const int dim,
                      int* idx, float* dist, int* idx2, float* dist2);

/* Brute-force L2 matcher (BFMatcher NORM_L2, knn k = 2) on uint8 descriptors [n][dim] (byte SIFT),
 * exact on the int8 matrix cores: d^2 = sum (q_k - t_k)^2 as an integer, order (d^2, train index)
 * (ties -> lowest train index), dist = (float)sqrt((double)d^2). Every output equals cvMatchL2's on the
 * same bytes converted to float32 (idx2 / dist2 = -1 / +inf when nt < 2; idx = -1, dist = +inf when
 * nt == 0). dim in [1, 512]; nq, nt <= 2^24. Returns nq, or -1 on failure. */
MCV_API int cvMatchL2U8(const uint8_t* q, const int nq, const uint8_t* t, const int nt, const int dim,
                        int* idx, float* dist, int* idx2, float* dist2);

/* Multi-GPU forms of the matchers (query blocks Nq / D per GPU, train set
 * replicated), for a host that calls one synchronous export from one process like the reference's
 * P/Invoke layer (OpenCV.fs:339-382). The queries are split into deviceCount contiguous blocks (the
 * first nq % deviceCount one query longer), block k runs on visible device (current + k) mod count,
 * the train set is uploaded once and peer-copied over xGMI to the other devices, and every block's
 * outputs land in the caller's arrays at its offset. Results are identical to deviceCount = 1.
 * deviceCount in [1, 16]; the other arguments and the return are cvMatchHamming's / cvMatchL2's. */
MCV_API int cvMatchHammingMulti(const uint8_t* q, const int nq, const uint8_t* t, const int nt,
                                const int bytesPerDesc, const int deviceCount, int* idx, int* dist, int* idx2,
                                int* dist2);
MCV_API int cvMatchL2Multi(const float* q, const int nq, const float* t, const int nt, const int dim,
                           const int deviceCount, int* idx, float* dist, int* idx2, float* dist2);
MCV_API int cvMatchL2U8Multi(const uint8_t* q, const int nq, const uint8_t* t, const int nt, const int dim,
                             const int deviceCount, int* idx, float* dist, int* idx2, float* dist2);

/* Diagnostics of the exact L2 re-rank: queries the calling thread's last L2 match sent to the exact
 * full scan (near-ties the GEMM form cannot separate); synchronises that match's stream. */
MCV_API int mcvL2LastExactScans(void);
/* GEMM form of the calling thread's last L2 match: 16 = f16 split (every |x| < 2^15, dim <= 128),
 * 32 = f32; synchronises that match's stream. */
MCV_API int mcvL2LastGemmForm(void);
/* Train chunks per batch of 32 queued queries (T) in the exact scan of the calling thread's last L2
 * match, 0 when nothing was queued; T = 1 is the form in which the scan writes the final results
 * itself. Computed on the host by the kernels' own rule; synchronises that match's stream. */
MCV_API int mcvL2LastScanChunks(void);
/* Query tiles per wave (1 or 2) of the calling thread's last fp4 GEMM-form Hamming launch on the
 * current device; 0 when the last launch took the popcount form or none ran. */
MCV_API int mcvHammingLastQueryTiles(void);

/* Last error message of the calling thread ("" if none). */
MCV_API const char* mcvGetLastError(void);
/* Library / device info: number of visible HIP devices (0 when none), -1 on runtime error. */
MCV_API int mcvDeviceCount(void);
MCV_API const char* mcvVersion(void);
/* ABI revision of this header: 3 (round 3: MCV_FLAG_FUSED_ERROR moved from 4 to 64, bit 4 rejected,
 * MCV_FLAG_CV_SAMPLER added, RansacConfig unchanged at 48 bytes). */
#define MCV_ABI_VERSION 3
MCV_API int mcvAbiVersion(void);

/* CameraPose.findScaled — src/MiniCV/CameraPose.fs:39-134, the managed
 * O(N^2) scale hypothesize-and-verify, moved onto the GPU behind a new export. The F# wrapper keeps
 * its signature `findScaled inlierThreshold srcCam worldObservations pose` and passes the tuple
 * list as two arrays; it builds `scale bestScale pose` itself from *outScale.
 *   candidates: for observation i (list order), the pose scales s = -z / n from the dst0 frame
 *     (CameraPose.fs:103-117), s.X then s.Y; skipped when |n.X| or |n.Y| < 1e-5 (Fun.IsTiny);
 *   cost(s) = avgReprojectionError s (CameraPose.fs:71-87): mean of |project1 dstCam(s) w - obs|^2
 *     over the observations visible in dstCam(s) (Camera.fs:72-83), +inf if none;
 *   selection: first strictly smaller cost wins (CameraPose.fs:119-125).
 * inlierThreshold is accepted and unused, as in the reference (only the dead countInliers uses it).
 * Writes *outCost = best cost (+inf when no candidate improves on +inf) and *outScale = its scale
 * (0 then). Returns the number of candidate scales evaluated (2 per non-tiny observation), -1 on
 * failure. N == 0 returns 0 with *outCost = +inf, *outScale = 0 (the reference's empty-list case). */
typedef struct {             /* Camera.fs:7-14, F# record field order: 13 doubles */
    mcvV3d location;
    mcvV3d forward;
    mcvV3d up;
    mcvV3d right;
    mcvV2d focal;
} mcvCamera;
MCV_API int cvFindScaledPose(double inlierThreshold, const mcvCamera* srcCam, const mcvV3d* worldPoints,
                             const mcvV2d* observations, int N, const mcvM33d* rotation, const mcvV3d* translation,
                             double* outCost, double* outScale);
/* Per-candidate costs of cvFindScaledPose (test / analysis helper): scales[2N] and costs[2N] in
 * candidate order (slot 2i = s.X, 2i+1 = s.Y of observation i; a skipped observation has NaN scales
 * and +inf costs). Returns N, -1 on failure. */
MCV_API int cvFindScaledPoseCosts(const mcvCamera* srcCam, const mcvV3d* worldPoints, const mcvV2d* observations,
                                  int N, const mcvM33d* rotation, const mcvV3d* translation, double* scales,
                                  double* costs);

/* Track triangulation — Ray.intersection (src/MiniCV/Utilities.fs:100-165), the reference's managed
 * multi-view triangulator, for T independent tracks in one call. Tracks are a CSR: offsets[T + 1]
 * ints over the rays (or observations), offsets[0] == 0, non-decreasing, at most MCV_MAX_TRACK_LEN
 * per track. All arithmetic is fp64 in the managed evaluation order. Per track, rays in
 * input order:
 *   dedupe: ray j is dropped when an earlier ray i < j equals it on all six doubles (HashSet.ofList;
 *     the kept rays stay in input order, which fixes the order F# leaves unspecified);
 *   pairs i < j of the kept rays, lexicographic: kept when |cross(dir_i, dir_j)| > sin 2 deg (the
 *     double 0x1.1de58c9f7dc27p-5, the reference's asin test without the asin), both closest-point
 *     parameters are > 0 (getClosestTs) and the midpoint of the two closest points is finite;
 *   point = (sum of the kept midpoints, one sequential chain in pair order) / their number.
 * Writes points[t] and pairCounts[t] = the number of midpoints; a track without one (F# None) gets
 * pairCounts[t] = 0 and a point of three quiet NaNs. cvIntersectRays takes the rays as given
 * (directions of unit length, as the reference assumes); cvTriangulateTracks builds them with
 * Camera.unproject1 (Camera.fs:85-91) from cameras[cameraIdx[k]] and observations[k], and fills the
 * optional per-track statistics in avgReprojectionError's form (CameraPose.fs:77-92): visible[t] =
 * the track's observations (duplicates included) in which Camera.project1 sees the point, cost[t] =
 * the sequential sum of |project1 - obs|^2 over them divided by visible[t], +inf when none (always
 * for a track without a point). Either of cost / visible may be null.
 * Return the number of tracks with pairCounts > 0; T == 0 returns 0. Return -1 with a message and
 * write nothing on a null required pointer, negative T, bad offsets, a track over the cap, a camera
 * index outside [0, nCameras), or when no HIP device is visible. */
#define MCV_MAX_TRACK_LEN 4096
typedef struct { mcvV3d origin, direction; } mcvRay3d;   /* Aardvark Ray3d: 48 B */
MCV_API int cvIntersectRays(const mcvRay3d* rays, const int* offsets, int T, mcvV3d* points, int* pairCounts);
MCV_API int cvTriangulateTracks(const mcvCamera* cameras, int nCameras, const int* cameraIdx,
                                const mcvV2d* observations, const int* offsets, int T, mcvV3d* points,
                                int* pairCounts, double* cost, int* visible);

/* Track building — the step between cvMatchFeaturesBatch and cvTriangulateTracks: pairwise matches
 * (a CSR over image pairs) to tracks (a CSR of (camera, feature) over tracks), on the GPU.
 * Inputs, host arrays in cvMatchFeaturesBatch's conventions: featureCounts[nImages] (each >= 0),
 * imagePairs[2 B], pairs[2 offsets[B]] and offsets[B + 1] (offsets[0] == 0, non-decreasing) as
 * cvMatchFeaturesBatch writes them, mask[offsets[B]] (nullable: cvMatchAndFindModelBatch's inlier
 * bytes; null keeps every match, a non-zero byte keeps its match), minLength >= 2.
 *   nodes: feature f of image i is node base[i] + f, base = the exclusive prefix sum of featureCounts;
 *   edges: kept match k of problem p over images (i, j) = imagePairs[2p], imagePairs[2p + 1] joins
 *     (i, pairs[2k]) and (j, pairs[2k + 1]); duplicates are harmless, i == j is legal, a self-loop
 *     touches its node and joins nothing;
 *   components: the connected components over the nodes touched by at least one kept edge.
 * A component is dropped, and counted once, by the first rule that applies: oversize (more than
 * MCV_MAX_TRACK_LEN nodes), conflicts (two different nodes of one image), short (fewer than minLength
 * nodes). The others are the tracks, ordered by their smallest node, the observations of a track by
 * node (that is by image). The order of the problems and of the matches changes no output bit.
 * Writes trackOffsets[T + 1], cameraIdx[nObs] and featureIdx[nObs] (cameraIdx and trackOffsets go to
 * cvTriangulateTracks as they are; the caller gathers its observation coordinates with featureIdx),
 * and the optional trackOfFeature[base[nImages]] (the track of every node, -1 for a node in none) and
 * dropped[3] (oversize, conflicts, short). trackOffsets has room for maxTracks + 1 ints, cameraIdx and
 * featureIdx for maxObs; maxObs >= min(2 offsets[B], base[nImages]) and maxTracks >= maxObs / 2 are
 * always enough. Returns T (0 is a valid result, as is B == 0). Returns -1 with a message and writes
 * nothing to any output on a null required pointer, a negative nImages, B, maxTracks, maxObs or
 * feature count, offsets that do not start at 0 or that decrease, an image index outside [0, nImages),
 * a feature index outside its image (masked-out matches included), minLength < 2, more than 2^30
 * nodes or matches, a result that does not fit maxTracks / maxObs, or when no HIP device is visible.
 * Every argument check runs on the host before the device is touched; the outputs are written only
 * after the whole result is known. */
MCV_API int cvBuildTracks(const int* featureCounts, int nImages, const int* imagePairs, int B,
                          const int* pairs, const int* offsets, const uint8_t* mask, int minLength,
                          int* trackOffsets, int maxTracks, int* cameraIdx, int* featureIdx, int maxObs,
                          int* trackOfFeature, long long* dropped);

/* Bundle adjustment — the refinement after cvTriangulateTracks: Levenberg-Marquardt over the cameras
 * (rotation and location; the focal lengths stay) and the track points, minimising the reprojection
 * error of the whole scene on the GPU. Inputs in the layouts the pipeline hands out: the
 * mcvCamera array, cvBuildTracks' trackOffsets / cameraIdx CSR, the observations, the points of
 * cvTriangulateTracks, fixedCameras[nCameras] (nullable: a non-zero byte keeps that camera constant).
 *   residual: r = focal * pc.xy / pc.z - observation with pc = R (X - c), R = rows (right, up, forward);
 *     project1's [-1, 1] window is not applied;
 *   used set, fixed at the input parameters: an observation is used when its point is finite, pc.z > 0
 *     and r is finite; a track with fewer than two used observations is excluded and its point comes
 *     back bit for bit (the NaN points of cvTriangulateTracks included); a fixed camera and a camera
 *     without a used observation come back bit for bit;
 *   loss: squared error, or Huber with huberDelta > 0 (cost = the sum of rho over the used observations);
 *   step: the reduced camera system by matrix-free preconditioned conjugate gradients, damping
 *     d + lambda clamp(d, 1e-6, 1e32), lambda / 10 after an accepted and 10 lambda after a rejected trial.
 * summary->termination: 1 accepted decrease <= functionTolerance x cost, 2 maxIterations reached,
 * 3 cost == 0, 4 lambda over 1e12, 5 nothing to do. All arithmetic is fp64 in one defined order: the
 * outputs equal mcvHostBundleAdjust's bit for bit.
 * Returns the LM iterations run (trials, accepted or rejected; 0 is valid). Returns -1 with a message
 * and writes no output on a null required pointer, a negative count, bad offsets, a track over
 * MCV_MAX_TRACK_LEN, a camera index outside [0, nCameras), more than 2^26 observations, a non-finite
 * camera, a configuration value that is not positive and finite where one is needed, or when no HIP
 * device is visible. Every check runs on the host before the device is touched. */
typedef struct { int maxIterations;      /* LM iterations, default 50 */
                 int maxCgIterations;    /* per linear solve, default 64 */
                 double cgTolerance;     /* stop when r.z <= tol^2 * r0.z0, default 0.1 */
                 double initialLambda;   /* default 1e-3 */
                 double functionTolerance; /* default 1e-6 */
                 double huberDelta;      /* <= 0: plain squared error */ } mcvBaConfig;
typedef struct { double initialCost, finalCost; int iterations, accepted, rejected, cgIterations,
                 usedObservations, usedTracks, termination; } mcvBaSummary;
MCV_API int cvBundleAdjust(const mcvCamera* cameras, int nCameras, const uint8_t* fixedCameras /*nullable*/,
                           const int* cameraIdx, const mcvV2d* observations, const int* offsets, int T,
                           const mcvV3d* points, const mcvBaConfig* cfg /*nullable = defaults*/,
                           mcvCamera* outCameras, mcvV3d* outPoints, mcvBaSummary* summary /*nullable*/);

/* Bundle adjustment that also refines the focal lengths: cvBundleAdjust's cost, used set,
 * loss, damping, termination codes and arguments, minimised over the focal lengths as well.
 *   focalMode 0: the focal lengths stay; the call runs cvBundleAdjust's kernels and returns its bits;
 *             1: one scale s per group, focal <- focal (1 + s): the aspect fy / fx stays;
 *             2: fx and fy on their own, focal <- focal + (dfx, dfy).
 *   focalGroup[nCameras] (nullable: every camera is its own group): cameras with the same value, any value
 *     in [0, nCameras), share one focal length and must enter with bit-equal focal;
 *   fixedFocal[nCameras] (nullable): a non-zero byte keeps the whole group of that camera constant. It is
 *     independent of fixedCameras, which fixes rotation and location only: the focal length of a
 *     pose-fixed camera is refined unless fixedFocal says otherwise.
 * A group that is fixed or has no used observation is constant: its cameras' focal comes back bit for bit.
 * outCameras[j].focal carries the same bits for every camera of a group. A trial whose focal length is
 * not finite and positive is rejected like one that puts a point behind a camera.
 * summary->freeFocalGroups counts the groups that were refined (0 with focalMode 0). The outputs equal
 * mcvHostBundleAdjustFocal's bit for bit. Returns as cvBundleAdjust does; refused in addition, on the
 * host before the device is touched and with no output written: an unknown focalMode, a focalGroup
 * value outside [0, nCameras), unequal focal lengths within a group, and (focalMode 1, 2) a focal length
 * of a group not marked fixed that is not finite and positive. cfg == NULL: the defaults with focalMode 1. */
typedef struct { mcvBaConfig base; int focalMode; int pad; } mcvBaFocalConfig;
typedef struct { mcvBaSummary base; int freeFocalGroups; int pad; } mcvBaFocalSummary;
MCV_API int cvBundleAdjustFocal(const mcvCamera* cameras, int nCameras, const uint8_t* fixedCameras /*nullable*/,
                                const int* focalGroup /*nullable*/, const uint8_t* fixedFocal /*nullable*/,
                                const int* cameraIdx, const mcvV2d* observations, const int* offsets, int T,
                                const mcvV3d* points, const mcvBaFocalConfig* cfg /*nullable*/,
                                mcvCamera* outCameras, mcvV3d* outPoints, mcvBaFocalSummary* summary /*nullable*/);

/* Batched CameraPose.findScaled: P independent cvFindScaledPose problems in one call, each bit-identical
 * to its own single call; the launches, copies and the one synchronisation do not grow with P (DESIGN
 * §7j). The observation sets are a CSR: offsets[S + 1] ints, offsets[0] == 0, non-decreasing, over the
 * offsets[S] rows of worldPoints / observations. Problem p is (srcCams[p], rotations[p], translations[p])
 * over set setIdx[p]; a null setIdx means set p and needs S == P. Several problems may share a set (the
 * candidate poses of one pair do): it is uploaded and packed once.
 * Per problem: costs[p] / scales[p] = cvFindScaledPose's *outCost / *outScale (+inf and 0.0 for an empty
 * set and when no candidate has a finite cost), evaluated[p] (may be null) = its return value.
 * Returns the number of problems with a finite cost; P == 0 returns 0. Returns -1 with a message and
 * writes nothing on a null required pointer, a negative P or S, offsets that do not start at 0 or that
 * decrease, a setIdx entry outside [0, S), offsets[S] or the candidates of the call (2 x the rows of
 * every problem's set, summed) over 2^28, or when no HIP device is visible. Every argument check runs
 * before the device is touched. */
MCV_API int cvFindScaledPoseBatch(const mcvCamera* srcCams, const mcvM33d* rotations, const mcvV3d* translations,
                                  const int* setIdx, int P,
                                  const mcvV3d* worldPoints, const mcvV2d* observations, const int* offsets, int S,
                                  double* costs, double* scales, int* evaluated);
/* Per-candidate scales and costs of cvFindScaledPoseBatch (test / analysis helper): problem after
 * problem in cvFindScaledPoseCosts' layout, problem p's 2 N_p entries starting at 2 x the sum of N_q
 * over q < p (N_p = the rows of p's set). Same inputs and checks. Returns the sum of N_p, -1 on failure. */
MCV_API int cvFindScaledPoseBatchCosts(const mcvCamera* srcCams, const mcvM33d* rotations,
                                       const mcvV3d* translations, const int* setIdx, int P,
                                       const mcvV3d* worldPoints, const mcvV2d* observations, const int* offsets,
                                       int S, double* scales, double* costs);

/* ------------------------------------------------------------------------------------------
 * (3) Device-level API: device pointers, caller's stream (hipStream_t as void*), current device.
 *     Points on device are packed fp32 correspondences float4 {x, y, x', y'} (16 B each).
 * ---------------------------------------------------------------------------------------- */

typedef struct mcvRansacPlan_ mcvRansacPlan;

#define MCV_MODEL_HOMOGRAPHY   0
#define MCV_MODEL_FUNDAMENTAL  1
#define MCV_MODEL_ESSENTIAL    2   /* points: double4 {x1, y1, x2, y2} normalised (mcvPackEssential);
                                      hypothesis h owns model slots 10h .. 10h+9: keys, counts and
                                      indices below are slot indices for this model */
#define MCV_MODEL_PNP          3   /* points: PnpPoint {X, Y, Z, u, v, pad[3]} fp32 (mcvPackPnP); camera
                                      via mcvRansacPlanSetCamera; threshold in pixels; cfg->pnpKind
                                      picks the minimal solver; finalize writes model9 = {rvec[3],
                                      tvec[3], 0, 0, 0}, the inlier solve of cfg->pnpKind unless
                                      MCV_FLAG_NO_REFINE */
#define MCV_MODEL_AFFINE       4   /* estimateAffine2D: float4 points, 3-point samples; finalize writes
                                      model9 = the 2x3 matrix followed by 0 0 1 */
#define MCV_MODEL_SIMILARITY   5   /* estimateAffinePartial2D: 2-point samples, model9 as for AFFINE */

/* Workspace for problems up to maxN correspondences and maxHyps hypotheses per evaluate call. */
MCV_API mcvRansacPlan* mcvRansacPlanCreate(int model, int maxN, int64_t maxHyps);
MCV_API void mcvRansacPlanDestroy(mcvRansacPlan* plan);

/* Pack host AoS fp64 pairs into the device float4 layout (synchronous H2D on `stream`). */
MCV_API int mcvPackCorrespondences(const mcvV2d* a, const mcvV2d* b, int N, float* d_pts4, void* stream);
/* PnP model: upload image V2d[N] + world V3d[N] and pack them on the device (32 B each). */
MCV_API int mcvPackPnP(const mcvV2d* img, const mcvV3d* world, int N, void* d_pts, void* stream);
/* PnP plans: camera matrix (row-major 3x3; fx = K[0], fy = K[4], cx = K[2], cy = K[5]) and
 * distortion (k1, k2, p1, p2; NULL = none). */
MCV_API int mcvRansacPlanSetCamera(mcvRansacPlan* plan, const double* K9, const double* dist4);
/* Essential model: upload host pairs and normalise on the device into double4 (32 B each). */
MCV_API int mcvPackEssential(const mcvV2d* a, const mcvV2d* b, int N, double focal, mcvV2d pp, double* d_pts4,
                             void* stream);

/* Evaluate hypotheses [hypBegin, hypBegin + hypCount) against all N correspondences:
 * sample + minimal solve + inlier count, then reduce to the best packed key
 *   key = (count << 32) | (0xFFFFFFFF - hypIndex)     (0 when no hypothesis has >= m inliers)
 * written to d_key[0]; d_key[1] = first hypothesis index whose sampler failed (or INT64 max).
 * d_counts (optional, may be NULL): per-hypothesis status/count (int32, -1 no model, -2 no sample).
 * Asynchronous on `stream`, except with MCV_FLAG_CV_SAMPLER: OpenCV's subset stream is generated on
 * the host, so the call synchronises `stream` (to check the plan's table against N and the points'
 * fingerprint, and to rebuild it when hypBegin == 0 or either differs). The plan fingerprints the
 * points of every evaluated chunk; mcvRansacFinalize re-solves the winner when the buffer's content
 * changed since (a rewrite in place, same pointer and N). Returns 1 on successful launch, 0 on error. */
MCV_API int mcvRansacEvaluate(mcvRansacPlan* plan, const void* d_pts4, int N, const RansacConfig* cfg,
                              int64_t hypBegin, int64_t hypCount, uint64_t* d_key, int* d_counts, void* stream);

/* Recompute the best hypothesis' model (hypIndex), write the inlier mask (d_mask, uint8[N]),
 * optionally refit on the inliers + LM refine (per cfg->flags), model out to host `model9`.
 * Synchronises `stream`. Returns the inlier count, 0 on failure. */
MCV_API int mcvRansacFinalize(mcvRansacPlan* plan, const void* d_pts4, int N, const RansacConfig* cfg,
                              int64_t hypIndex, double* model9, uint8_t* d_mask, void* stream);

/* Sequential-RANSAC replay over per-hypothesis counts (host arrays), OpenCV semantics:
 * improvement iff count > max(best, m-1); niters <- RANSACUpdateNumIters(conf, 1-count/N, m, niters);
 * loop stops at iter >= niters or at the first sampler failure. State carried across chunks.
 * Returns 1 when the replay stopped inside this chunk (no more hypotheses needed), else 0. */
typedef struct {
    int64_t niters;      /* current iteration budget */
    int64_t bestIndex;   /* -1 if none */
    int32_t bestCount;
    int32_t stopped;
} mcvReplayState;
MCV_API void mcvReplayInit(mcvReplayState* st, int maxIters);
MCV_API int  mcvReplayChunk(mcvReplayState* st, const int* counts, int64_t hypBegin, int64_t hypCount,
                            int N, int modelPoints, double confidence, int fixedIters);
/* Multi-model hypotheses (essential: slotsPerHyp = 10): counts[h * slotsPerHyp + s], -2 at slot 0 =
 * sampler failure, -1 = no model; models of one hypothesis are tried in slot order, niters is
 * checked per hypothesis (RANSACPointSetRegistrator::run). bestIndex is the slot index. */
MCV_API int  mcvReplayChunkModels(mcvReplayState* st, const int* counts, int64_t hypBegin, int64_t hypCount,
                                  int slotsPerHyp, int N, int modelPoints, double confidence, int fixedIters);

/* Device-level matchers: d_q/d_t device arrays, outputs device arrays. Asynchronous on stream. */
MCV_API int mcvMatchHammingDevice(const uint8_t* d_q, int nq, const uint8_t* d_t, int nt, int bytesPerDesc,
                                  int* d_idx, int* d_dist, int* d_idx2, int* d_dist2, void* stream);
/* The same with the kernel form chosen explicitly: 0 = fp4 GEMM on the matrix cores (the default of
 * every other Hamming entry point), 1 = the XOR / popcount sweep. Identical results. */
MCV_API int mcvMatchHammingDeviceForm(const uint8_t* d_q, int nq, const uint8_t* d_t, int nt, int bytesPerDesc,
                                      int* d_idx, int* d_dist, int* d_idx2, int* d_dist2, int form, void* stream);
MCV_API int mcvMatchL2Device(const float* d_q, int nq, const float* d_t, int nt, int dim,
                             int* d_idx, float* d_dist, int* d_idx2, float* d_dist2, void* stream);
/* cvMatchL2U8 on device arrays (three launches, no host round trip). */
MCV_API int mcvMatchL2U8Device(const uint8_t* d_q, int nq, const uint8_t* d_t, int nt, int dim,
                               int* d_idx, float* d_dist, int* d_idx2, float* d_dist2, void* stream);

/* Device-level CameraPose.findScaled: d_world V3d[N], d_obs V2d[N] on the device. Synchronises
 * `stream`; same outputs and return value as cvFindScaledPose. */
MCV_API int mcvFindScaledPoseDevice(const mcvCamera* srcCam, const mcvV3d* d_world, const mcvV2d* d_obs, int N,
                                    const mcvM33d* rotation, const mcvV3d* translation, double* outCost,
                                    double* outScale, void* stream);

/* cvTriangulateTracks with every array (cameras and offsets included) on the device. Runs on the
 * null stream and synchronises it before returning; the argument checks run on the device first
 * (one extra synchronisation), so a bad call still writes nothing. cost / visible may be null. */
MCV_API int mcvTriangulateTracksDevice(const mcvCamera* d_cameras, int nCameras, const int* d_cameraIdx,
                                       const mcvV2d* d_observations, const int* d_offsets, int T,
                                       mcvV3d* d_points, int* d_pairCounts, double* d_cost, int* d_visible);

/* Opt-in kernel timing: HIP events recorded around the inlier-sweep launches on their stream.
 * mcvProfileRead returns the number of launches of `kernel` ("h_verify", "f_verify", "a_verify") and their
 * summed duration in ms (synchronises the recorded events). */
MCV_API void mcvProfileEnable(int on);
MCV_API void mcvProfileReset(void);
MCV_API int  mcvProfileRead(const char* kernel, double* total_ms);

/* ------------------------------------------------------------------------------------------
 * Test hooks: the host-compiled copy of the per-hypothesis code that the kernels run
 * (sampler + subset check + minimal solver + error), so CPU tests can check it against the
 * oracle bit for bit without a GPU. Never on a product path.
 * ---------------------------------------------------------------------------------------- */
#define MCV_HOST_FAST_MINIMAL 0x100   /* or-ed into mcvHostHypothesis' model: the elimination solver */
/* model MCV_MODEL_AFFINE / MCV_MODEL_SIMILARITY: model9 / modelf9 hold the 6 values of the 2x3 matrix
 * (the rest untouched), sampleIdx 3 / 2 indices. */
MCV_API int mcvHostHypothesis(int model, const float* pts4, int N, uint64_t seed, int64_t hyp,
                              double* model9, float* modelf9, int* sampleIdx);
/* Device self-test: the packed affine inlier sweep (mcv_a_verify_pk) on caller-supplied fp32 models
 * (6 floats each) over host float4 points; fused: 0 = op-by-op error, 1 = fused. counts[k] = inliers of
 * model k. Timed under mcvProfileEnable as "a_verify". Returns 1, 0 on failure. */
MCV_API int mcvTestAffineSweep(const float* pts4, int N, const float* models6, int nModels, float thr2, int fused,
                               int* counts);
/* Host twin of the affine-family refine: the LM solver of the product on the masked correspondences
 * (mask NULL: all) with sequential sums (point order) instead of the device's block order. model =
 * MCV_MODEL_AFFINE or MCV_MODEL_SIMILARITY; A6: in the start (2x3), out the refined matrix. Returns the
 * number of correspondences used, -1 on failure. */
MCV_API int mcvHostAffineRefine(int model, const float* pts4, int N, const uint8_t* mask, double* A6);
/* Device self-test: number of 32-bit patterns w where a reciprocal differs from 1.f/w (mode 0 =
 * rcp_exact; 1 = rcp_newton everywhere; 2 = rcp_newton + v_div_fixup; 3 = rcp_newton on its domain
 * |w| in [2^-126, 2^126) only; 4 = raw v_rcp_f32; 5 = rcp_exact_bounded on |w| < 2^126 and NaN). */
MCV_API long long mcvTestRcpExhaustive(int mode, uint32_t* firstMismatches16);
/* Device self-test: number of sampled (n, d), d in +-[2^-64, 2^64], where the unscaled fp64
 * division (rcp_f64_refined + div_f64_refined) differs from n / d (mode 0: 2^-900 <= |n| < 2^700;
 * 1: n = 1; 2: n = k d, |k| <= 1000; 3: d at the domain ends); first 16 (n, d) pairs returned.
 * Mode 4: sampled x in [1, 2] where the rotation's unscaled sqrt_f64_1to2 differs from sqrt (pairs (x, 0)). */
MCV_API long long mcvTestDivF64(int mode, unsigned long long seed, long long count, double* firstMismatches32);
/* Device self-test: run the homography inlier sweep on caller-supplied fp32 models (8 floats each);
 * fused: 0 = op-by-op error (scalar sweep), 1 = fused (scalar sweep), 2 = fused through the packed-f32
 * sweep, 3 = op-by-op through the certified division-free sweep (the default path: the form the
 * size rule picks), 4 = the certified sweep's packed-f32 VALU form, forced, 5 = its bf16 matrix-core
 * form, forced whatever the size. */
MCV_API int mcvTestHomographySweep(const float* pts4, int N, const float* models8, int nModels, float thr2, int fused,
                                   int* counts);
/* Device self-test: the affine forms W = h6 x + h7 y + 1, U = h0 x + h1 y + h2, V = h3 x + h4 y + h5 as
 * the bf16 matrix-core form of the certified sweep produces them (three-way bf16 split of every f32
 * operand, six products per variable, one v_mfma_f32_32x32x16_bf16 per form).
 * wuv[(k * N + i) * 3 + {0, 1, 2}] = W, U, V of model k at correspondence i. Returns 1, 0 on failure. */
MCV_API int mcvTestHMfmaWuv(const float* pts4, int N, const float* models8, int nModels, float* wuv);
/* The form of the certified homography sweep. mode 0: automatic (the size rule), 1: the packed-f32 VALU
 * kernel everywhere, 2: the bf16 matrix-core kernel in every launch and stage, 3: the matrix-core kernel
 * in the full-width launches and the VALU kernel in the survivor stages; any other mode leaves the
 * setting. Returns the previous mode, -1 on error. stats (may be NULL; 3 values), for the calling
 * thread's last certified homography sweep (evaluate or mcvTestHomographySweep), read after its stream
 * was synchronised: [0] the (32-point tile, hypothesis) rows the matrix-core kernel logged as undecided
 * (rows of slots it writes only), [1] the waves whose event list overflowed, [2] the waves with a model
 * outside the bound's domain (the slots of both kinds were recounted by the exact scalar sweep); all 0
 * when the sweep ran the VALU kernel only. Not thread-safe, and the plan of the last evaluate must
 * still exist and have been released, if at all, by the calling thread: tests only. */
MCV_API int mcvTestHMfma(int mode, long long* stats);
/* Device self-test: the LMedS rank kernel (lmeds.hip) on caller-supplied models: values[k] = the error
 * of rank `rank` (0-based, ascending; NaN last) of model k over pts4 (N float4 correspondences), NaN
 * when that element is a NaN. model MCV_MODEL_HOMOGRAPHY: 8 floats per model, errKind 0 = op-by-op,
 * 1 = fused error; MCV_MODEL_FUNDAMENTAL: 9 doubles per model, errKind = errorKind * 2 + unfused (0..3);
 * MCV_MODEL_AFFINE / MCV_MODEL_SIMILARITY: 6 floats per model, errKind 0 = op-by-op, 1 = fused.
 * Returns 1, 0 on failure. mcvHostErrorRank: the host twin (the same three radix passes, sequentially). */
MCV_API int mcvTestErrorRank(int model, const float* pts4, int N, const void* models, int nModels, int errKind,
                             int rank, float* values);
MCV_API int mcvHostErrorRank(int model, const float* pts4, int N, const void* models, int nModels, int errKind,
                             int rank, float* values);
/* Host twins of the essential path: hypothesis (double4 normalised points; E90 = 10 x 9; the reference's
 * solver, as the default GPU path) and the raw five-point solves (x1[5], y1[5], x2[5], y2[5] packed in
 * p20): mcvHostFivePoint = the opt-in replacement solver, mcvHostFivePointRef = the reference's.
 * Return the model count / status. */
MCV_API int mcvHostEssential(const double* pts4, int N, uint64_t seed, int64_t hyp, double* E90, int* sampleIdx);
/* mcvHostEssential with the opt-in replacement solver (MCV_FLAG_FAST_MINIMAL). */
MCV_API int mcvHostEssentialFast(const double* pts4, int N, uint64_t seed, int64_t hyp, double* E90, int* sampleIdx);
MCV_API int mcvHostFivePoint(const double* p20, double* E90);
/* Host build of the cvFivePoint export's own path (e_solve5_ref), same packing as mcvHostFivePoint. */
MCV_API int mcvHostFivePointRef(const double* p20, double* E90);
/* Host twin of one 7-point fundamental hypothesis (MCV_FLAG_SEVEN_POINT): F27 = up to 3 models,
 * idx7 = the accepted sample (may be NULL). Returns the model count or the kStatus code. */
MCV_API int mcvHostF7(const float* pts4, int N, uint64_t seed, int64_t hyp, double* F27, int* idx7);
MCV_API void mcvHostDecomposeEssential(const double* E9, double* R1, double* R2, double* t3);
/* Host twin of the real-root finder (Rolle brackets + Illinois) of sum c[k] x^k, deg <= 10;
 * fixed = 1 (deg == 4 only) runs the register-resident fixed-size form the AP3P quartic uses.
 * Writes the ascending roots, returns their count (-1 on bad arguments). */
MCV_API int mcvHostRealRoots(const double* c, int deg, int fixed, double* roots);
/* Host twins of the PnP path: one hypothesis on packed PnpPoint[N] (cam8 = fx, fy, cx, cy, k1, k2,
 * p1, p2), and the Rodrigues maps used by the LM refit. */
MCV_API int mcvHostPnP(const void* pts, int N, const double* cam8, uint64_t seed, int64_t hyp, double* R9, double* t3,
                       int* idx4);
/* mcvHostPnP with the opt-in real-root-finder AP3P quartic (MCV_FLAG_FAST_MINIMAL). */
MCV_API int mcvHostPnPFast(const void* pts, int N, const double* cam8, uint64_t seed, int64_t hyp, double* R9,
                           double* t3, int* idx4);
/* EPnP twins: a 5-point EPnP hypothesis (idx5: the sample), and epnp_solve_small<5> on given world
 * points pw15 (5 x 3) and pixel observations us10 (5 x 2), cam4 = fu, fv, uc, vc. */
MCV_API int mcvHostPnPEpnp(const void* pts, int N, const double* cam8, uint64_t seed, int64_t hyp, double* R9,
                           double* t3, int* idx5);
MCV_API void mcvHostEpnp5(const double* pw15, const double* us10, const double* cam4, double* R9, double* t3);
/* Device self-test: the PnP generate kernel's poses for hypotheses [hypBegin, hypBegin + hypCount) on
 * host PnpPoint[N] (kind: solverKind, EPnP kernel unless 2 / 5; | MCV_HOST_FAST_MINIMAL: the opt-in
 * real-root-finder AP3P quartic). poses12[h] = {R (9), t (3)},
 * status[h] = 1 or -1 / -2. Returns hypCount, -1 on failure. */
MCV_API int mcvTestPnpHypotheses(const float* pts, int N, const double* cam8, uint64_t seed, int64_t hypBegin,
                                 int hypCount, int kind, double* poses12, int* status);
/* Device self-test: the PnP inlier sweep on caller-supplied poses (poses12[h] = {R (9), t (3)}) over
 * host PnpPoint[N]; mode 0 = the certified packed-fp32 sweep (the default path), 1 = the all-fp64
 * sweep. counts[h] = inliers. Returns nPoses, -1 on failure. */
MCV_API int mcvTestPnpSweep(const float* pts, int N, const double* cam8, const double* poses12, int nPoses,
                            float thr2, int fused, int mode, int* counts);
/* Host twin of the certified PnP prefilter (pnp_pk.h) for one pose over host PnpPoint[N]: decision[i]
 * = 1 certified inlier, 0 certified outlier, -1 undecided; exact[i] = the fp64 test (pnp_error).
 * fused: bit 0 = the FMA-contracted error; bit 1 = the cheap tier alone (default: the cheap tier, then
 * the exact per-lane bound for what it leaves undecided: MCV_PNP_TIERS=2's order; the default sweep
 * runs the exact bound alone, whose decisions are a superset of the cheap tier's on its domain).
 * Returns the number of decided points whose decision differs from the exact test (must be 0). */
MCV_API int mcvHostPnpCert(const float* pts, int N, const double* cam8, const double* R9, const double* t3,
                           float thr2, int fused, int* decision, int* exact);
/* Host twin of the certified Sampson prefilter (sampson_pk.h) for one fp64 model F9 over host float4
 * points {x1, y1, x2, y2}: decision[i] = 1 certified inlier, 0 certified outlier, -1 undecided; exact[i]
 * = the fp64 Sampson test (kind 0 fused, 1 op-by-op). Returns the number of decided points whose decision
 * differs from the exact test (must be 0). */
MCV_API int mcvHostSampsonCert(const float* pts4, int N, const double* F9, float thr2, int kind, int* decision,
                               int* exact);
/* Host build of solveAp3p's computation (mu3 / mv3 pixels, W9 = 3 world points), R36 / t12 out. */
MCV_API int mcvHostSolveAp3p(const double* mu3, const double* mv3, const double* W9, double inv_fx, double inv_fy,
                             double cx_fx, double cy_fy, double* R36, double* t12);
/* Host twin of cvSolvePnP kind 6 (SQPnP) on double img (N x 2) / world (N x 3), cam8 as above: the
 * computeOmega sums in the device passes' block order, then the same host solve. R9 / t3 = the first
 * solution; returns the solution count, 0 (none), or -1 / -2 / -3 (computeOmega's assertions). */
MCV_API int mcvHostSqpnp(const double* img, const double* world, int N, const double* cam8, double* R9, double* t3);
MCV_API void mcvHostRodrigues(const double* r, double* R, double* dR27);
MCV_API void mcvHostRodriguesInv(const double* R, double* r);
/* OpenCV's sample stream (MCV_FLAG_CV_SAMPLER) on the host: rows [0, rows) of m indices each for the
 * model family (homography / fundamental / affine: pts4 = the float4 points their checkSubset reads;
 * essential / PnP / similarity: no check, pts4 may be NULL; m in 2, 3, 4, 5, 7, 8). Rows from the first failed getSubset on are -1. Returns the number
 * of accepted rows, -1 on bad arguments. */
MCV_API int64_t mcvCvSubsets(int model, int m, const float* pts4, int N, int64_t rows, int* out);
/* glibc_math.h's restatements over arrays: fn 0 cbrt(a), 1 hypot(a, b), 2 the real part of clog(a + i b),
 * 3 a^2 + b^2 - 1 (glibc's __x2y2m1), 4 exp(a), 5 log(a), 6 log1p(a), 7 cos(a), 8 atan2(a, b) — glibc
 * 2.35's x86_64 (FMA multiarch) code paths, restated so the device computes AP3P's complex cube root
 * bit-identically to the reference's std::pow. Returns n, -1 on bad arguments. */
MCV_API int mcvHostGlibcMath(int fn, const double* a, const double* b, int n, double* out);
/* The plan guards' fingerprint (mcv_common.h fp_term summed over the 32-bit words) of a host buffer:
 * the device kernel gives the same value for the same bytes. */
MCV_API uint64_t mcvHostFingerprint(const void* buf, size_t bytes);
/* The device kernel's fingerprint of a device buffer into d_out[0] (synchronous). Returns 1, 0 on error. */
MCV_API int mcvTestFingerprint(const void* d_buf, size_t bytes, uint64_t* d_out);
/* Round 6: the homography generate's split eigen-solve logs at most `cap` rotations per hypothesis
 * (default and maximum 192; a cfg3 LtL takes 110-157); a hypothesis needing more is solved again by
 * the one-pass kernel. Lowering the cap sends lanes down that path (tests). Returns the previous cap. */
MCV_API int mcvTestEigLogCap(int cap);
/* The homography sweep's self-pruning stages (key-only evaluations: mcvRansacEvaluate with d_counts ==
 * NULL, fixed-iteration cvFindHomography). mode 0: automatic (large calls only), 1: staged whatever
 * the call's size (it still switches itself off without a candidate, on a sampler failure, or when
 * the first boundary is too late to pay), 2: never; any other mode leaves the setting. Returns the
 * previous mode, -1 on error. stats (may be NULL; 16 values), for the calling thread's last
 * homography evaluate, read after its stream was synchronised: [0] 0 = the stages pruned, 1 = no
 * candidate, 2 = sampler failure in the chunk, 3 = first boundary too late, 4 = forced off (mode 2),
 * 5 = the call did not qualify, -1 = no evaluate yet; [1] B, the candidate's full count; [2] the
 * number of stages (4, or 5 where the per-cell bound's second pass runs: the plan then has the half boundary,
 * stage 1 in two launches);
 * [3..9] the stage boundaries in points (stage s sweeps [3 + s], [4 + s]);
 * [10..15] the slots alive entering each stage ([10]: the slots stage 0 swept, fewer than the chunk's where
 * stage 0 ran on a leading subset, see mcvTestHStage0Slots; [4] then reads 0). Not thread-safe: tests only. */
MCV_API int mcvTestHStaging(int mode, long long* stats);
/* The slots stage 0 of the staged homography sweep covers where the per-cell bound runs. Stage 0 only names the
 * candidate, so it may sweep its prefix for a leading subset of the chunk's slots (into a scratch buffer); stage 1
 * then runs the bound's list from point 0. slots 0: automatic (max(2^14, hypotheses / 16) from 2^18 hypotheses,
 * every slot below), > 0: that many at any size (every slot where the chunk has no more), -1: leaves the setting.
 * Returns the previous value, -1 on error. With a subset, mcvTestHStaging's stats[10] (alive[0]) is the number of
 * slots stage 0 swept, not the chunk's, and stats[4] (the boundary stage 1 starts at) reads 0. Not thread-safe:
 * tests only. */
MCV_API int mcvTestHStage0Slots(int slots);
/* The second pass of the per-cell bound (the candidate-relative test and the per-slot points-left). mode 0: where
 * the rule or mcvTestHCellMode's mode 1 engages it, 2: never (the box pass alone; the stages' survivor tests then
 * use the points not yet processed, and the plan has no half boundary); any other mode leaves the setting. Returns
 * the previous mode, -1 on error. It exists because mcvTestHCellMode's mode 1 forces both passes: the box pass
 * alone otherwise runs only under the automatic rule, from 2^31 (hypothesis, correspondence) evaluations, which no
 * test can afford to check against the oracle. Not thread-safe: tests only. */
MCV_API int mcvTestHCellSecondPass(int mode);
/* The survivor lists of the staged homography sweep as its kernels push them (one atomic per block), on given data:
 * the per-cell bound's box pass with the second pass behind it, the second pass, and two compactions. models8:
 * nModels x 8 floats; cand8: the candidate's model; B: its count; counts (nModels ints): each slot's count so far
 * (negative: a status, never listed); boundPairs: the boundary the compactions test at, in pairs of correspondences.
 * lists (4 x nModels ints) and lens (4 ints): [0] the slots the box pass hands to the second pass, [1] the list of
 * stage 1 (what the box pass keeps outright, then what the second pass keeps), [2] the compaction of [1] with the
 * per-slot points-left, [3] a compaction over every slot with the points not yet processed. Lists are in any order;
 * entries beyond a list's length read -1. Returns 1, 0 on error. Tests only. */
MCV_API int mcvTestHListPush(const float* pts4, int N, const float* cand8, const float* models8, int nModels,
                             float thr2, int B, int G, int Gs, int boundPairs, const int* counts, int* lists,
                             int* lens);
/* The stage plan of the staged homography sweep for N correspondences, computed on the host by the function the
 * planner kernel runs (no device is touched). candidate: stage 0 named one (its full count is B); failure: the
 * chunk holds a sampler failure; cellBound 0: no per-cell bound, 1: its box pass alone (a shorter stage 0), 2: with
 * its second pass, which puts the half boundary in the middle of stage 1's range; subset: stage 0 swept a leading
 * subset (only with cellBound), so stage 1 starts at point 0. out (10 ints): [0] the reason as mcvTestHStaging's
 * stats[0] (0 = the stages prune), [1] the number of stages, [2] stage 0's range in pairs of correspondences,
 * [3..9] the stage boundaries in pairs (stage s sweeps the pairs [3 + s], [4 + s]; the last boundary is
 * (N + 1) / 2). Returns the number of stages, -1 on error. */
MCV_API int mcvHostHStagePlan(int N, int candidate, int failure, int B, int cellBound, int subset, int* out);
/* The per-cell inlier upper bound that drops hypotheses before stage 1 of the staged homography sweep.
 * mode 0: automatic (where the staged sweep's own size rule holds, from 20000 correspondences; its second pass,
 * the candidate-relative test and the per-slot points-left of the later compactions, from 35000), 1: both
 * passes whenever the sweep is staged, 2: never;
 * any other mode leaves the setting. G, Gs: the 4-D grid of the points the candidate rejects and the 2-D grid
 * of its inliers (1..6 and 1..24; 0 leaves them; defaults 4 and 12). Returns the previous mode, -1 on error.
 * stats (may be NULL; 6 values), for the calling thread's last homography evaluate, read after its stream was
 * synchronised: [0] 1 = the bound ran, 0 = it did not; [1] non-empty cells; [2] slots alive after the bound
 * (entering stage 1); [3] cell slots (G^4 + Gs^2); [4] G; [5] Gs. Not thread-safe: tests only. */
MCV_API int mcvTestHCellMode(int mode, int G, int Gs, long long* stats);
/* The cell build and the bound on caller-supplied data: pts4 (N float4 correspondences), the candidate's
 * model cand8, nModels models (8 floats each), the threshold and B. device 1: the kernels of the staged
 * sweep; 0: their host twin (the same header, no device needed). Outputs: cellId[N]; boxes[8 cells] = min /
 * max of x, y, x', y' per cell and sizes[cells] (cells = G^4 + Gs^2; an empty cell's box is NaN); ub[nModels]
 * = the upper bound of each model's inlier count; bits[nModels * ceil(cells / 32)] = the cells certified as
 * all-outlier (bit c & 31 of word c >> 5); *alive = the models with ub >= B. Returns 1, 0 on failure. */
MCV_API int mcvTestHCellBound(const float* pts4, int N, const float* cand8, const float* models8, int nModels,
                              float thr2, int B, int G, int Gs, int device, int* cellId, float* boxes, int* sizes,
                              int* ub, unsigned int* bits, int* alive);
/* The bound's second pass on caller-supplied data: the union of the box test above and the candidate-relative
 * test (cells of the candidate's inliers, index >= G^4), arguments as for mcvTestHCellBound. bounds[nBounds]
 * (1..4 of them): stage boundaries in pairs of points, each within 0..(N + 1) / 2; boundary b stands for the
 * first min(2 b, N) correspondences. Outputs: cellId[N]; ub[nModels]; bits as above, of the union test;
 * left[j * nModels + k] = the correspondences of model k's uncertified cells with index >= min(2 bounds[j], N);
 * *alive = the models with ub >= B. Returns 1, 0 on failure. */
MCV_API int mcvTestHCellRel(const float* pts4, int N, const float* cand8, const float* models8, int nModels,
                            float thr2, int B, int G, int Gs, const int* bounds, int nBounds, int device,
                            int* cellId, int* ub, unsigned int* bits, int* left, int* alive);
/* The certified fp32 prefilter in front of the box test of both bound passes. For one (model, cell) it answers
 * certified, not certified or undecided; undecided pairs run the fp64 box test, and a decided verdict always
 * equals the fp64 test's, so every output of the bound is the same with the prefilter on or off. mode 0:
 * automatic (on), 1: off (fp64 alone); any other mode leaves the setting. It applies to the staged sweep and to
 * mcvTestHCellBound / mcvTestHCellRel, device and host twin. Returns the previous mode, -1 on error. stats (may be
 * NULL; 2 values), for the calling thread's last staged evaluate with the bound (read after its stream was
 * synchronised) or call of one of those two hooks: [0] the (model, cell) tests the prefilter decided, [1] those it
 * left to fp64 (all of them with the prefilter off); lanes without a model are not counted. A staged evaluate
 * counts only after the first call of this hook (the counters cost atomics). Not thread-safe: tests only. */
MCV_API int mcvTestHCellPre(int mode, long long* stats);
/* The homography generate's certified one-row pass 2. Where an evaluate hands out only the chunk's key (op-by-op
 * error, eigen solver), pass 2 of the split generate replays one row of V from the rotation log in reverse, bounds
 * its distance to the row of the exact replay, and keeps the fp32 model only where that bound proves it to be the
 * exact path's, bit for bit; every other lane runs the exact pass 2. Models, statuses, keys and finalize results
 * are the same either way. mode 0: automatic (chunks of at least 2^14 hypotheses), 1: wherever it applies, 2:
 * never, 3: as 1 with the bound multiplied by 2^40, so that no lane is decided and every one takes the fallback;
 * any other mode leaves the setting. Returns the previous mode, -1 on error. stats (may be NULL; 2 values), for the
 * calling thread's last homography generate (read after its stream was synchronised): [0] lanes decided, [1] lanes
 * left to the exact pass or the log-overflow kernel; both 0 where the pass did not run. Not thread-safe: tests only. */
MCV_API int mcvTestHGenRow(int mode, long long* stats);
/* Device self-test: the split generate alone on host float4 points, hypotheses [hypBegin, hypBegin + hypCount).
 * table (may be NULL): a sample table, 4 indices per hypothesis from hypothesis 0 (no subset check), instead of
 * the seeded stream. row 0: the exact pass 2; 1: the certified one-row pass; 2: that with the bound times 2^40.
 * models8[8 hypCount] and counts[hypCount] receive the fp32 models and the statuses as the generate leaves them;
 * stats as for mcvTestHGenRow. Honours mcvTestEigLogCap. Returns 1, 0 on failure. */
MCV_API int mcvTestHGenerate(const float* pts4, int N, uint64_t seed, const int* table, int64_t hypBegin, int hypCount,
                             int row, float* models8, int* counts, long long* stats);
/* Host twin of the one-row pass beside the exact solve, arguments as above (errHuge: the bound times 2^40). Per
 * hypothesis: modelsFwd8 / statusFwd = the exact path's fp32 model and status; decided = 1 where the one-row pass
 * certifies its model, then in modelsRow8; err = its bound on |y - v|_inf (the reverse row against the forward
 * replay's row of the same log) and dev = that distance as measured. Returns 1, 0 on failure. */
MCV_API int mcvHostHGenRow(const float* pts4, int N, uint64_t seed, const int* table, int64_t hypBegin, int hypCount,
                           int errHuge, float* modelsRow8, float* modelsFwd8, int* statusFwd, int* decided,
                           double* err, double* dev);
/* The prefilter's verdict on caller-supplied data, arguments as for mcvTestHCellBound (B is not read).
 * verdicts[k * cells + c] for model k and cell c: 0 not certified, 1 certified, 2 undecided; an empty cell is
 * undecided or not certified, never certified. Returns 1, 0 on failure. */
MCV_API int mcvTestHCellPreVerdicts(const float* pts4, int N, const float* cand8, const float* models8, int nModels,
                                    float thr2, int B, int G, int Gs, int device, int* cellId, float* boxes,
                                    int* sizes, unsigned char* verdicts);
/* cvFindModelBatch's index arithmetic, as the export itself computes it (no device). Problems with more
 * than m (the sample size) correspondences run on the device and are numbered in order (d = 0, 1, ...).
 * desc4[4 p ..]: point offset (= offsets[p]: float4 points, no padding), N, slot offset (d * per, 64-bit;
 * -1 for a problem not on the device), sampler row offset (d * max(maxIters, 1); -1 likewise).
 * info4: device problems D, per = hypotheses per problem per round = clamp(cap / D, 1, max(maxIters, 1)),
 * rounds = ceil(max(maxIters, 1) / per), slots of a full round D * per. cap <= 0: the export's own cap
 * (2^21 slots). Returns D, -1 on a bad argument. */
MCV_API int mcvHostBatchLayout(const int* offsets, int B, int m, int maxIters, long long cap, long long* desc4,
                               long long* info4);
/* The plan of one hypothesis round of the RANSAC batches (cvFindModelBatch, the essential and the PnP batches), as
 * their shared round driver computes it (no device). Device problem d has the points [ptOff[d], ptOff[d] + N[d]),
 * the sampler rows from rowOff[d] (NULL: 0) and the replay state niters[d] / stopped[d]; active[nActive]: the
 * ascending device indices still in the search. The round holds the hypotheses [begin, begin + size) of every
 * active problem that is not stopped and has niters > begin; they are compacted in order. desc6[6 j ..] of entry
 * j: point offset, N, hypBegin = begin, hypCount = min(niters - begin, size), slot offset = j * stride (stride =
 * the round's largest hypCount), row offset; activeOut[j]: its device index (both with room for nActive entries);
 * info2 = {n, stride}. Returns n, -1 on a null array, nActive outside [0, D], begin outside [0, 2^31), size
 * outside [1, 2^31) or an active list that is not ascending within [0, D). */
MCV_API int mcvHostBatchRound(const int* ptOff, const int* N, const long long* rowOff, const long long* niters,
                              const int* stopped, int D, const int* active, int nActive, long long begin,
                              long long size, long long* desc6, int* activeOut, long long* info2);
/* The slot cap of cvFindModelBatch's rounds (cap <= 0: back to the default). Returns the previous cap.
 * Not thread-safe: tests only. */
MCV_API long long mcvTestBatchCap(long long cap);
/* The calling thread's last cvFindModelBatch: stats16[0] kernel launches, [1] stream synchronisations,
 * [2] hypothesis rounds, [3] Levenberg-Marquardt rounds, [4] problems routed through the single export,
 * [5] B (the launches and synchronisations of routed problems are the single export's and not counted),
 * [6] host microseconds spent converting the points to float4, [7] host microseconds spent drawing
 * OpenCV's sample tables (MCV_FLAG_CV_SAMPLER; 0 with the Philox sampler), [8] the problems summed over the
 * hypothesis rounds they ran in, [9] the host <-> device copies enqueued (memsets are not counted; every RANSAC
 * batch family counts [8] and [9] the same way). Returns 1. */
MCV_API int mcvTestBatchStats(long long* stats16);
/* Device self-test: the batched inlier sweep (mcv_batch_sweep) on caller-supplied models. pts4: the
 * segmented float4 points, problem p owning [offsets[p], offsets[p+1]); its models are
 * [modelOffsets[p], modelOffsets[p+1]) of `models` (homography: 8 floats each, affine / similarity: 6
 * floats, fundamental: 9 doubles). errKind: fundamental 0..3 (errorKind * 2 + unfused), else 0 (op-by-op).
 * counts[k] = inliers of model k over its problem's points. Returns 1, 0 on failure. */
MCV_API int mcvTestBatchSweep(int model, const float* pts4, const int* offsets, int B, const void* models,
                              const int* modelOffsets, float thr2, int errKind, int* counts);
/* The essential batches (cvFindEssentialMatBatch, cvRecoverPoseBatch) share the hooks above: their layout is
 * mcvHostBatchLayout with m = 5 and their own default cap of 2^18 hypotheses per round (pass it: cap <= 0
 * means the 2-D default); mcvTestBatchCap overrides their cap too (a cap other than the 2-D default holds for
 * both; cap <= 0 restores both defaults); mcvTestBatchStats reports the calling thread's last batch call of
 * either kind ([3] is 0, [6] the host microseconds staging the raw points and the descriptors, [8] the
 * problems summed over the hypothesis rounds they ran in: below [2] x the device problems once a problem has
 * stopped early and dropped out of the later rounds).
 * Device self-test: the batched essential sweep (mcv_batch_e_sweep) on caller-supplied models. pts4d: the
 * segmented double4 normalised points, problem p owning [offsets[p], offsets[p+1]); its models are
 * [modelOffsets[p], modelOffsets[p+1]) of models9 (9 doubles each, row-major E); thr2[B]: one threshold per
 * problem; kind: 0 fused / 1 op-by-op Sampson error. counts[k] = points of model k's problem with
 * f_error <= thr2. Returns 1, 0 on failure. */
MCV_API int mcvTestBatchSweepE(const double* pts4d, const int* offsets, int B, const double* models9,
                               const int* modelOffsets, const float* thr2, int kind, int* counts);
/* cvSolvePnPRansacBatch shares the hooks above as well: its layout is mcvHostBatchLayout with m = 4 (P3P /
 * AP3P) or 5 (the other kinds) and its own default cap of 2^18 hypotheses per round; mcvTestBatchCap overrides
 * it like the essential cap; mcvTestBatchStats reports [3] the lockstep LM steps (at most 21), [6] the host
 * microseconds staging the raw points and cameras, [8] and [9] as above.
 * Device self-test: the batched PnP sweep (mcv_batch_pnp_sweep) on caller-supplied poses. pts8: the segmented
 * PnpPoint rows (8 floats: X, Y, Z, u, v, 3 pad), problem p owning [offsets[p], offsets[p+1]); cam8: 8 doubles
 * per problem (fx, fy, cx, cy, k1, k2, p1, p2); its poses are [poseOffsets[p], poseOffsets[p+1]) of poses12
 * (R row-major, then t). counts[k] = points of pose k's problem with pnp_error <= thr2. Returns 1, 0 on failure. */
MCV_API int mcvTestBatchSweepPnp(const float* pts8, const int* offsets, int B, const double* cam8 /* 8 per problem */,
                                 const double* poses12, const int* poseOffsets, float thr2, int* counts);
/* The index arithmetic of cvRefinePnPBatch, as the export computes it (no device): counts[B] = the selected rows
 * of every problem (mask NULL: all of its rows; any non-zero byte selects), compOff[B + 1] = their exclusive
 * prefix sum, problem p's place in the compact array the reductions run over. Returns the largest count, -1
 * on a null offsets / counts / compOff, a negative B or bad offsets. mcvTestBatchStats reports
 * cvRefinePnPBatch and cvSolvePnPRansacRefineBatch like cvSolvePnPRansacBatch: [3] the lockstep steps of the
 * call (the RANSAC tail's and the refine's together for the fused call), [9] the copies. */
MCV_API int mcvHostRefinePnPBatchLayout(const int* offsets, int B, const uint8_t* mask, int* counts, int* compOff);
/* Device self-test: cvRefinePnPLM (refineKind 0) / cvRefinePnPVVS (1) with a byte mask applied in place: the
 * reductions skip the unselected rows of the whole array (the order of the RANSAC tail's LM) instead of running
 * over gathered rows. cvRefinePnPBatch's tests tell the two orders apart with it. Returns 1, 0 on failure. */
MCV_API int mcvTestRefinePnPMasked(const mcvV2d* imgPoints, const mcvV3d* worldPoints, int N, const mcvM33d* K,
                                   const double* distortionCoeffs, const uint8_t* mask, int refineKind, mcvV3d* tVec,
                                   mcvV3d* rVec);
/* The index arithmetic of cvMatchFeaturesBatch, as the export computes it (no device). featureCounts[nImages],
 * imagePairs[2 B]; norm picks the kernel form (MCV_NORM_L2: int8 matrix cores, else XOR / popcount).
 * Directed problem d < B is pair d (query image first); with crossCheck, d in [B, 2B) is pair d - B reversed.
 * problems5[5 d ..] (may be NULL): query image, train image, nq, nt, output offset (the queries of the
 * problems before d). info4: directed problems D, query rows per workgroup, workgroups G, queries of the B
 * forward problems. wgTable (may be NULL; room for maxWorkgroups entries): G x (problem, query tile), the
 * problems in descending nt (ties: ascending d), each problem's tiles ascending; a problem with nq == 0
 * has none. Returns G, -1 on a bad argument. */
MCV_API int mcvHostMatchBatchLayout(const int* featureCounts, int nImages, const int* imagePairs, int B,
                                    int crossCheck, int norm, int* problems5, int* info4, int* wgTable,
                                    int maxWorkgroups);
/* The calling thread's last cvMatchFeaturesBatch / cvMatchAndFindModelBatch (matching part) /
 * mcvTestMatchBatchKnn: stats8[0] kernel launches, [1] stream synchronisations, [2] directed problems,
 * [3] workgroups of the knn launch, [4] host <-> device copies. Returns 1. */
MCV_API int mcvTestMatchBatchStats(long long* stats8);
/* Device self-test: the batched knn-2 kernel alone, before any filter. rows: the images' descriptor rows
 * one image after the other ([sum featureCounts][dim] uint8); directedPairs[2 D]: (query image, train
 * image) per directed problem; norm MCV_NORM_HAMMING or MCV_NORM_L2. Outputs: problem after problem, nq
 * entries each; dist / dist2: int32 for Hamming (missing place: -1 / INT_MAX), float for L2 (-1 / +inf).
 * Returns the number of entries, -1 on failure. */
MCV_API int mcvTestMatchBatchKnn(const uint8_t* rows, const int* featureCounts, int nImages, int dim,
                                 const int* directedPairs, int D, int norm, int* idx, void* dist, int* idx2,
                                 void* dist2);
MCV_API void mcvHostPhilox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                           uint32_t* out4);
/* Host twin of CameraPose.findScaled: the same candidates and costs as cvFindScaledPoseCosts,
 * computed by the host-compiled kernel code with the reference's sequential sums (list order). */
MCV_API int mcvHostScaledCosts(const mcvCamera* srcCam, const mcvV3d* worldPoints, const mcvV2d* observations, int N,
                               const mcvM33d* rotation, const mcvV3d* translation, double* scales, double* costs);
/* Host twins of cvIntersectRays / cvTriangulateTracks: the same arguments, checks, outputs and
 * return value, computed sequentially by the host-compiled kernel arithmetic (hyp_rays.h). No GPU. */
MCV_API int mcvHostIntersectRays(const mcvRay3d* rays, const int* offsets, int T, mcvV3d* points, int* pairCounts);
MCV_API int mcvHostTriangulateTracks(const mcvCamera* cameras, int nCameras, const int* cameraIdx,
                                     const mcvV2d* observations, const int* offsets, int T, mcvV3d* points,
                                     int* pairCounts, double* cost, int* visible);
/* Counters of the calling thread's last cvIntersectRays / cvTriangulateTracks / mcvTriangulateTracksDevice
 * call that reached the device: stats8 = {kernel launches, stream synchronisations, host<->device
 * copies, memsets, short tracks (at most 16 rays), long tracks, 0, 0}. Returns 0. */
MCV_API int mcvTestTriangulateStats(long long* stats8);
/* Host twin of cvFindScaledPoseBatch: the same arguments, checks, outputs and return value, computed
 * problem after problem by the host-compiled code behind mcvHostScaledCosts. No GPU. */
MCV_API int mcvHostFindScaledPoseBatch(const mcvCamera* srcCams, const mcvM33d* rotations,
                                       const mcvV3d* translations, const int* setIdx, int P,
                                       const mcvV3d* worldPoints, const mcvV2d* observations, const int* offsets,
                                       int S, double* costs, double* scales, int* evaluated);
/* Counters of the calling thread's last cvFindScaledPoseBatch / cvFindScaledPoseBatchCosts call that
 * reached the device: stats8 = {kernel launches, stream synchronisations, host<->device copies, memsets,
 * problems on the device (those over a non-empty set), candidate tiles (blocks of 64 candidates of the
 * sweep), 0, 0}. Returns 0. */
MCV_API int mcvTestScaledBatchStats(long long* stats8);
/* Host twin of cvBuildTracks: the same arguments, checks, outputs and return value, computed by a
 * sequential union-find (union by smaller id). No GPU. */
MCV_API int mcvHostBuildTracks(const int* featureCounts, int nImages, const int* imagePairs, int B,
                               const int* pairs, const int* offsets, const uint8_t* mask, int minLength,
                               int* trackOffsets, int maxTracks, int* cameraIdx, int* featureIdx, int maxObs,
                               int* trackOfFeature, long long* dropped);
/* Counters of the calling thread's last cvBuildTracks call that passed its checks: stats8 = {kernel
 * launches, stream synchronisations, host<->device copies, memsets, candidate components (those that
 * were sorted), of them the long ones (more than 32 nodes: one workgroup each), kept matches, 0}; all
 * are 0 for a call without a kept match, which launches nothing. Returns 0. */
MCV_API int mcvTestTracksStats(long long* stats8);
/* Host twin of cvDetectFeatures: the same arguments, checks and result (freed with cvFreeFeatures),
 * computed sequentially by the host-compiled sample arithmetic (sift_math.h). No GPU. */
MCV_API DetectorResult* mcvHostDetectFeatures(char* data, int width, int height, int channels, int mode,
                                              void* config);
/* What the calling thread's last cvDetectFeatures call enqueued and found: stats8 = {kernel launches,
 * stream synchronisations, host<->device copies, memsets, extremum candidates, refined keypoints,
 * keypoints with orientations (before duplicates and FeatureCount), keypoints returned}. The
 * descriptor kernel has one path for every radius, so there is no short / long count. Returns 0. */
MCV_API int mcvTestSiftStats(long long* stats8);
/* A stage of the calling thread's last finished cvDetectFeatures call, read from that thread's
 * workspace on the current device. what 0: the Gaussian pyramid, floats, octave by octave, image by
 * image (OctaveLayers + 3 per octave), row-major; *count = the floats. what 1: the extremum
 * candidates, int[4] records (octave, layer, row, column) in arrival order, which differs from run to
 * run; *count = the records. One device-to-host copy, no launch; mcvTestSiftStats reads the same after
 * it. Returns 0, or -1 with an error for an unknown `what`, a null argument, a capBytes below the
 * stage's size, or a thread without a finished call on the current device. */
MCV_API int mcvTestSiftStage(int what, void* out, long long capBytes, long long* count);
/* stats8 of the calling thread's last cvDetectFeaturesBatch: {launches, synchronisations, copies, memsets,
 * candidates, refined, oriented, returned}, the last four summed over the images. */
MCV_API int mcvTestSiftBatchStats(long long* stats8);
/* The plan of a batch, on the host alone (no device): out8 = {maxOctaves, launches, synchronisations,
 * copies, memsets, buckets, workspace bytes, nImages with no octave}. Same argument checks as the call. */
MCV_API int mcvTestSiftBatchPlan(const mcvImage* images, int nImages, int mode, const void* config, long long* out8);
/* Host twin of cvBundleAdjust: the same arguments, checks, outputs, summary and return value, computed
 * sequentially by the host-compiled kernel arithmetic (ba_terms.h) in the kernels' summation orders. No GPU. */
MCV_API int mcvHostBundleAdjust(const mcvCamera* cameras, int nCameras, const uint8_t* fixedCameras,
                                const int* cameraIdx, const mcvV2d* observations, const int* offsets, int T,
                                const mcvV3d* points, const mcvBaConfig* cfg, mcvCamera* outCameras,
                                mcvV3d* outPoints, mcvBaSummary* summary);
/* The twin's linearisation at the given parameters: used[n], and per observation A[12] (2x6 row-major over
 * (omega, dc); zero for a camera that stays constant), B[6] (2x3), r[2] (all three scaled by sqrt(w)) and
 * w; zeros for an unused observation. Returns the number of used observations, -1 on failure. */
MCV_API int mcvHostBaLinearize(const mcvCamera* cameras, int nCameras, const uint8_t* fixedCameras,
                               const int* cameraIdx, const mcvV2d* observations, const int* offsets, int T,
                               const mcvV3d* points, const mcvBaConfig* cfg, uint8_t* used, double* A, double* B,
                               double* r, double* w);
/* The twin's first step at damping lambda: dCameras[6 nCameras] (omega, dc; zero for a constant camera)
 * and dPoints[3 T] (zero for an excluded track). Returns the PCG iterations, -1 on failure (a failed solve
 * included). */
MCV_API int mcvHostBaStep(const mcvCamera* cameras, int nCameras, const uint8_t* fixedCameras,
                          const int* cameraIdx, const mcvV2d* observations, const int* offsets, int T,
                          const mcvV3d* points, const mcvBaConfig* cfg, double lambda, double* dCameras,
                          double* dPoints);
/* Counters of the calling thread's last cvBundleAdjust call that reached the device: stats8 = {kernel
 * launches, stream synchronisations, host<->device copies, memsets, linearisations, trials (LM
 * iterations), chunks of 8 PCG iterations, segments of the camera lists}. Returns 0. */
MCV_API int mcvTestBundleAdjustStats(long long* stats8);
/* Host twin of cvBundleAdjustFocal: the same arguments, checks, outputs, summary and return value. No GPU. */
MCV_API int mcvHostBundleAdjustFocal(const mcvCamera* cameras, int nCameras, const uint8_t* fixedCameras,
                                     const int* focalGroup, const uint8_t* fixedFocal, const int* cameraIdx,
                                     const mcvV2d* observations, const int* offsets, int T, const mcvV3d* points,
                                     const mcvBaFocalConfig* cfg, mcvCamera* outCameras, mcvV3d* outPoints,
                                     mcvBaFocalSummary* summary);
/* The twin's first step at damping lambda with focalMode 1 or 2: focalBlocks[2 n] (per observation the
 * focal block scaled by sqrt(w): the column (u0, u1) of s for mode 1, diag(u0, u1) for mode 2; zero for an
 * unused observation or a constant group), dCameras[6 nCameras], dFocal[2 nCameras] (each camera's group
 * step: (s, 0) or (dfx, dfy)) and dPoints[3 T]. Returns the PCG iterations, -1 on failure. */
MCV_API int mcvHostBaFocalStep(const mcvCamera* cameras, int nCameras, const uint8_t* fixedCameras,
                               const int* focalGroup, const uint8_t* fixedFocal, const int* cameraIdx,
                               const mcvV2d* observations, const int* offsets, int T, const mcvV3d* points,
                               const mcvBaFocalConfig* cfg, double lambda, double* focalBlocks, double* dCameras,
                               double* dFocal, double* dPoints);
/* mcvTestBundleAdjustStats for the calling thread's last cvBundleAdjustFocal call that reached the device. */
MCV_API int mcvTestBundleAdjustFocalStats(long long* stats8);

#ifdef __cplusplus
}
#endif

#endif /* MINICV_NATIVE_H */
