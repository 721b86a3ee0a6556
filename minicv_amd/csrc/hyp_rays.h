// hyp_rays.h — Ray.intersection (src/MiniCV/Utilities.fs:100-165), the reference's multi-view
// triangulator, and the camera terms around it (Camera.unproject1 / Camera.project1,
// src/MiniCV/Camera.fs:72-91), compiled for gfx950 (triangulate.hip) and x86-64 (the mcvHost* twins,
// triangulate_ref.h). Every expression is fp64 in the evaluation order of the managed code (F#
// left to right, no FMA contraction: files are built -ffp-contract=off), with the IEEE quotient and
// square root (plain `/` and sqrt on both sides), so a value computed here is bit-identical on
// the host and on the GPU.
//
// Aardvark.Base semantics restated [ext: as recorded in hyp_scaled.h]: Vec.normalize(v) =
// v * (1 / |v|) (zero vector -> zero), |v| = sqrt(x*x + y*y + z*z), Vec.cross(a, b) =
// (a.Y b.Z - a.Z b.Y, a.Z b.X - a.X b.Z, a.X b.Y - a.Y b.X), s * V3d and V3d / s per component,
// Ray3d.GetPointOnRay(t) = Origin + Direction * t, Ray3d equality = == on the six doubles.
#pragma once

#include "mcv_common.h"

namespace mcv {

// sin 2 deg as the reference sees it: Utilities.fs:120-127 tests asin(clamp 0 1 len) * DegreesPerRadian
// > 2.0; this is the largest double for which that predicate is false with glibc's asin (found by
// bisection, and the double nearest sin 2 deg; tests/test_triangulate.py repeats the bisection), so
// `len > kSinMinAngle` is the same predicate without an asin on the device.
static const double kSinMinAngle = 0x1.1de58c9f7dc27p-5;

// ray_pair verdicts, in the order the reference tests them.
static const int kRayPairOk = 0, kRayPairAngle = 1, kRayPairBehind = 2, kRayPairNonFinite = 3;

// A ray is six doubles {origin, direction}: the layout of Aardvark's Ray3d and of mcvRay3d.
// cam points at the 14 doubles of an mcvCamera: location, forward, up, right, focal.

// Camera.unproject1 (Camera.fs:85-91).
MCV_HD void ray_unproject(const double* __restrict__ cam, double ox, double oy, double (&ray)[6]) {
    const double a = ox / cam[12], b = oy / cam[13];
    const double d0 = a * cam[9] + b * cam[6] + cam[3];
    const double d1 = a * cam[10] + b * cam[7] + cam[4];
    const double d2 = a * cam[11] + b * cam[8] + cam[5];
    const double l = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
    const double r = 1.0 / l;
    ray[0] = cam[0];
    ray[1] = cam[1];
    ray[2] = cam[2];
    ray[3] = l == 0.0 ? 0.0 : d0 * r;
    ray[4] = l == 0.0 ? 0.0 : d1 * r;
    ray[5] = l == 0.0 ? 0.0 : d2 * r;
}

MCV_HD bool ray_equal(const double (&a)[6], const double (&b)[6]) {
    return a[0] == b[0] && a[1] == b[1] && a[2] == b[2] && a[3] == b[3] && a[4] == b[4] && a[5] == b[5];
}

// One pair of intersections' (Utilities.fs:118-152): the angle test, getClosestTs
// (Utilities.fs:102-111), the in-front test and the midpoint. Returns kRayPairOk with the midpoint
// in pt, or the first test that rejected the pair.
MCV_HD int ray_pair(const double (&p)[6], const double (&q)[6], double (&pt)[3]) {
    const double cx = p[4] * q[5] - p[5] * q[4];
    const double cy = p[5] * q[3] - p[3] * q[5];
    const double cz = p[3] * q[4] - p[4] * q[3];
    const double len = sqrt(cx * cx + cy * cy + cz * cz);
    if (!(len > kSinMinAngle)) return kRayPairAngle;
    const double a0 = p[0] - q[0], a1 = p[1] - q[1], a2 = p[2] - q[2];
    const double udotv = p[3] * q[3] + p[4] * q[4] + p[5] * q[5];
    const double au = a0 * p[3] + a1 * p[4] + a2 * p[5];
    const double av = a0 * q[3] + a1 * q[4] + a2 * q[5];
    const double t1 = (au * udotv - av) / (udotv * udotv - 1.0);
    const double t0 = t1 * udotv - au;
    if (!(t0 > 0.0 && t1 > 0.0)) return kRayPairBehind;
    bool finite = true;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < 3; ++k) {
        pt[k] = 0.5 * ((p[k] + p[3 + k] * t0) + (q[k] + q[3 + k] * t1));
        finite = finite && __builtin_fabs(pt[k]) <= 0x1.fffffffffffffp1023;   // false for NaN and +-inf
    }
    return finite ? kRayPairOk : kRayPairNonFinite;
}

// One observation of avgReprojectionError's form (CameraPose.fs:77-92) against a fixed point:
// Camera.project1 (Camera.fs:72-83) and the squared distance to the observation. Returns false when
// the point is not visible (always for a NaN point); err is meaningful only when visible.
MCV_HD bool ray_project_term(const double* __restrict__ cam, const double (&pt)[3], double ox, double oy,
                             double& err) {
    const double o0 = pt[0] - cam[0], o1 = pt[1] - cam[1], o2 = pt[2] - cam[2];
    const double p0 = o0 * cam[9] + o1 * cam[10] + o2 * cam[11];
    const double p1 = o0 * cam[6] + o1 * cam[7] + o2 * cam[8];
    const double p2 = o0 * cam[3] + o1 * cam[4] + o2 * cam[5];
    const double cx = cam[12] * p0 / p2, cy = cam[13] * p1 / p2;
    const double dx = cx - ox, dy = cy - oy;
    err = dx * dx + dy * dy;
    return p2 >= 0.0 && cx >= -1.0 && cy >= -1.0 && cx <= 1.0 && cy <= 1.0;
}

}  // namespace mcv
