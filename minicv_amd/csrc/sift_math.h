// sift_math.h — the per-sample arithmetic of SIFT detection, compiled for gfx950 (sift.hip)
// and for the host twin (sift_ref.h). Every function here is the specification's evaluation order
// written out: float operations round once each as written (-ffp-contract=off), quotients and square
// roots go through double (the correctly rounded float result on both sides), exp and atan2 are glibc's
// bits (glibc_math.h), and the two histograms are sums of integers.
#pragma once

#include "mcv_common.h"
#include "glibc_math.h"

namespace mcv {

static const int kSiftBorder = 5;          // candidates and refined positions keep this distance from the rim
static const int kSiftMaxSteps = 5;        // refinement steps
static const int kSiftOriBins = 36;
static const int kSiftMaxPeaks = 18;       // strict circular maxima of 36 bins
static const int kSiftDescLen = 128;       // 4 x 4 x 8
static const int kSiftFixShift = 20;       // histogram contributions are integers of 2^-20
static const int kSiftMinLayers = 1, kSiftMaxLayers = 6;
static const int kSiftMaxSide = 8192;      // input width and height
static const double kSiftMaxSigma = 4.0;
// largest blur radius: OctaveLayers 1, Sigma 4 gives sigma 27.7, 223 taps; the column blur's LDS tile
// (32 + 2 x 111 rows of 64 floats) is then 65 024 bytes, under the 64 KiB a launch gets without opting in
static const int kSiftMaxRadius = 111;
static const int kSiftMaxCandidates = 1 << 22;   // extremum candidates of one call
// cvDetectFeaturesBatch. The three caps are design constants, not measurements: the image
// count keeps the image index in a grid's z and in 27 bits of a candidate record, the candidate cap
// keeps 18 records per candidate in 32-bit places, and the workspace cap (the buffers the plan sizes:
// images, pyramids, scratch, buckets, candidates) refuses a batch that should be split.
static const int kSiftBatchMaxImages = 4096;
static const int kSiftBatchMaxCandidates = 1 << 24;              // of all images of one call together
static const unsigned long long kSiftBatchMaxWorkspaceBytes = 1ull << 35;
static const int kSiftKeyBits = 45;        // of sift_key; a batch puts the image index above them

struct SiftParams {
    int nl;              // OctaveLayers
    float thr;           // candidate threshold floor(0.5 ContrastThreshold / nl * 255)
    float edge;          // (float)EdgeThreshold
    double contrast;     // ContrastThreshold
    double sigma;        // Sigma
};

// One refined extremum: octave o (0 = the doubled image), layer, integer position, sub-pixel offsets.
struct SiftKp {
    int o, layer, r, c;
    float xc, xr, xi, response, scl, size;
    int octave;   // OpenCV's packed code
};

// One output keypoint before descriptors: the sort keys, the KeyPoint2d fields and what the descriptor needs.
struct SiftRec {
    float x, y, size, angle, response;
    int octave, o, layer, r, c;
    float scl;
    int pad;
};

MCV_HD float sift_fdiv(float a, float b) { return (float)((double)a / (double)b); }
MCV_HD float sift_fsqrt(float a) { return (float)sqrt((double)a); }
MCV_HD float sift_rintf(float a) { return __builtin_rintf(a); }

// grey value of one pixel: 1 channel as it is, 3 or 4 as RGB(A) in OpenCV's fixed-point weights
MCV_HD float sift_grey(const uint8_t* px, int channels) {
    if (channels == 1) return (float)px[0];
    return (float)((4899 * (int)px[0] + 9617 * (int)px[1] + 1868 * (int)px[2] + 8192) >> 14);
}

// reflect-101, as often as needed; a length-1 axis maps to 0
MCV_HD int sift_reflect(int i, int n) {
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    int m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - m;
}

// (o, layer, r, c, bin): 5 + 4 + 15 + 15 + 6 bits
MCV_HD unsigned long long sift_key(int o, int layer, int r, int c, int bin) {
    return ((unsigned long long)o << 40) | ((unsigned long long)layer << 36) | ((unsigned long long)r << 21) |
           ((unsigned long long)c << 6) | (unsigned long long)bin;
}

// DoG sample: image l + 1 minus image l of the octave's Gaussian stack (plane = w h floats per image)
MCV_HD float sift_dog(const float* g, size_t plane, int w, int l, int r, int c) {
    const size_t at = (size_t)r * (size_t)w + (size_t)c;
    return g[(size_t)(l + 1) * plane + at] - g[(size_t)l * plane + at];
}

// Solves the symmetric 3 x 3 system H x = b by Gaussian elimination with partial pivoting (the first
// largest |pivot| of the column), rows updated left to right. False for a zero pivot.
MCV_HD bool sift_solve3(float a[3][3], float b[3], float x[3]) {
    for (int k = 0; k < 3; ++k) {
        int p = k;
        for (int i = k + 1; i < 3; ++i)
            if (fabsf(a[i][k]) > fabsf(a[p][k])) p = i;
        if (a[p][k] == 0.0f) return false;
        if (p != k) {
            for (int j = 0; j < 3; ++j) {
                const float t = a[k][j];
                a[k][j] = a[p][j];
                a[p][j] = t;
            }
            const float t = b[k];
            b[k] = b[p];
            b[p] = t;
        }
        for (int i = k + 1; i < 3; ++i) {
            const float f = sift_fdiv(a[i][k], a[k][k]);
            for (int j = k + 1; j < 3; ++j) a[i][j] = a[i][j] - f * a[k][j];
            b[i] = b[i] - f * b[k];
        }
    }
    x[2] = sift_fdiv(b[2], a[2][2]);
    x[1] = sift_fdiv(b[1] - a[1][2] * x[2], a[1][1]);
    x[0] = sift_fdiv((b[0] - a[0][1] * x[1]) - a[0][2] * x[2], a[0][0]);
    return true;
}

// Sub-pixel refinement and the contrast / edge rejections of one candidate (cv::SIFT's adjustLocalExtrema).
MCV_HD bool sift_refine(const float* g, int w, int h, int o, int layer, int r, int c, const SiftParams& P,
                        SiftKp& kp) {
    const size_t plane = (size_t)w * (size_t)h;
    const float is = 1.0f / 255.0f, ds = is * 0.5f, cs = is * 0.25f;
    float xc = 0, xr = 0, xi = 0;
    float dD[3];
    int step = 0;
    for (; step < kSiftMaxSteps; ++step) {
#define MCV_D(l, rr, cc) sift_dog(g, plane, w, (l), (rr), (cc))
        dD[0] = (MCV_D(layer, r, c + 1) - MCV_D(layer, r, c - 1)) * ds;
        dD[1] = (MCV_D(layer, r + 1, c) - MCV_D(layer, r - 1, c)) * ds;
        dD[2] = (MCV_D(layer + 1, r, c) - MCV_D(layer - 1, r, c)) * ds;
        const float v2 = MCV_D(layer, r, c) * 2.0f;
        const float dxx = ((MCV_D(layer, r, c + 1) + MCV_D(layer, r, c - 1)) - v2) * is;
        const float dyy = ((MCV_D(layer, r + 1, c) + MCV_D(layer, r - 1, c)) - v2) * is;
        const float dss = ((MCV_D(layer + 1, r, c) + MCV_D(layer - 1, r, c)) - v2) * is;
        const float dxy = (((MCV_D(layer, r + 1, c + 1) - MCV_D(layer, r + 1, c - 1)) - MCV_D(layer, r - 1, c + 1)) +
                           MCV_D(layer, r - 1, c - 1)) * cs;
        const float dxs = (((MCV_D(layer + 1, r, c + 1) - MCV_D(layer + 1, r, c - 1)) - MCV_D(layer - 1, r, c + 1)) +
                           MCV_D(layer - 1, r, c - 1)) * cs;
        const float dys = (((MCV_D(layer + 1, r + 1, c) - MCV_D(layer + 1, r - 1, c)) - MCV_D(layer - 1, r + 1, c)) +
                           MCV_D(layer - 1, r - 1, c)) * cs;
        float A[3][3] = {{dxx, dxy, dxs}, {dxy, dyy, dys}, {dxs, dys, dss}};
        float b[3] = {dD[0], dD[1], dD[2]}, X[3];
        if (!sift_solve3(A, b, X)) return false;
        xc = -X[0];
        xr = -X[1];
        xi = -X[2];
        if (fabsf(xi) < 0.5f && fabsf(xr) < 0.5f && fabsf(xc) < 0.5f) break;
        if (!(fabsf(xi) < 65536.0f && fabsf(xr) < 65536.0f && fabsf(xc) < 65536.0f)) return false;
        c += (int)sift_rintf(xc);
        r += (int)sift_rintf(xr);
        layer += (int)sift_rintf(xi);
        if (layer < 1 || layer > P.nl || c < kSiftBorder || c >= w - kSiftBorder || r < kSiftBorder ||
            r >= h - kSiftBorder)
            return false;
    }
    if (step >= kSiftMaxSteps) return false;
    const float t = (dD[0] * xc + dD[1] * xr) + dD[2] * xi;
    const float contr = MCV_D(layer, r, c) * is + t * 0.5f;
    if ((double)(fabsf(contr) * (float)P.nl) < P.contrast) return false;
    const float v2 = MCV_D(layer, r, c) * 2.0f;
    const float dxx = ((MCV_D(layer, r, c + 1) + MCV_D(layer, r, c - 1)) - v2) * is;
    const float dyy = ((MCV_D(layer, r + 1, c) + MCV_D(layer, r - 1, c)) - v2) * is;
    const float dxy = (((MCV_D(layer, r + 1, c + 1) - MCV_D(layer, r + 1, c - 1)) - MCV_D(layer, r - 1, c + 1)) +
                       MCV_D(layer, r - 1, c - 1)) * cs;
#undef MCV_D
    const float tr = dxx + dyy, det = dxx * dyy - dxy * dxy;
    if (det <= 0.0f || (tr * tr) * P.edge >= ((P.edge + 1.0f) * (P.edge + 1.0f)) * det) return false;
    kp.o = o;
    kp.layer = layer;
    kp.r = r;
    kp.c = c;
    kp.xc = xc;
    kp.xr = xr;
    kp.xi = xi;
    kp.response = fabsf(contr);
    // scale within the octave: Sigma 2^((layer + xi) / nl), the power through exp in double
    const double e = ((double)((float)layer + xi) / (double)P.nl) * 0.6931471805599453;
    const double sd = P.sigma * glibc_exp(e);
    kp.scl = (float)sd;
    kp.size = (float)(sd * (double)(1 << o));   // x 2 for the diameter, x 1/2 for the doubled first octave
    kp.octave = ((o - 1) & 255) | (layer << 8) | ((int)sift_rintf((xi + 0.5f) * 255.0f) << 16);
    return true;
}

// Gradient of Gaussian image img at (r, c), 0 < r < h - 1, 0 < c < w - 1: magnitude (float) and glibc's
// atan2(dy, dx) in radians (0 for a zero gradient).
MCV_HD void sift_gradient(const float* img, int w, int r, int c, float& mag, double& ang) {
    const size_t at = (size_t)r * (size_t)w + (size_t)c;
    const float dx = img[at + 1] - img[at - 1];
    const float dy = img[at - (size_t)w] - img[at + (size_t)w];
    mag = (float)sqrt((double)dx * (double)dx + (double)dy * (double)dy);
    ang = (dx == 0.0f && dy == 0.0f) ? 0.0 : glibc_atan2((double)dy, (double)dx);
}

MCV_HD long long sift_fix(float v) { return (long long)__builtin_rint((double)v * (double)(1 << kSiftFixShift)); }
MCV_HD float sift_unfix(long long s) { return (float)((double)s * (1.0 / (double)(1 << kSiftFixShift))); }

MCV_HD int sift_ori_radius(float scl) { return (int)sift_rintf(4.5f * scl); }

// Sample (i, j) of the orientation window around (r, c): false outside the image's interior.
MCV_HD bool sift_ori_sample(const float* img, int w, int h, int r, int c, int i, int j, float escale, int& bin,
                            long long& q) {
    const int y = r + i, x = c + j;
    if (y <= 0 || y >= h - 1 || x <= 0 || x >= w - 1) return false;
    float mag;
    double ang;
    sift_gradient(img, w, y, x, mag, ang);
    const float wt = (float)glibc_exp((double)((float)(i * i + j * j) * escale));
    int b = (int)__builtin_rint(ang * 5.729577951308232);   // 36 / (2 pi)
    if (b < 0) b += kSiftOriBins;
    if (b >= kSiftOriBins) b -= kSiftOriBins;
    bin = b;
    q = sift_fix(wt * mag);
    return true;
}
MCV_HD float sift_ori_escale(float scl) {
    const float so = 1.5f * scl;
    return sift_fdiv(-1.0f, (2.0f * so) * so);
}

// The integer histogram -> smoothed float histogram -> peaks: bins[k], angles[k] (degrees); the count.
MCV_HD int sift_ori_peaks(const long long* sum, int* bins, float* angles) {
    float raw[kSiftOriBins], hist[kSiftOriBins];
    for (int k = 0; k < kSiftOriBins; ++k) raw[k] = sift_unfix(sum[k]);
    float mx = 0.0f;
    for (int k = 0; k < kSiftOriBins; ++k) {
        const float m2 = raw[(k + 34) % 36], m1 = raw[(k + 35) % 36], p1 = raw[(k + 1) % 36], p2 = raw[(k + 2) % 36];
        hist[k] = ((m2 + p2) * (1.0f / 16.0f) + (m1 + p1) * (4.0f / 16.0f)) + raw[k] * (6.0f / 16.0f);
        if (hist[k] > mx) mx = hist[k];
    }
    const float thr = mx * 0.8f;
    int n = 0;
    for (int k = 0; k < kSiftOriBins; ++k) {
        const float l = hist[(k + 35) % 36], rt = hist[(k + 1) % 36], v = hist[k];
        if (v > l && v > rt && v >= thr) {
            float bin = (float)k + sift_fdiv(0.5f * (l - rt), (l - 2.0f * v) + rt);
            if (bin < 0.0f) bin = bin + 36.0f;
            if (bin >= 36.0f) bin = bin - 36.0f;
            float a = 360.0f - 10.0f * bin;
            if (fabsf(a - 360.0f) < 1.1920929e-7f) a = 0.0f;
            bins[n] = k;
            angles[n] = a;
            ++n;
        }
    }
    return n;
}

// cos and sin of an angle in degrees, [0, 360]: the quadrant by rint(a / 90), then the Taylor
// polynomials of degree 13 / 12 in double, Horner from the highest term.
MCV_HD void sift_sincos_deg(float deg, float& c, float& s) {
    const double a = (double)deg;
    const int q = (int)__builtin_rint(a / 90.0);
    const double x = (a - 90.0 * (double)q) * 0.017453292519943295;
    const double x2 = x * x;
    double ps = 1.0 / 6227020800.0;
    ps = -1.0 / 39916800.0 + x2 * ps;
    ps = 1.0 / 362880.0 + x2 * ps;
    ps = -1.0 / 5040.0 + x2 * ps;
    ps = 1.0 / 120.0 + x2 * ps;
    ps = -1.0 / 6.0 + x2 * ps;
    ps = x * (1.0 + x2 * ps);
    double pc = 1.0 / 479001600.0;
    pc = -1.0 / 3628800.0 + x2 * pc;
    pc = 1.0 / 40320.0 + x2 * pc;
    pc = -1.0 / 720.0 + x2 * pc;
    pc = 1.0 / 24.0 + x2 * pc;
    pc = -1.0 / 2.0 + x2 * pc;
    pc = 1.0 + x2 * pc;
    const int k = q & 3;
    const double cd = k == 0 ? pc : k == 1 ? -ps : k == 2 ? -pc : ps;
    const double sd = k == 0 ? ps : k == 1 ? pc : k == 2 ? -ps : -pc;
    c = (float)cd;
    s = (float)sd;
}

// What the descriptor of one keypoint needs, computed once.
struct SiftDescFrame {
    float ct, st;      // cos, sin of the orientation over the histogram width
    double ori;        // the orientation in radians
    int radius;
};
MCV_HD SiftDescFrame sift_desc_frame(float angle, float scl, int w, int h) {
    SiftDescFrame F;
    float ori = 360.0f - angle;
    if (fabsf(ori - 360.0f) < 1.1920929e-7f) ori = 0.0f;
    float c, s;
    sift_sincos_deg(ori, c, s);
    const float hw = 3.0f * scl;
    int radius = (int)sift_rintf(((hw * 1.4142135623730951f) * 5.0f) * 0.5f);
    const int diag = (int)sqrt((double)w * (double)w + (double)h * (double)h);
    F.radius = radius < diag ? radius : diag;
    F.ct = sift_fdiv(c, hw);
    F.st = sift_fdiv(s, hw);
    F.ori = (double)ori * 0.017453292519943295;
    return F;
}

// Sample (i, j) of the descriptor window around (r, c): up to 8 trilinear contributions, each handed to
// add(index in [0, 128), integer value).
template <class Add>
MCV_HD void sift_desc_sample(const float* img, int w, int h, int r, int c, int i, int j, const SiftDescFrame& F,
                             Add add) {
    const float fi = (float)i, fj = (float)j;
    const float crot = fj * F.ct - fi * F.st, rrot = fj * F.st + fi * F.ct;
    float rbin = rrot + 1.5f, cbin = crot + 1.5f;
    const int y = r + i, x = c + j;
    if (!(rbin > -1.0f && rbin < 4.0f && cbin > -1.0f && cbin < 4.0f && y > 0 && y < h - 1 && x > 0 && x < w - 1))
        return;
    float gm;
    double ang;
    sift_gradient(img, w, y, x, gm, ang);
    const float wt = (float)glibc_exp((double)((crot * crot + rrot * rrot) * -0.125f));
    float obin = (float)((ang - F.ori) * 1.2732395447351628);   // 8 / (2 pi)
    const float mag = wt * gm;
    const float r0f = floorf(rbin), c0f = floorf(cbin), o0f = floorf(obin);
    rbin = rbin - r0f;
    cbin = cbin - c0f;
    obin = obin - o0f;
    const int r0 = (int)r0f, c0 = (int)c0f;
    int o0 = (int)o0f % 8;
    if (o0 < 0) o0 += 8;
    const int o1 = (o0 + 1) & 7;
    const float vr1 = mag * rbin, vr0 = mag - vr1;
    const float v11 = vr1 * cbin, v10 = vr1 - v11, v01 = vr0 * cbin, v00 = vr0 - v01;
    const float v111 = v11 * obin, v110 = v11 - v111, v101 = v10 * obin, v100 = v10 - v101;
    const float v011 = v01 * obin, v010 = v01 - v011, v001 = v00 * obin, v000 = v00 - v001;
    const bool ra = r0 >= 0, rb = r0 + 1 < 4, ca = c0 >= 0, cb = c0 + 1 < 4;   // r0, c0 in [-1, 3]
    if (ra && ca) {
        add((r0 * 4 + c0) * 8 + o0, sift_fix(v000));
        add((r0 * 4 + c0) * 8 + o1, sift_fix(v001));
    }
    if (ra && cb) {
        add((r0 * 4 + c0 + 1) * 8 + o0, sift_fix(v010));
        add((r0 * 4 + c0 + 1) * 8 + o1, sift_fix(v011));
    }
    if (rb && ca) {
        add(((r0 + 1) * 4 + c0) * 8 + o0, sift_fix(v100));
        add(((r0 + 1) * 4 + c0) * 8 + o1, sift_fix(v101));
    }
    if (rb && cb) {
        add(((r0 + 1) * 4 + c0 + 1) * 8 + o0, sift_fix(v110));
        add(((r0 + 1) * 4 + c0 + 1) * 8 + o1, sift_fix(v111));
    }
}

// The 128 integer sums -> the normalised float descriptor (clamp at 0.2 of the norm, scale to 512).
MCV_HD void sift_desc_finish(const long long* sum, float* out) {
    float n2 = 0.0f;
    for (int k = 0; k < kSiftDescLen; ++k) {
        out[k] = sift_unfix(sum[k]);
        n2 = n2 + out[k] * out[k];
    }
    const float thr = sift_fsqrt(n2) * 0.2f;
    n2 = 0.0f;
    for (int k = 0; k < kSiftDescLen; ++k) {
        const float v = out[k] < thr ? out[k] : thr;
        out[k] = v;
        n2 = n2 + v * v;
    }
    float nrm = sift_fsqrt(n2);
    if (nrm < 1.1920929e-7f) nrm = 1.1920929e-7f;
    const float scale = sift_fdiv(512.0f, nrm);
    for (int k = 0; k < kSiftDescLen; ++k) out[k] = out[k] * scale;
}
MCV_HD uint8_t sift_desc_byte(float v) {
    const float r = sift_rintf(v);
    return r <= 0.0f ? (uint8_t)0 : r >= 255.0f ? (uint8_t)255 : (uint8_t)(int)r;
}

}  // namespace mcv
