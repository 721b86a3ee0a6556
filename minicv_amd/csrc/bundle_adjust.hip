// bundle_adjust.hip — gfx950 kernels of cvBundleAdjust: Levenberg-Marquardt over cameras
// and track points with a matrix-free PCG on the reduced camera system. The arithmetic is ba_terms.h
// (fp64, shared with the host twin); what lives here is who sums what, in the orders of the contract:
//
//   per point    a track of at most kBaShortMax observations is one lane's chain in track order; a
//                longer one is a wave: lane l chains entries l, l + 64, ..., then p[l] += p[l + s],
//                s = 32 .. 1 (long tracks are queued on the device by mcv_ba_used_track)
//   per camera   a workgroup per (camera, segment of kBaSeg entries): lane l of 256 chains entries
//                l, l + 256, ..., then p[l] += p[l + s], s = 128 .. 1; a per-camera final chains the
//                segments in order
//   over cameras (dot products, the total cost) one workgroup: 256 strided lanes and the same tree
//
// No floating-point atomics anywhere; the integer counters and flags are order-free. The PCG scalars
// live in a BaCgState on the device: every kernel of a finished solve returns at once, and no kernel
// waits on memory another kernel writes.
#include "minicv_native.h"
#include "ba_terms.h"
#include "kernels.h"
#include "plan.h"

namespace mcv {

// ---- the reductions ----

// Wave per long track: lane's chain, then the fold. Every lane of the wave must call it; lane 0
// holds the sums.
template <int NQ, class F>
__device__ __forceinline__ void ba_wave_sum(int o0, int R, int lane, F f, double (&acc)[NQ]) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
    for (int i = lane; i < R; i += 64) f(o0 + i, acc);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) acc[q] = acc[q] + __shfl_down(acc[q], s, 64);   // lanes >= s hold unused values
    }
}

// Workgroup of kBaSegLanes threads: lds[NQ][kBaSegLanes]; every thread must call it. The sums are
// in lds[q * kBaSegLanes] afterwards (visible to every thread).
template <int NQ>
__device__ __forceinline__ void ba_block_tree(const double (&acc)[NQ], double* lds) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int q = 0; q < NQ; ++q) lds[q * kBaSegLanes + tid] = acc[q];
    __syncthreads();
    for (int s = kBaSegLanes / 2; s >= 1; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int q = 0; q < NQ; ++q)
                lds[q * kBaSegLanes + tid] = lds[q * kBaSegLanes + tid] + lds[q * kBaSegLanes + tid + s];
        }
        __syncthreads();
    }
}

// One segment of a camera's list: f(k, acc) adds observation k's terms; the NQ sums go to part.
template <int NQ, class F>
__device__ __forceinline__ void ba_seg_sum(const BaDevice& D, int seg, F f, double* lds) {
    double acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
    const int end = D.segEnd[seg];
    for (int i = D.segStart[seg] + (int)threadIdx.x; i < end; i += kBaSegLanes) f(D.camObs[i], acc);
    ba_block_tree<NQ>(acc, lds);
    if (threadIdx.x < NQ) D.part[27 * (size_t)seg + threadIdx.x] = lds[threadIdx.x * kBaSegLanes];
}

// The segments of camera j, chained in order from +0.0.
template <int NQ>
__device__ __forceinline__ void ba_cam_total(const BaDevice& D, int j, double (&out)[NQ]) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) out[q] = 0.0;
    for (int s = D.camSegPtr[j]; s < D.camSegPtr[j + 1]; ++s) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) out[q] = out[q] + D.part[27 * (size_t)s + q];
    }
}

// One value per thread (its chain over the cameras tid, tid + 256, ...) to the total, in every thread.
__device__ __forceinline__ double ba_block_total(double v, double* lds) {
    const double acc[1] = {v};
    __syncthreads();   // lds may still be read from the previous total
    ba_block_tree<1>(acc, lds);
    return lds[0];
}

// ---- setup: the used set ----

__global__ __launch_bounds__(256) void mcv_ba_used_obs(BaDevice D) {
    for (int k = blockIdx.x * 256 + threadIdx.x; k < D.n; k += gridDim.x * 256) {
        const double* X = D.pts + 3 * (size_t)D.obsTrack[k];
        double pc[3], r[2];
        const bool fin = ba_finite(X[0]) && ba_finite(X[1]) && ba_finite(X[2]);
        const bool ok = ba_project(D.cams + 14 * (size_t)D.cameraIdx[k], X, D.obs[2 * (size_t)k], D.obs[2 * (size_t)k + 1], pc, r);
        D.used[k] = fin && ok ? 1 : 0;
    }
}

// Lane per track: a track with fewer than two used observations is excluded; long used tracks are queued.
__global__ __launch_bounds__(256) void mcv_ba_used_track(BaDevice D, int* __restrict__ camHas) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= D.T) return;
    const int o0 = D.offsets[t], o1 = D.offsets[t + 1];
    int cnt = 0;
    for (int k = o0; k < o1; ++k) cnt += D.used[k];
    if (cnt < 2) {
        for (int k = o0; k < o1; ++k) D.used[k] = 0;
        D.trackUsed[t] = 0;
        return;
    }
    D.trackUsed[t] = 1;
    for (int k = o0; k < o1; ++k)
        if (D.used[k]) camHas[D.cameraIdx[k]] = 1;   // every writer stores the same value
    atomicAdd(&D.ctr[1], (unsigned int)cnt);
    atomicAdd(&D.ctr[2], 1u);
    if (o1 - o0 > kBaShortMax) D.longList[atomicAdd(&D.ctr[0], 1u)] = t;
}

__global__ __launch_bounds__(256) void mcv_ba_active(BaDevice D, const int* __restrict__ camHas) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < D.nCameras) D.active[j] = camHas[j] && !D.fixed[j] ? 1 : 0;
}

// ---- cost of given parameters ----

__global__ __launch_bounds__(kBaSegLanes) void mcv_ba_cost_seg(BaDevice D, const double* __restrict__ cams,
                                                               const double* __restrict__ pts) {
    __shared__ double lds[kBaSegLanes];
    const int seg = blockIdx.x;
    const double* cam = cams + 14 * (size_t)D.segCam[seg];
    bool bad = false;
    ba_seg_sum<1>(D, seg, [&](int k, double (&acc)[1]) {
        if (!D.used[k]) return;
        bool zp;
        const double rho = ba_rho(cam, pts + 3 * (size_t)D.obsTrack[k], D.obs[2 * (size_t)k], D.obs[2 * (size_t)k + 1], D.delta, zp);
        bad = bad || !zp;
        acc[0] = acc[0] + rho;
    }, lds);
    if (bad) atomicOr(&D.ctr[4], 1u);
}

__global__ __launch_bounds__(kBaSegLanes) void mcv_ba_cost_final(BaDevice D) {
    __shared__ double lds[kBaSegLanes];
    double acc = 0.0;
    for (int j = threadIdx.x; j < D.nCameras; j += kBaSegLanes) {
        double c[1];
        ba_cam_total<1>(D, j, c);
        acc = acc + c[0];
    }
    const double total = ba_block_total(acc, lds);
    if (threadIdx.x == 0) {
        D.rec->cost = total;
        D.rec->badz = (int)D.ctr[4];
        D.ctr[4] = 0;
    }
}

// ---- linearise ----

__device__ __forceinline__ void ba_lin_entry(const BaDevice& D, int t, int k, double* acc) {
    if (!D.used[k]) return;
    const int j = D.cameraIdx[k];
    double e[kBaEntry];
    ba_linearize(D.cams + 14 * (size_t)j, D.pts + 3 * (size_t)t, D.obs[2 * (size_t)k], D.obs[2 * (size_t)k + 1], D.delta,
                 D.active[j] != 0, e);
    double* out = D.E + (size_t)kBaEntry * k;
#pragma unroll
    for (int q = 0; q < kBaEntry; ++q) out[q] = e[q];
    ba_acc_point_lin(e, acc);
}

__device__ __forceinline__ void ba_lin_store(const BaDevice& D, int t, const double (&acc)[9]) {
#pragma unroll
    for (int q = 0; q < 6; ++q) D.V[6 * (size_t)t + q] = acc[q];
#pragma unroll
    for (int q = 0; q < 3; ++q) D.h[3 * (size_t)t + q] = -acc[6 + q];
}

__global__ __launch_bounds__(256) void mcv_ba_lin_short(BaDevice D) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= D.T || !D.trackUsed[t]) return;
    const int o0 = D.offsets[t], R = D.offsets[t + 1] - o0;
    if (R > kBaShortMax) return;
    double acc[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < R; ++i) ba_lin_entry(D, t, o0 + i, acc);
    ba_lin_store(D, t, acc);
}

__global__ __launch_bounds__(256) void mcv_ba_lin_long(BaDevice D) {
    const int lane = threadIdx.x & 63, nLong = (int)D.ctr[0];
    for (int w = blockIdx.x * 4 + (threadIdx.x >> 6); w < nLong; w += gridDim.x * 4) {
        const int t = D.longList[w], o0 = D.offsets[t];
        double acc[9];
        ba_wave_sum<9>(o0, D.offsets[t + 1] - o0, lane, [&](int k, double (&a)[9]) { ba_lin_entry(D, t, k, a); }, acc);
        if (lane == 0) ba_lin_store(D, t, acc);
    }
}

__global__ __launch_bounds__(kBaSegLanes) void mcv_ba_lin_cam_seg(BaDevice D) {
    __shared__ double lds[27 * kBaSegLanes];
    ba_seg_sum<27>(D, blockIdx.x, [&](int k, double (&acc)[27]) {
        if (!D.used[k]) return;
        double e[kBaEntry];
#pragma unroll
        for (int q = 0; q < kBaEntry; ++q) e[q] = D.E[(size_t)kBaEntry * k + q];
        ba_acc_cam_lin(e, acc);
    }, lds);
}

__global__ __launch_bounds__(256) void mcv_ba_lin_cam_final(BaDevice D) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= D.nCameras) return;
    double acc[27];
    ba_cam_total<27>(D, j, acc);
#pragma unroll
    for (int q = 0; q < 21; ++q) D.U[21 * (size_t)j + q] = acc[q];
#pragma unroll
    for (int q = 0; q < 6; ++q) D.g[6 * (size_t)j + q] = -acc[21 + q];
}

// ---- the damped reduced system ----

__global__ __launch_bounds__(256) void mcv_ba_point_solve(BaDevice D) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= D.T || !D.trackUsed[t]) return;
    double V[6], inv[6], h[3], tt[3];
#pragma unroll
    for (int q = 0; q < 6; ++q) V[q] = D.V[6 * (size_t)t + q];
#pragma unroll
    for (int q = 0; q < 3; ++q) h[q] = D.h[3 * (size_t)t + q];
    if (!ba_inv3(V, D.lambda, inv)) atomicOr(&D.ctr[3], 1u);
    ba_symv3(inv, h, tt);
#pragma unroll
    for (int q = 0; q < 6; ++q) D.Vinv[6 * (size_t)t + q] = inv[q];
#pragma unroll
    for (int q = 0; q < 3; ++q) D.t[3 * (size_t)t + q] = tt[q];
}

__global__ __launch_bounds__(kBaSegLanes) void mcv_ba_schur_seg(BaDevice D) {
    __shared__ double lds[27 * kBaSegLanes];
    ba_seg_sum<27>(D, blockIdx.x, [&](int k, double (&acc)[27]) {
        if (!D.used[k]) return;
        const int i = D.obsTrack[k];
        double e[kBaEntry], inv[6], tt[3];
#pragma unroll
        for (int q = 0; q < kBaEntry; ++q) e[q] = D.E[(size_t)kBaEntry * k + q];
#pragma unroll
        for (int q = 0; q < 6; ++q) inv[q] = D.Vinv[6 * (size_t)i + q];
#pragma unroll
        for (int q = 0; q < 3; ++q) tt[q] = D.t[3 * (size_t)i + q];
        ba_acc_cam_schur(e, inv, tt, acc);
    }, lds);
}

__global__ __launch_bounds__(256) void mcv_ba_schur_final(BaDevice D) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= D.nCameras) return;
    double acc[27], S[21], L[21];
    ba_cam_total<27>(D, j, acc);
#pragma unroll
    for (int q = 0; q < 21; ++q) S[q] = D.U[21 * (size_t)j + q];
#pragma unroll
    for (int a = 0; a < 6; ++a) S[ba_u6(a, a)] = ba_damp(S[ba_u6(a, a)], D.lambda);
#pragma unroll
    for (int q = 0; q < 21; ++q) S[q] = S[q] - acc[q];
#pragma unroll
    for (int q = 0; q < 6; ++q) D.b[6 * (size_t)j + q] = D.g[6 * (size_t)j + q] - acc[21 + q];
    if (!ba_chol6(S, L)) atomicOr(&D.ctr[3], 1u);
#pragma unroll
    for (int q = 0; q < 21; ++q) D.L[21 * (size_t)j + q] = L[q];
}

__device__ __forceinline__ void ba_precondition(const BaDevice& D, int j, const double (&r)[6], double (&z)[6]) {
    double L[21];
#pragma unroll
    for (int q = 0; q < 21; ++q) L[q] = D.L[21 * (size_t)j + q];
    ba_chol6_solve(L, r, z);
}

// One workgroup: x = 0, r = b, z = M r, p = z, r.z, and the record of the solve.
__global__ __launch_bounds__(kBaSegLanes) void mcv_ba_pcg_init(BaDevice D) {
    __shared__ double lds[kBaSegLanes];
    const bool failed = D.ctr[3] != 0;
    double acc = 0.0;
    if (!failed) {
        for (int j = threadIdx.x; j < D.nCameras; j += kBaSegLanes) {
            double r[6], z[6];
#pragma unroll
            for (int a = 0; a < 6; ++a) r[a] = D.b[6 * (size_t)j + a];
            ba_precondition(D, j, r, z);
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                D.x[6 * (size_t)j + a] = 0.0;
                D.r[6 * (size_t)j + a] = r[a];
                D.z[6 * (size_t)j + a] = z[a];
                D.p[6 * (size_t)j + a] = z[a];
            }
            acc = acc + ba_dot6(r, z);
        }
    }
    const double rz = ba_block_total(acc, lds);
    if (threadIdx.x == 0) {
        const bool bad = failed || !ba_finite(rz);
        D.cg->rz = rz;
        D.cg->rz0 = rz;
        D.cg->iter = 0;
        D.cg->failed = bad ? 1 : 0;
        D.cg->done = bad || rz <= D.tol2 * rz || D.maxCg <= 0 ? 1 : 0;
    }
}

// ---- PCG ----

// MODE 0: y = Vinv sum W^T p of the solve in flight. MODE 1: the same over x, then the point's
// trial value pts2 = pts + (t - y); the points of excluded tracks are copied.
template <int MODE>
__device__ __forceinline__ void ba_point_entry(const BaDevice& D, int k, double* acc) {
    if (!D.used[k]) return;
    double e[18], v[6];
#pragma unroll
    for (int q = 0; q < 18; ++q) e[q] = D.E[(size_t)kBaEntry * k + q];
    const double* src = (MODE == 0 ? D.p : D.x) + 6 * (size_t)D.cameraIdx[k];
#pragma unroll
    for (int q = 0; q < 6; ++q) v[q] = src[q];
    ba_acc_point_wtp(e, v, acc);
}

template <int MODE>
__device__ __forceinline__ void ba_point_store(const BaDevice& D, int t, const double (&acc)[3]) {
    double inv[6], y[3];
#pragma unroll
    for (int q = 0; q < 6; ++q) inv[q] = D.Vinv[6 * (size_t)t + q];
    ba_symv3(inv, acc, y);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        if (MODE == 0) D.y[3 * (size_t)t + q] = y[q];
        else D.pts2[3 * (size_t)t + q] = D.pts[3 * (size_t)t + q] + (D.t[3 * (size_t)t + q] - y[q]);
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void mcv_ba_point_short(BaDevice D) {
    if (MODE == 0 && D.cg->done) return;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= D.T) return;
    if (!D.trackUsed[t]) {
        if (MODE == 1) {
#pragma unroll
            for (int q = 0; q < 3; ++q) D.pts2[3 * (size_t)t + q] = D.pts[3 * (size_t)t + q];
        }
        return;
    }
    const int o0 = D.offsets[t], R = D.offsets[t + 1] - o0;
    if (R > kBaShortMax) return;
    double acc[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < R; ++i) ba_point_entry<MODE>(D, o0 + i, acc);
    ba_point_store<MODE>(D, t, acc);
}

template <int MODE>
__global__ __launch_bounds__(256) void mcv_ba_point_long(BaDevice D) {
    if (MODE == 0 && D.cg->done) return;
    const int lane = threadIdx.x & 63, nLong = (int)D.ctr[0];
    for (int w = blockIdx.x * 4 + (threadIdx.x >> 6); w < nLong; w += gridDim.x * 4) {
        const int t = D.longList[w], o0 = D.offsets[t];
        double acc[3];
        ba_wave_sum<3>(o0, D.offsets[t + 1] - o0, lane, [&](int k, double (&a)[3]) { ba_point_entry<MODE>(D, k, a); }, acc);
        if (lane == 0) ba_point_store<MODE>(D, t, acc);
    }
}

__global__ __launch_bounds__(kBaSegLanes) void mcv_ba_wy_seg(BaDevice D) {
    __shared__ double lds[6 * kBaSegLanes];
    if (D.cg->done) return;
    ba_seg_sum<6>(D, blockIdx.x, [&](int k, double (&acc)[6]) {
        if (!D.used[k]) return;
        double e[18], y[3];
#pragma unroll
        for (int q = 0; q < 18; ++q) e[q] = D.E[(size_t)kBaEntry * k + q];
#pragma unroll
        for (int q = 0; q < 3; ++q) y[q] = D.y[3 * (size_t)D.obsTrack[k] + q];
        ba_acc_cam_wy(e, y, acc);
    }, lds);
}

// q_j = U_lambda p_j - sum W y, and the camera's share of p.q
__global__ __launch_bounds__(256) void mcv_ba_q_final(BaDevice D) {
    if (D.cg->done) return;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= D.nCameras) return;
    double acc[6], U[21], p[6], up[6], q[6];
    ba_cam_total<6>(D, j, acc);
#pragma unroll
    for (int k = 0; k < 21; ++k) U[k] = D.U[21 * (size_t)j + k];
#pragma unroll
    for (int a = 0; a < 6; ++a) U[ba_u6(a, a)] = ba_damp(U[ba_u6(a, a)], D.lambda);
#pragma unroll
    for (int a = 0; a < 6; ++a) p[a] = D.p[6 * (size_t)j + a];
    ba_symv6(U, p, up);
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        q[a] = up[a] - acc[a];
        D.q[6 * (size_t)j + a] = q[a];
    }
    D.pq[j] = ba_dot6(p, q);
}

// One workgroup: alpha, x, r, z = M r, beta, p and the record of the solve.
__global__ __launch_bounds__(kBaSegLanes) void mcv_ba_pcg_update(BaDevice D) {
    __shared__ double lds[kBaSegLanes];
    const BaCgState st = *D.cg;   // read by every thread before thread 0 writes it below (barriers between)
    if (st.done) return;
    double acc = 0.0;
    for (int j = threadIdx.x; j < D.nCameras; j += kBaSegLanes) acc = acc + D.pq[j];
    const double pq = ba_block_total(acc, lds);
    const double alpha = st.rz / pq;
    if (!(pq > 0.0) || !ba_finite(alpha)) {
        if (threadIdx.x == 0) {
            D.cg->failed = 1;
            D.cg->done = 1;
        }
        return;
    }
    acc = 0.0;
    for (int j = threadIdx.x; j < D.nCameras; j += kBaSegLanes) {
        double r[6], z[6];
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            D.x[6 * (size_t)j + a] = D.x[6 * (size_t)j + a] + alpha * D.p[6 * (size_t)j + a];
            r[a] = D.r[6 * (size_t)j + a] - alpha * D.q[6 * (size_t)j + a];
            D.r[6 * (size_t)j + a] = r[a];
        }
        ba_precondition(D, j, r, z);
#pragma unroll
        for (int a = 0; a < 6; ++a) D.z[6 * (size_t)j + a] = z[a];
        acc = acc + ba_dot6(r, z);
    }
    const double rzn = ba_block_total(acc, lds);
    if (!ba_finite(rzn)) {
        if (threadIdx.x == 0) {
            D.cg->failed = 1;
            D.cg->done = 1;
        }
        return;
    }
    const double beta = rzn / st.rz;
    for (int j = threadIdx.x; j < D.nCameras; j += kBaSegLanes) {
#pragma unroll
        for (int a = 0; a < 6; ++a) D.p[6 * (size_t)j + a] = D.z[6 * (size_t)j + a] + beta * D.p[6 * (size_t)j + a];
    }
    if (threadIdx.x == 0) {
        D.cg->rz = rzn;
        D.cg->iter = st.iter + 1;
        D.cg->done = rzn <= D.tol2 * st.rz0 || st.iter + 1 >= D.maxCg ? 1 : 0;
    }
}

// ---- the trial parameters ----

__global__ __launch_bounds__(256) void mcv_ba_retract(BaDevice D) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= D.nCameras) return;
    double cam[14], x[6], out[14];
#pragma unroll
    for (int q = 0; q < 14; ++q) cam[q] = D.cams[14 * (size_t)j + q];
    if (D.active[j]) {
#pragma unroll
        for (int q = 0; q < 6; ++q) x[q] = D.x[6 * (size_t)j + q];
        ba_retract(cam, x, out);
    } else {
#pragma unroll
        for (int q = 0; q < 14; ++q) out[q] = cam[q];
    }
#pragma unroll
    for (int q = 0; q < 14; ++q) D.cams2[14 * (size_t)j + q] = out[q];
}

// ---- launches ----

static inline unsigned ba_blocks(long long n) { return (unsigned)((n + 255) / 256 > 0 ? (n + 255) / 256 : 1); }
static inline unsigned ba_seg_blocks(const BaDevice& D) { return (unsigned)D.nSeg; }
static inline unsigned ba_long_blocks(const BaDevice& D) { return (unsigned)(D.T < kBaLongBlocks ? (D.T > 0 ? D.T : 1) : kBaLongBlocks); }

void launch_ba_setup(const BaDevice& D, hipStream_t s) {
    ProfScope ps("ba_setup", s);
    int* camHas = reinterpret_cast<int*>(D.pq);   // nCameras doubles of scratch, free before the first solve
    hipLaunchKernelGGL(mcv_ba_used_obs, dim3(kBaGrid), dim3(256), 0, s, D);
    hipLaunchKernelGGL(mcv_ba_used_track, dim3(ba_blocks(D.T)), dim3(256), 0, s, D, camHas);
    hipLaunchKernelGGL(mcv_ba_active, dim3(ba_blocks(D.nCameras)), dim3(256), 0, s, D, camHas);
}

void launch_ba_cost(const BaDevice& D, const double* d_cams, const double* d_pts, hipStream_t s) {
    ProfScope ps("ba_cost", s);
    hipLaunchKernelGGL(mcv_ba_cost_seg, dim3(ba_seg_blocks(D)), dim3(kBaSegLanes), 0, s, D, d_cams, d_pts);
    hipLaunchKernelGGL(mcv_ba_cost_final, dim3(1), dim3(kBaSegLanes), 0, s, D);
}

void launch_ba_linearize(const BaDevice& D, hipStream_t s) {
    ProfScope ps("ba_linearize", s);
    hipLaunchKernelGGL(mcv_ba_lin_short, dim3(ba_blocks(D.T)), dim3(256), 0, s, D);
    hipLaunchKernelGGL(mcv_ba_lin_long, dim3(ba_long_blocks(D)), dim3(256), 0, s, D);
    hipLaunchKernelGGL(mcv_ba_lin_cam_seg, dim3(ba_seg_blocks(D)), dim3(kBaSegLanes), 0, s, D);
    hipLaunchKernelGGL(mcv_ba_lin_cam_final, dim3(ba_blocks(D.nCameras)), dim3(256), 0, s, D);
}

void launch_ba_system(const BaDevice& D, hipStream_t s) {
    ProfScope ps("ba_system", s);
    hipLaunchKernelGGL(mcv_ba_point_solve, dim3(ba_blocks(D.T)), dim3(256), 0, s, D);
    hipLaunchKernelGGL(mcv_ba_schur_seg, dim3(ba_seg_blocks(D)), dim3(kBaSegLanes), 0, s, D);
    hipLaunchKernelGGL(mcv_ba_schur_final, dim3(ba_blocks(D.nCameras)), dim3(256), 0, s, D);
    hipLaunchKernelGGL(mcv_ba_pcg_init, dim3(1), dim3(kBaSegLanes), 0, s, D);
}

void launch_ba_cg_iteration(const BaDevice& D, hipStream_t s) {
    ProfScope ps("ba_cg_iteration", s);
    hipLaunchKernelGGL(mcv_ba_point_short<0>, dim3(ba_blocks(D.T)), dim3(256), 0, s, D);
    hipLaunchKernelGGL(mcv_ba_point_long<0>, dim3(ba_long_blocks(D)), dim3(256), 0, s, D);
    hipLaunchKernelGGL(mcv_ba_wy_seg, dim3(ba_seg_blocks(D)), dim3(kBaSegLanes), 0, s, D);
    hipLaunchKernelGGL(mcv_ba_q_final, dim3(ba_blocks(D.nCameras)), dim3(256), 0, s, D);
    hipLaunchKernelGGL(mcv_ba_pcg_update, dim3(1), dim3(kBaSegLanes), 0, s, D);
}

void launch_ba_trial(const BaDevice& D, hipStream_t s) {
    {
        ProfScope ps("ba_trial_update", s);
        hipLaunchKernelGGL(mcv_ba_point_short<1>, dim3(ba_blocks(D.T)), dim3(256), 0, s, D);
        hipLaunchKernelGGL(mcv_ba_point_long<1>, dim3(ba_long_blocks(D)), dim3(256), 0, s, D);
        hipLaunchKernelGGL(mcv_ba_retract, dim3(ba_blocks(D.nCameras)), dim3(256), 0, s, D);
    }
    launch_ba_cost(D, D.cams2, D.pts2, s);
}

// ================= focal groups =================
// cvBundleAdjustFocal with focalMode 1 or 2 (FM). Every kernel above that the focal lengths do not
// change is launched as it is; the kernels here are the per-observation passes with the focal
// accumulators beside the cameras' (instantiated per mode, so the kernels above carry none of it), and
// one lane per group for what a group sums: the chain, from +0.0 over the group's cameras in ascending
// index, of those cameras' per-camera sums (each the chain of the camera's segments, as above).

// One segment with NC camera sums and NF focal sums: the first go to D.part, the others to F.partF.
template <int NC, int NF, class Fn>
__device__ __forceinline__ void baf_seg_sum(const BaDevice& D, const BaFocal& F, int seg, Fn f, double* lds) {
    double acc[NC + NF];
#pragma unroll
    for (int q = 0; q < NC + NF; ++q) acc[q] = 0.0;
    const int end = D.segEnd[seg];
    for (int i = D.segStart[seg] + (int)threadIdx.x; i < end; i += kBaSegLanes) f(D.camObs[i], acc);
    ba_block_tree<NC + NF>(acc, lds);
    if (threadIdx.x < NC) D.part[27 * (size_t)seg + threadIdx.x] = lds[threadIdx.x * kBaSegLanes];
    else if (threadIdx.x < NC + NF) F.partF[kBaFocalPart * (size_t)seg + (threadIdx.x - NC)] = lds[threadIdx.x * kBaSegLanes];
}

template <int NF>
__device__ __forceinline__ void baf_group_total(const BaDevice& D, const BaFocal& F, int g, double (&out)[NF]) {
#pragma unroll
    for (int q = 0; q < NF; ++q) out[q] = 0.0;
    for (int i = F.grpPtr[g]; i < F.grpPtr[g + 1]; ++i) {
        const int j = F.grpCam[i];
        double c[NF];
#pragma unroll
        for (int q = 0; q < NF; ++q) c[q] = 0.0;
        for (int s = D.camSegPtr[j]; s < D.camSegPtr[j + 1]; ++s) {
#pragma unroll
            for (int q = 0; q < NF; ++q) c[q] = c[q] + F.partF[kBaFocalPart * (size_t)s + q];
        }
#pragma unroll
        for (int q = 0; q < NF; ++q) out[q] = out[q] + c[q];
    }
}

// The first group of thread tid in the chain over cameras, then groups, at stride kBaSegLanes.
__device__ __forceinline__ int baf_first_group(const BaDevice& D) {
    return (int)(((unsigned)threadIdx.x + kBaSegLanes - (unsigned)(D.nCameras % kBaSegLanes)) % kBaSegLanes);
}

__global__ __launch_bounds__(256) void mcv_baf_free(BaDevice D, BaFocal F, const int* __restrict__ camHas) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= F.nG) return;
    bool has = false;
    for (int i = F.grpPtr[g]; i < F.grpPtr[g + 1]; ++i) has = has || camHas[F.grpCam[i]] != 0;
    const bool fr = has && !F.grpFixed[g];
    F.grpFree[g] = fr ? 1 : 0;
    if (fr) atomicAdd(&D.ctr[5], 1u);
}

template <int FM>
__global__ __launch_bounds__(256) void mcv_baf_u(BaDevice D, BaFocal F) {
    for (int k = blockIdx.x * 256 + threadIdx.x; k < D.n; k += gridDim.x * 256) {
        if (!D.used[k]) continue;
        const int j = D.cameraIdx[k];
        double u[2];
        ba_linearize_focal(FM, D.cams + 14 * (size_t)j, D.pts + 3 * (size_t)D.obsTrack[k], D.obs[2 * (size_t)k],
                           D.obs[2 * (size_t)k + 1], D.delta, F.grpFree[F.camGrp[j]] != 0, u);
        F.Ef[2 * (size_t)k] = u[0];
        F.Ef[2 * (size_t)k + 1] = u[1];
    }
}

template <int FM>
__global__ __launch_bounds__(kBaSegLanes) void mcv_baf_lin_cam_seg(BaDevice D, BaFocal F) {
    constexpr int NF = FM == 1 ? 2 : 4;
    __shared__ double lds[(27 + NF) * kBaSegLanes];
    baf_seg_sum<27, NF>(D, F, blockIdx.x, [&](int k, double (&acc)[27 + NF]) {
        if (!D.used[k]) return;
        double e[kBaEntry], u[2];
#pragma unroll
        for (int q = 0; q < kBaEntry; ++q) e[q] = D.E[(size_t)kBaEntry * k + q];
        u[0] = F.Ef[2 * (size_t)k];
        u[1] = F.Ef[2 * (size_t)k + 1];
        ba_acc_cam_lin(e, acc);
        ba_acc_focal_lin(FM, u, e, acc + 27);
    }, lds);
}

template <int FM>
__global__ __launch_bounds__(256) void mcv_baf_grp_lin(BaDevice D, BaFocal F) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= F.nG) return;
    constexpr int NF = FM == 1 ? 2 : 4, ND = FM == 1 ? 1 : 2;
    double acc[NF];
    baf_group_total<NF>(D, F, g, acc);
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        F.Gd[2 * (size_t)g + a] = a < ND ? acc[a % ND] : 0.0;
        F.gf[2 * (size_t)g + a] = a < ND ? -acc[ND + a % ND] : 0.0;
    }
}

template <int FM>
__global__ __launch_bounds__(kBaSegLanes) void mcv_baf_schur_seg(BaDevice D, BaFocal F) {
    constexpr int NF = FM == 1 ? 2 : 5;
    __shared__ double lds[(27 + NF) * kBaSegLanes];
    baf_seg_sum<27, NF>(D, F, blockIdx.x, [&](int k, double (&acc)[27 + NF]) {
        if (!D.used[k]) return;
        const int i = D.obsTrack[k];
        double e[kBaEntry], inv[6], tt[3], u[2];
#pragma unroll
        for (int q = 0; q < kBaEntry; ++q) e[q] = D.E[(size_t)kBaEntry * k + q];
#pragma unroll
        for (int q = 0; q < 6; ++q) inv[q] = D.Vinv[6 * (size_t)i + q];
#pragma unroll
        for (int q = 0; q < 3; ++q) tt[q] = D.t[3 * (size_t)i + q];
        u[0] = F.Ef[2 * (size_t)k];
        u[1] = F.Ef[2 * (size_t)k + 1];
        ba_acc_cam_schur(e, inv, tt, acc);
        ba_acc_focal_schur(FM, u, e, inv, tt, acc + 27);
    }, lds);
}

template <int FM>
__global__ __launch_bounds__(256) void mcv_baf_grp_schur(BaDevice D, BaFocal F) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= F.nG) return;
    constexpr int NF = FM == 1 ? 2 : 5;
    double acc[NF], sums[kBaFocalPart] = {0.0, 0.0, 0.0, 0.0, 0.0}, L[3], b[2];
    baf_group_total<NF>(D, F, g, acc);
#pragma unroll
    for (int q = 0; q < NF; ++q) sums[q] = acc[q];
    const double Gd[2] = {F.Gd[2 * (size_t)g], F.Gd[2 * (size_t)g + 1]};
    const double gf[2] = {F.gf[2 * (size_t)g], F.gf[2 * (size_t)g + 1]};
    if (!ba_focal_block(FM, Gd, gf, sums, D.lambda, L, b)) atomicOr(&D.ctr[3], 1u);
#pragma unroll
    for (int q = 0; q < 3; ++q) F.Lf[3 * (size_t)g + q] = L[q];
    F.bf[2 * (size_t)g] = b[0];
    F.bf[2 * (size_t)g + 1] = b[1];
}

template <int FM>
__device__ __forceinline__ void baf_precondition(const BaFocal& F, int g, const double (&r)[2], double (&z)[2]) {
    const double L[3] = {F.Lf[3 * (size_t)g], F.Lf[3 * (size_t)g + 1], F.Lf[3 * (size_t)g + 2]};
    ba_focal_solve(FM, L, r, z);
}

template <int FM>
__global__ __launch_bounds__(kBaSegLanes) void mcv_baf_pcg_init(BaDevice D, BaFocal F) {
    __shared__ double lds[kBaSegLanes];
    const bool failed = D.ctr[3] != 0;
    double acc = 0.0;
    if (!failed) {
        for (int j = threadIdx.x; j < D.nCameras; j += kBaSegLanes) {
            double r[6], z[6];
#pragma unroll
            for (int a = 0; a < 6; ++a) r[a] = D.b[6 * (size_t)j + a];
            ba_precondition(D, j, r, z);
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                D.x[6 * (size_t)j + a] = 0.0;
                D.r[6 * (size_t)j + a] = r[a];
                D.z[6 * (size_t)j + a] = z[a];
                D.p[6 * (size_t)j + a] = z[a];
            }
            acc = acc + ba_dot6(r, z);
        }
        for (int g = baf_first_group(D); g < F.nG; g += kBaSegLanes) {
            double r[2], z[2];
#pragma unroll
            for (int a = 0; a < 2; ++a) r[a] = F.bf[2 * (size_t)g + a];
            baf_precondition<FM>(F, g, r, z);
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                F.xf[2 * (size_t)g + a] = 0.0;
                F.rf[2 * (size_t)g + a] = r[a];
                F.zf[2 * (size_t)g + a] = z[a];
                F.pf[2 * (size_t)g + a] = z[a];
            }
            acc = acc + ba_focal_dot(FM, r, z);
        }
    }
    const double rz = ba_block_total(acc, lds);
    if (threadIdx.x == 0) {
        const bool bad = failed || !ba_finite(rz);
        D.cg->rz = rz;
        D.cg->rz0 = rz;
        D.cg->iter = 0;
        D.cg->failed = bad ? 1 : 0;
        D.cg->done = bad || rz <= D.tol2 * rz || D.maxCg <= 0 ? 1 : 0;
    }
}

template <int MODE, int FM>
__device__ __forceinline__ void baf_point_entry(const BaDevice& D, const BaFocal& F, int k, double* acc) {
    if (!D.used[k]) return;
    double e[18], v[6], u[2], vf[2];
#pragma unroll
    for (int q = 0; q < 18; ++q) e[q] = D.E[(size_t)kBaEntry * k + q];
    const int j = D.cameraIdx[k];
    const double* src = (MODE == 0 ? D.p : D.x) + 6 * (size_t)j;
#pragma unroll
    for (int q = 0; q < 6; ++q) v[q] = src[q];
    const double* srcf = (MODE == 0 ? F.pf : F.xf) + 2 * (size_t)F.camGrp[j];
    vf[0] = srcf[0];
    vf[1] = srcf[1];
    u[0] = F.Ef[2 * (size_t)k];
    u[1] = F.Ef[2 * (size_t)k + 1];
    ba_acc_point_wtp_focal(FM, e, u, v, vf, acc);
}

template <int MODE, int FM>
__global__ __launch_bounds__(256) void mcv_baf_point_short(BaDevice D, BaFocal F) {
    if (MODE == 0 && D.cg->done) return;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= D.T) return;
    if (!D.trackUsed[t]) {
        if (MODE == 1) {
#pragma unroll
            for (int q = 0; q < 3; ++q) D.pts2[3 * (size_t)t + q] = D.pts[3 * (size_t)t + q];
        }
        return;
    }
    const int o0 = D.offsets[t], R = D.offsets[t + 1] - o0;
    if (R > kBaShortMax) return;
    double acc[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < R; ++i) baf_point_entry<MODE, FM>(D, F, o0 + i, acc);
    ba_point_store<MODE>(D, t, acc);
}

template <int MODE, int FM>
__global__ __launch_bounds__(256) void mcv_baf_point_long(BaDevice D, BaFocal F) {
    if (MODE == 0 && D.cg->done) return;
    const int lane = threadIdx.x & 63, nLong = (int)D.ctr[0];
    for (int w = blockIdx.x * 4 + (threadIdx.x >> 6); w < nLong; w += gridDim.x * 4) {
        const int t = D.longList[w], o0 = D.offsets[t];
        double acc[3];
        ba_wave_sum<3>(o0, D.offsets[t + 1] - o0, lane, [&](int k, double (&a)[3]) { baf_point_entry<MODE, FM>(D, F, k, a); }, acc);
        if (lane == 0) ba_point_store<MODE>(D, t, acc);
    }
}

template <int FM>
__global__ __launch_bounds__(kBaSegLanes) void mcv_baf_wy_seg(BaDevice D, BaFocal F) {
    constexpr int NF = FM == 1 ? 1 : 2;
    __shared__ double lds[(6 + NF) * kBaSegLanes];
    if (D.cg->done) return;
    const int j = D.segCam[blockIdx.x];
    double p[6], pf[2];
#pragma unroll
    for (int q = 0; q < 6; ++q) p[q] = D.p[6 * (size_t)j + q];
    pf[0] = F.pf[2 * (size_t)F.camGrp[j]];
    pf[1] = F.pf[2 * (size_t)F.camGrp[j] + 1];
    baf_seg_sum<6, NF>(D, F, blockIdx.x, [&](int k, double (&acc)[6 + NF]) {
        if (!D.used[k]) return;
        double e[18], y[3], u[2];
#pragma unroll
        for (int q = 0; q < 18; ++q) e[q] = D.E[(size_t)kBaEntry * k + q];
#pragma unroll
        for (int q = 0; q < 3; ++q) y[q] = D.y[3 * (size_t)D.obsTrack[k] + q];
        u[0] = F.Ef[2 * (size_t)k];
        u[1] = F.Ef[2 * (size_t)k + 1];
        ba_acc_cam_wy_focal(FM, e, u, y, p, pf, acc);
    }, lds);
}

// q of a group and its share of p.q
template <int FM>
__global__ __launch_bounds__(256) void mcv_baf_grp_q(BaDevice D, BaFocal F) {
    if (D.cg->done) return;
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= F.nG) return;
    constexpr int NF = FM == 1 ? 1 : 2;
    double acc[NF], sums[2] = {0.0, 0.0}, q[2];
    baf_group_total<NF>(D, F, g, acc);
#pragma unroll
    for (int a = 0; a < NF; ++a) sums[a] = acc[a];
    const double Gd[2] = {F.Gd[2 * (size_t)g], F.Gd[2 * (size_t)g + 1]};
    const double pf[2] = {F.pf[2 * (size_t)g], F.pf[2 * (size_t)g + 1]};
    ba_focal_q(FM, Gd, D.lambda, pf, sums, q);
    F.qf[2 * (size_t)g] = q[0];
    F.qf[2 * (size_t)g + 1] = q[1];
    F.pqf[g] = ba_focal_dot(FM, pf, q);
}

template <int FM>
__global__ __launch_bounds__(kBaSegLanes) void mcv_baf_pcg_update(BaDevice D, BaFocal F) {
    __shared__ double lds[kBaSegLanes];
    const BaCgState st = *D.cg;   // read by every thread before thread 0 writes it below (barriers between)
    if (st.done) return;
    const int g0 = baf_first_group(D);
    double acc = 0.0;
    for (int j = threadIdx.x; j < D.nCameras; j += kBaSegLanes) acc = acc + D.pq[j];
    for (int g = g0; g < F.nG; g += kBaSegLanes) acc = acc + F.pqf[g];
    const double pq = ba_block_total(acc, lds);
    const double alpha = st.rz / pq;
    if (!(pq > 0.0) || !ba_finite(alpha)) {
        if (threadIdx.x == 0) {
            D.cg->failed = 1;
            D.cg->done = 1;
        }
        return;
    }
    acc = 0.0;
    for (int j = threadIdx.x; j < D.nCameras; j += kBaSegLanes) {
        double r[6], z[6];
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            D.x[6 * (size_t)j + a] = D.x[6 * (size_t)j + a] + alpha * D.p[6 * (size_t)j + a];
            r[a] = D.r[6 * (size_t)j + a] - alpha * D.q[6 * (size_t)j + a];
            D.r[6 * (size_t)j + a] = r[a];
        }
        ba_precondition(D, j, r, z);
#pragma unroll
        for (int a = 0; a < 6; ++a) D.z[6 * (size_t)j + a] = z[a];
        acc = acc + ba_dot6(r, z);
    }
    for (int g = g0; g < F.nG; g += kBaSegLanes) {
        double r[2], z[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            F.xf[2 * (size_t)g + a] = F.xf[2 * (size_t)g + a] + alpha * F.pf[2 * (size_t)g + a];
            r[a] = F.rf[2 * (size_t)g + a] - alpha * F.qf[2 * (size_t)g + a];
            F.rf[2 * (size_t)g + a] = r[a];
        }
        baf_precondition<FM>(F, g, r, z);
#pragma unroll
        for (int a = 0; a < 2; ++a) F.zf[2 * (size_t)g + a] = z[a];
        acc = acc + ba_focal_dot(FM, r, z);
    }
    const double rzn = ba_block_total(acc, lds);
    if (!ba_finite(rzn)) {
        if (threadIdx.x == 0) {
            D.cg->failed = 1;
            D.cg->done = 1;
        }
        return;
    }
    const double beta = rzn / st.rz;
    for (int j = threadIdx.x; j < D.nCameras; j += kBaSegLanes) {
#pragma unroll
        for (int a = 0; a < 6; ++a) D.p[6 * (size_t)j + a] = D.z[6 * (size_t)j + a] + beta * D.p[6 * (size_t)j + a];
    }
    for (int g = g0; g < F.nG; g += kBaSegLanes) {
#pragma unroll
        for (int a = 0; a < 2; ++a) F.pf[2 * (size_t)g + a] = F.zf[2 * (size_t)g + a] + beta * F.pf[2 * (size_t)g + a];
    }
    if (threadIdx.x == 0) {
        D.cg->rz = rzn;
        D.cg->iter = st.iter + 1;
        D.cg->done = rzn <= D.tol2 * st.rz0 || st.iter + 1 >= D.maxCg ? 1 : 0;
    }
}

// The trial focal lengths, over mcv_ba_retract's copies; a value that is not finite and positive
// raises the flag that rejects the trial.
template <int FM>
__global__ __launch_bounds__(256) void mcv_baf_focal(BaDevice D, BaFocal F) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= D.nCameras) return;
    const int g = F.camGrp[j];
    if (!F.grpFree[g]) return;
    const double f[2] = {D.cams[14 * (size_t)j + 12], D.cams[14 * (size_t)j + 13]};
    const double xf[2] = {F.xf[2 * (size_t)g], F.xf[2 * (size_t)g + 1]};
    double out[2];
    if (!ba_focal_update(FM, f, xf, out)) atomicOr(&D.ctr[4], 1u);
    D.cams2[14 * (size_t)j + 12] = out[0];
    D.cams2[14 * (size_t)j + 13] = out[1];
}

#define MCV_BAF_LAUNCH(kernel, grid, block, ...)                                               \
    do {                                                                                       \
        if (F.fm == 1) hipLaunchKernelGGL(HIP_KERNEL_NAME(kernel<1>), grid, block, 0, s, __VA_ARGS__); \
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(kernel<2>), grid, block, 0, s, __VA_ARGS__);   \
    } while (0)
#define MCV_BAF_LAUNCH_M(kernel, M, grid, block, ...)                                          \
    do {                                                                                       \
        if (F.fm == 1) hipLaunchKernelGGL(HIP_KERNEL_NAME(kernel<M, 1>), grid, block, 0, s, __VA_ARGS__); \
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(kernel<M, 2>), grid, block, 0, s, __VA_ARGS__); \
    } while (0)

void launch_baf_setup(const BaDevice& D, const BaFocal& F, hipStream_t s) {
    launch_ba_setup(D, s);
    ProfScope ps("baf_setup", s);
    hipLaunchKernelGGL(mcv_baf_free, dim3(ba_blocks(F.nG)), dim3(256), 0, s, D, F, reinterpret_cast<const int*>(D.pq));
}

void launch_baf_linearize(const BaDevice& D, const BaFocal& F, hipStream_t s) {
    ProfScope ps("baf_linearize", s);
    hipLaunchKernelGGL(mcv_ba_lin_short, dim3(ba_blocks(D.T)), dim3(256), 0, s, D);
    hipLaunchKernelGGL(mcv_ba_lin_long, dim3(ba_long_blocks(D)), dim3(256), 0, s, D);
    MCV_BAF_LAUNCH(mcv_baf_u, dim3(kBaGrid), dim3(256), D, F);
    MCV_BAF_LAUNCH(mcv_baf_lin_cam_seg, dim3(ba_seg_blocks(D)), dim3(kBaSegLanes), D, F);
    hipLaunchKernelGGL(mcv_ba_lin_cam_final, dim3(ba_blocks(D.nCameras)), dim3(256), 0, s, D);
    MCV_BAF_LAUNCH(mcv_baf_grp_lin, dim3(ba_blocks(F.nG)), dim3(256), D, F);
}

void launch_baf_system(const BaDevice& D, const BaFocal& F, hipStream_t s) {
    ProfScope ps("baf_system", s);
    hipLaunchKernelGGL(mcv_ba_point_solve, dim3(ba_blocks(D.T)), dim3(256), 0, s, D);
    MCV_BAF_LAUNCH(mcv_baf_schur_seg, dim3(ba_seg_blocks(D)), dim3(kBaSegLanes), D, F);
    hipLaunchKernelGGL(mcv_ba_schur_final, dim3(ba_blocks(D.nCameras)), dim3(256), 0, s, D);
    MCV_BAF_LAUNCH(mcv_baf_grp_schur, dim3(ba_blocks(F.nG)), dim3(256), D, F);
    MCV_BAF_LAUNCH(mcv_baf_pcg_init, dim3(1), dim3(kBaSegLanes), D, F);
}

void launch_baf_cg_iteration(const BaDevice& D, const BaFocal& F, hipStream_t s) {
    ProfScope ps("baf_cg_iteration", s);
    MCV_BAF_LAUNCH_M(mcv_baf_point_short, 0, dim3(ba_blocks(D.T)), dim3(256), D, F);
    MCV_BAF_LAUNCH_M(mcv_baf_point_long, 0, dim3(ba_long_blocks(D)), dim3(256), D, F);
    MCV_BAF_LAUNCH(mcv_baf_wy_seg, dim3(ba_seg_blocks(D)), dim3(kBaSegLanes), D, F);
    hipLaunchKernelGGL(mcv_ba_q_final, dim3(ba_blocks(D.nCameras)), dim3(256), 0, s, D);
    MCV_BAF_LAUNCH(mcv_baf_grp_q, dim3(ba_blocks(F.nG)), dim3(256), D, F);
    MCV_BAF_LAUNCH(mcv_baf_pcg_update, dim3(1), dim3(kBaSegLanes), D, F);
}

void launch_baf_trial(const BaDevice& D, const BaFocal& F, hipStream_t s) {
    {
        ProfScope ps("baf_trial_update", s);
        MCV_BAF_LAUNCH_M(mcv_baf_point_short, 1, dim3(ba_blocks(D.T)), dim3(256), D, F);
        MCV_BAF_LAUNCH_M(mcv_baf_point_long, 1, dim3(ba_long_blocks(D)), dim3(256), D, F);
        hipLaunchKernelGGL(mcv_ba_retract, dim3(ba_blocks(D.nCameras)), dim3(256), 0, s, D);
        MCV_BAF_LAUNCH(mcv_baf_focal, dim3(ba_blocks(D.nCameras)), dim3(256), D, F);
    }
    launch_ba_cost(D, D.cams2, D.pts2, s);
}

}  // namespace mcv
