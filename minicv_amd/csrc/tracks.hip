// tracks.hip — gfx950 kernels of track building: the connected components of the match graph, the
// multi-view consistency filter and the track CSR cvTriangulateTracks consumes. All
// integer arithmetic; every output is defined exactly and independent of the order of the edges.
//
//   mcv_trk_init      lane per node: parent = self, size = 0, touched = 0, trk = 0
//   mcv_trk_hook      lane per kept edge: lock-free union, the larger root CASed under the smaller, so
//                     a component's root ends as its smallest node whatever order the hardware takes
//   mcv_trk_flatten   lane per node: chase to the root (in place), count the component at the root
//   mcv_trk_sums<M> / mcv_trk_scan / mcv_trk_place<M>   exclusive scan over the nodes in id order of a
//                     packed (count << 32 | nodes) value. M = 0: the candidate components (2 <= size <=
//                     min(cap, nImages)) get a candidate index and a slot range, and the components
//                     that need no sort are counted (oversize; size > nImages: a conflict by
//                     pigeonhole; size 1: short). M = 1: the surviving components get their track index
//                     and observation offset
//   mcv_trk_scatter   lane per node: into its component's slot range through the root's cursor
//   mcv_trk_short     lane per candidate of at most kTrkShortMax nodes: insertion sort by node id, two
//                     neighbours of one image = conflict; longer candidates are queued
//   mcv_trk_long      workgroup per queued candidate: bitonic sort of up to 4096 ids in LDS (16 KiB)
//   mcv_trk_copy      lane per slot: cameraIdx / featureIdx of the kept tracks; lane per node:
//                     trackOfFeature
//
// Words that several workgroups read and write inside one launch (parent[] in mcv_trk_hook) are only
// touched by agent-scope atomics: a CU's L1 is never refreshed by another CU's stores.
#include "minicv_native.h"
#include "kernels.h"
#include "plan.h"

#include <climits>

namespace mcv {

typedef unsigned long long u64;

static_assert(MCV_MAX_TRACK_LEN == 4096, "mcv_trk_long sorts one component in 16 KiB of LDS");
static_assert(kTrkScanItems == 256 * 8, "eight nodes per thread of the scan blocks");

__device__ __forceinline__ int trk_aload(const int* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void trk_astore(int* p, int v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The i with base[i] <= g < base[i + 1]; g < base[nImages].
__device__ __forceinline__ int trk_image_of(const int* __restrict__ base, int nImages, int g) {
    int lo = 0, hi = nImages - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (base[mid + 1] > g) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

__global__ __launch_bounds__(256) void mcv_trk_init(int nNodes, int* __restrict__ parent, int* __restrict__ size,
                                                    int* __restrict__ trk, uint8_t* __restrict__ touched) {
    for (long long g = blockIdx.x * 256 + threadIdx.x; g < nNodes; g += (long long)gridDim.x * 256) {
        parent[g] = (int)g;
        size[g] = 0;
        trk[g] = 0;
        touched[g] = 0;
    }
}

// Root of x with path splitting. Every value parent[y] ever holds is <= y and a node of y's tree, so
// the walk descends strictly and ends within x steps; the bound only guards that invariant.
__device__ __forceinline__ int trk_find(int* parent, int x, int nNodes) {
    int p = trk_aload(parent + x);
    for (int steps = 0; p != x; ++steps) {
        if (steps > nNodes || p > x) return -1;
        const int gp = trk_aload(parent + p);
        if (gp != p) trk_astore(parent + x, gp);
        x = p;
        p = gp;
    }
    return x;
}

// An ancestor of x by plain loads, which may hit lines of this CU's L1 that other CUs have rewritten
// since: every value parent[y] ever holds is an ancestor of y (or y), so a stale one is an older
// ancestor. Two nodes with a common ancestor are in one tree for good: most edges of a dense match
// graph end here, on L1 hits, and never read the contended root words through to L2.
__device__ __forceinline__ int trk_ancestor(const int* parent, int x) {
    int p = parent[x];
    while (p < x) {
        x = p;
        p = parent[x];
    }
    return x;
}

__global__ __launch_bounds__(256) void mcv_trk_hook(const int* __restrict__ edges, long long nEdges, int nNodes,
                                                    int* parent, uint8_t* touched, u64* ctr) {
    for (long long k = blockIdx.x * 256 + threadIdx.x; k < nEdges; k += (long long)gridDim.x * 256) {
        int u = edges[2 * k], v = edges[2 * k + 1];
        touched[u] = 1;
        touched[v] = 1;
        if (u == v) continue;
        u = trk_ancestor(parent, u);
        v = trk_ancestor(parent, v);
        if (u == v) continue;
        bool done = false;
        // A failed CAS means another lane hooked that root in between; the successful hooks of a call
        // number at most nNodes - 1, so neither do the retries of one edge.
        for (int tries = 0; tries < nNodes && !done; ++tries) {
            u = trk_find(parent, u, nNodes);
            v = trk_find(parent, v, nNodes);
            if (u < 0 || v < 0) break;
            if (u == v) {
                done = true;
                break;
            }
            const int hi = u > v ? u : v, lo = u > v ? v : u;
            done = atomicCAS(parent + hi, hi, lo) == hi;
            u = hi;
            v = lo;
        }
        if (!done) atomicOr(ctr + 3, 1ull);
    }
}

__global__ __launch_bounds__(256) void mcv_trk_flatten(int nNodes, int* parent, const uint8_t* __restrict__ touched,
                                                       int* __restrict__ size, u64* ctr) {
    for (long long g0 = blockIdx.x * 256; g0 < nNodes; g0 += (long long)gridDim.x * 256) {
        const long long g = g0 + threadIdx.x;
        int r = -1;
        if (g < nNodes && touched[g]) {
            // Other lanes store roots over parent[] meanwhile; whichever value a load sees, old or
            // new, is an ancestor of its node with a smaller id, so the walk still ends at the root.
            r = (int)g;
            int p = parent[r], steps = 0;
            while (p != r && steps <= nNodes) {
                r = p;
                p = parent[r];
                ++steps;
            }
            if (p != r) {
                atomicOr(ctr + 3, 2ull);
                r = -1;
            } else {
                parent[g] = r;
            }
        }
        // one add per distinct root among the wave's lanes: neighbouring features often share a big
        // component, and 64 adds to one word serialise
        bool open = r >= 0;
        while (true) {
            const u64 m = __ballot(open);
            if (!m) break;
            const int leader = __ffsll((long long)m) - 1;
            const int r0 = __shfl(r, leader, 64);
            const bool same = open && r == r0;
            const u64 ms = __ballot(same);
            if ((int)(threadIdx.x & 63) == leader) atomicAdd(size + r0, (int)__popcll(ms));
            open = open && !same;
        }
    }
}

struct TrkScan {
    const int* parent;
    const int* size;
    int* trk;
    int* cursor;
    int* candList;
    int* trackOffsets;
    int nNodes, maxLen;   // maxLen = min(MCV_MAX_TRACK_LEN, nImages)
};

// M = 0: (1 << 32 | size) at the root of a candidate. M = 1: (1 << 32 | size) at the root of a survivor.
template <int M>
__device__ __forceinline__ u64 trk_value(const TrkScan& a, int g) {
    if (M == 0) {
        if (a.parent[g] != g) return 0;
        const int s = a.size[g];
        return s >= 2 && s <= a.maxLen ? (1ull << 32 | (u64)s) : 0;
    }
    const int s = a.trk[g];
    return s > 0 ? (1ull << 32 | (u64)s) : 0;
}

template <int M>
__global__ __launch_bounds__(256) void mcv_trk_sums(TrkScan a, u64* __restrict__ blockSums, u64* ctr) {
    __shared__ u64 w[4];
    const long long b0 = (long long)blockIdx.x * kTrkScanItems;
    u64 sum = 0;
    int over = 0, conf = 0, shrt = 0;
    for (int j = 0; j < 8; ++j) {
        const long long g = b0 + j * 256 + threadIdx.x;
        if (g >= a.nNodes) break;
        sum += trk_value<M>(a, (int)g);
        if (M == 0 && a.parent[g] == g) {   // the components that need no sort (an untouched node has size 0)
            const int s = a.size[g];
            if (s > MCV_MAX_TRACK_LEN) over += 1;
            else if (s > a.maxLen) conf += 1;
            else if (s == 1) shrt += 1;
        }
    }
    for (int o = 32; o >= 1; o >>= 1) {
        sum += __shfl_xor(sum, o, 64);
        if (M == 0) {
            over += __shfl_xor(over, o, 64);
            conf += __shfl_xor(conf, o, 64);
            shrt += __shfl_xor(shrt, o, 64);
        }
    }
    if ((threadIdx.x & 63) == 0) {
        w[threadIdx.x >> 6] = sum;
        if (M == 0) {
            if (over) atomicAdd(ctr + 0, (u64)over);
            if (conf) atomicAdd(ctr + 1, (u64)conf);
            if (shrt) atomicAdd(ctr + 2, (u64)shrt);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) blockSums[blockIdx.x] = w[0] + w[1] + w[2] + w[3];
}

// Exclusive scan of nb block sums in one block, in place (chunks of kTrkScanChunk, fixed order); *total = the sum.
__global__ __launch_bounds__(kTrkScanChunk) void mcv_trk_scan(u64* __restrict__ sums, int nb,
                                                               u64* __restrict__ total) {
    __shared__ u64 sh[kTrkScanChunk];
    __shared__ u64 carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int b0 = 0; b0 < nb; b0 += kTrkScanChunk) {
        const int i = b0 + threadIdx.x;
        const u64 v = i < nb ? sums[i] : 0;
        sh[threadIdx.x] = v;
        __syncthreads();
        for (int o = 1; o < kTrkScanChunk; o <<= 1) {
            const u64 t = (int)threadIdx.x >= o ? sh[threadIdx.x - o] : 0;
            __syncthreads();
            sh[threadIdx.x] += t;
            __syncthreads();
        }
        if (i < nb) sums[i] = carry + sh[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == kTrkScanChunk - 1) carry += sh[kTrkScanChunk - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

template <int M>
__global__ __launch_bounds__(256) void mcv_trk_place(TrkScan a, const u64* __restrict__ blockOff) {
    __shared__ u64 sh[256];
    const long long g0 = (long long)blockIdx.x * kTrkScanItems + threadIdx.x * 8;   // eight consecutive nodes
    u64 v[8], mine = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        v[j] = g0 + j < a.nNodes ? trk_value<M>(a, (int)(g0 + j)) : 0;
        mine += v[j];
    }
    sh[threadIdx.x] = mine;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const u64 t = (int)threadIdx.x >= o ? sh[threadIdx.x - o] : 0;
        __syncthreads();
        sh[threadIdx.x] += t;
        __syncthreads();
    }
    u64 pre = blockOff[blockIdx.x] + sh[threadIdx.x] - mine;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const long long g = g0 + j;
        if (g >= a.nNodes) break;
        if (M == 0) {
            if (v[j]) {
                a.candList[pre >> 32] = (int)g;
                a.cursor[g] = (int)(unsigned int)pre;
            }
        } else {
            if (v[j]) a.trackOffsets[pre >> 32] = (int)(unsigned int)pre;
            a.trk[g] = v[j] ? (int)(pre >> 32) : -1;
        }
        pre += v[j];
        if (M == 1 && g == a.nNodes - 1) a.trackOffsets[pre >> 32] = (int)(unsigned int)pre;   // offsets[T] = nObs
    }
}

__global__ __launch_bounds__(256) void mcv_trk_scatter(int nNodes, int maxLen, const int* __restrict__ parent,
                                                       const uint8_t* __restrict__ touched,
                                                       const int* __restrict__ size, int* cursor,
                                                       int* __restrict__ slots) {
    for (long long g = blockIdx.x * 256 + threadIdx.x; g < nNodes; g += (long long)gridDim.x * 256) {
        if (!touched[g]) continue;
        const int r = parent[g], s = size[r];
        if (s >= 2 && s <= maxLen) slots[atomicAdd(cursor + r, 1)] = (int)g;
    }
}

// The verdict on a sorted candidate: 1 conflict, 2 short, 0 a track.
__device__ __forceinline__ void trk_settle(bool conflict, int s, int minLength, int root, int* __restrict__ trk,
                                           int& conf, int& shrt) {
    if (conflict) conf += 1;
    else if (s < minLength) shrt += 1;
    else trk[root] = s;
}

__global__ __launch_bounds__(256) void mcv_trk_short(const int* __restrict__ candList, const int* __restrict__ size,
                                                     const int* __restrict__ cursor, const int* __restrict__ base,
                                                     int nImages, int minLength, int* slots, int* __restrict__ trk,
                                                     int* __restrict__ longList, u64* ctr) {
    const long long nCand = (long long)(ctr[4] >> 32);
    int conf = 0, shrt = 0;
    for (long long c = blockIdx.x * 256 + threadIdx.x; c < nCand; c += (long long)gridDim.x * 256) {
        const int r = candList[c], s = size[r];
        if (s > kTrkShortMax) {
            longList[atomicAdd(ctr + 6, 1ull)] = (int)c;
            continue;
        }
        int* m = slots + (cursor[r] - s);   // the scatter left the cursor at the range's end
        for (int i = 1; i < s; ++i) {
            const int x = m[i];
            int j = i - 1;
            while (j >= 0 && m[j] > x) {
                m[j + 1] = m[j];
                --j;
            }
            m[j + 1] = x;
        }
        bool conflict = false;
        int end = base[trk_image_of(base, nImages, m[0]) + 1];   // the first node of the next image
        for (int i = 1; i < s && !conflict; ++i) {
            if (m[i] < end) conflict = true;
            else end = base[trk_image_of(base, nImages, m[i]) + 1];
        }
        trk_settle(conflict, s, minLength, r, trk, conf, shrt);
    }
    for (int o = 32; o >= 1; o >>= 1) {
        conf += __shfl_xor(conf, o, 64);
        shrt += __shfl_xor(shrt, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (conf) atomicAdd(ctr + 1, (u64)conf);
        if (shrt) atomicAdd(ctr + 2, (u64)shrt);
    }
}

__global__ __launch_bounds__(256) void mcv_trk_long(const int* __restrict__ candList, const int* __restrict__ longList,
                                                    const int* __restrict__ size, const int* __restrict__ cursor,
                                                    const int* __restrict__ base, int nImages, int minLength,
                                                    int* slots, int* __restrict__ trk, u64* ctr) {
    __shared__ int ids[MCV_MAX_TRACK_LEN];
    const int nLong = (int)ctr[6];
    for (int q = blockIdx.x; q < nLong; q += gridDim.x) {
        const int r = candList[longList[q]], s = size[r];   // kTrkShortMax < s <= MCV_MAX_TRACK_LEN
        int* m = slots + (cursor[r] - s);
        int P = 64;
        while (P < s) P <<= 1;
        for (int i = threadIdx.x; i < P; i += 256) ids[i] = i < s ? m[i] : INT_MAX;
        __syncthreads();
        for (int k = 2; k <= P; k <<= 1)
            for (int j = k >> 1; j >= 1; j >>= 1) {
                for (int i = threadIdx.x; i < P; i += 256) {
                    const int l = i ^ j;
                    if (l > i) {
                        const int x = ids[i], y = ids[l];
                        if ((x > y) == ((i & k) == 0)) {
                            ids[i] = y;
                            ids[l] = x;
                        }
                    }
                }
                __syncthreads();
            }
        int conflict = 0;
        for (int i = threadIdx.x; i < s; i += 256) {
            m[i] = ids[i];
            if (i + 1 < s && ids[i + 1] < base[trk_image_of(base, nImages, ids[i]) + 1]) conflict = 1;
        }
        conflict = __syncthreads_or(conflict);   // also: ids is rewritten by the next candidate
        if (threadIdx.x == 0) {
            int conf = 0, shrt = 0;
            trk_settle(conflict != 0, s, minLength, r, trk, conf, shrt);
            if (conf) atomicAdd(ctr + 1, 1ull);
            if (shrt) atomicAdd(ctr + 2, 1ull);
        }
    }
}

__global__ __launch_bounds__(256) void mcv_trk_copy(int nNodes, const int* __restrict__ parent,
                                                    const int* __restrict__ size, const int* __restrict__ cursor,
                                                    const int* __restrict__ trk, const int* __restrict__ slots,
                                                    const int* __restrict__ base, int nImages,
                                                    const int* __restrict__ trackOffsets, int* __restrict__ cameraIdx,
                                                    int* __restrict__ featureIdx, int* __restrict__ trackOfFeature,
                                                    const u64* __restrict__ ctr) {
    const long long nSlots = (long long)(unsigned int)ctr[4];
    for (long long pos = blockIdx.x * 256 + threadIdx.x; pos < nSlots; pos += (long long)gridDim.x * 256) {
        const int g = slots[pos], r = parent[g], t = trk[r];
        if (t < 0) continue;
        const long long o = (long long)trackOffsets[t] + (pos - (cursor[r] - size[r]));
        const int img = trk_image_of(base, nImages, g);
        cameraIdx[o] = img;
        featureIdx[o] = g - base[img];
    }
    if (trackOfFeature)
        for (long long g = blockIdx.x * 256 + threadIdx.x; g < nNodes; g += (long long)gridDim.x * 256)
            trackOfFeature[g] = trk[parent[g]];   // an untouched node is its own root, and no track
}

static unsigned trk_grid(long long n) {
    const long long b = (n + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > kTrkGrid ? kTrkGrid : b));
}

void launch_build_tracks(const TrkDevice& D, hipStream_t s) {
    const int maxLen = D.nImages < MCV_MAX_TRACK_LEN ? D.nImages : MCV_MAX_TRACK_LEN;
    const unsigned nodeGrid = trk_grid(D.nNodes), slotGrid = trk_grid(D.slotCap);
    const int nb = (int)(((long long)D.nNodes + kTrkScanItems - 1) / kTrkScanItems);
    TrkScan a{D.parent, D.size, D.trk, D.cursor, D.candList, D.trackOffsets, D.nNodes, maxLen};
    {
        ProfScope ps("trk_init", s);
        hipLaunchKernelGGL(mcv_trk_init, dim3(nodeGrid), dim3(256), 0, s, D.nNodes, D.parent, D.size, D.trk,
                           D.touched);
    }
    {
        ProfScope ps("trk_hook", s);
        hipLaunchKernelGGL(mcv_trk_hook, dim3(trk_grid(D.nEdges)), dim3(256), 0, s, D.edges, D.nEdges, D.nNodes,
                           D.parent, D.touched, D.ctr);
    }
    {
        ProfScope ps("trk_flatten", s);
        hipLaunchKernelGGL(mcv_trk_flatten, dim3(nodeGrid), dim3(256), 0, s, D.nNodes, D.parent, D.touched, D.size,
                           D.ctr);
    }
    {
        ProfScope ps("trk_layout", s);
        hipLaunchKernelGGL(mcv_trk_sums<0>, dim3(nb), dim3(256), 0, s, a, D.blockSums, D.ctr);
        hipLaunchKernelGGL(mcv_trk_scan, dim3(1), dim3(kTrkScanChunk), 0, s, D.blockSums, nb, D.ctr + 4);
        hipLaunchKernelGGL(mcv_trk_place<0>, dim3(nb), dim3(256), 0, s, a, D.blockSums);
    }
    {
        ProfScope ps("trk_scatter", s);
        hipLaunchKernelGGL(mcv_trk_scatter, dim3(nodeGrid), dim3(256), 0, s, D.nNodes, maxLen, D.parent, D.touched,
                           D.size, D.cursor, D.slots);
    }
    {
        ProfScope ps("trk_short", s);
        hipLaunchKernelGGL(mcv_trk_short, dim3(trk_grid(D.slotCap / 2)), dim3(256), 0, s, D.candList, D.size,
                           D.cursor, D.base, D.nImages, D.minLength, D.slots, D.trk, D.longList, D.ctr);
    }
    {
        // the queue's length stays on the device: a fixed grid strides over it
        const int longCap = D.slotCap / kTrkShortMax + 1;
        ProfScope ps("trk_long", s);
        hipLaunchKernelGGL(mcv_trk_long, dim3(longCap < kTrkGrid ? longCap : kTrkGrid), dim3(256), 0, s, D.candList,
                           D.longList, D.size, D.cursor, D.base, D.nImages, D.minLength, D.slots, D.trk, D.ctr);
    }
    {
        ProfScope ps("trk_compact", s);
        hipLaunchKernelGGL(mcv_trk_sums<1>, dim3(nb), dim3(256), 0, s, a, D.blockSums, D.ctr);
        hipLaunchKernelGGL(mcv_trk_scan, dim3(1), dim3(kTrkScanChunk), 0, s, D.blockSums, nb, D.ctr + 5);
        hipLaunchKernelGGL(mcv_trk_place<1>, dim3(nb), dim3(256), 0, s, a, D.blockSums);
    }
    {
        ProfScope ps("trk_copy", s);
        const unsigned g = D.trackOfFeature && nodeGrid > slotGrid ? nodeGrid : slotGrid;
        hipLaunchKernelGGL(mcv_trk_copy, dim3(g), dim3(256), 0, s, D.nNodes, D.parent, D.size, D.cursor, D.trk,
                           D.slots, D.base, D.nImages, D.trackOffsets, D.cameraIdx, D.featureIdx, D.trackOfFeature,
                           D.ctr);
    }
}

}  // namespace mcv
