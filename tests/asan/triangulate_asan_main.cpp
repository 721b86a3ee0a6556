// Stand-alone sanitizer program for the host side of track triangulation (triangulate_ref.h): the
// CSR checks, the dedupe and the pair loop on empty tracks, single-ray tracks and a track at the
// cap. Built by tests/test_triangulate.py with -fsanitize=address,undefined and run as a process of
// its own; every array is allocated at its exact size so an index past an end is caught.
#include "triangulate_ref.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace mcv;

static int failures = 0;
#define EXPECT(c)                                                   \
    do {                                                            \
        if (!(c)) {                                                 \
            std::printf("FAILED %s (line %d)\n", #c, __LINE__);     \
            ++failures;                                             \
        }                                                           \
    } while (0)

int main() {
    const int cap = MCV_MAX_TRACK_LEN;
    // tracks: empty, one ray, empty, two rays, the cap (every fourth ray repeats an earlier one), empty, one ray
    const int lens[] = {0, 1, 0, 2, cap, 0, 1};
    const int T = (int)(sizeof(lens) / sizeof(lens[0]));
    std::vector<int> offsets(T + 1, 0);
    for (int t = 0; t < T; ++t) offsets[t + 1] = offsets[t] + lens[t];
    const int n = offsets[T];

    // cameras on a circle of radius 10 looking at the origin, one observation each
    const int nCams = 64;
    std::vector<double> cams(14 * (size_t)nCams);
    for (int c = 0; c < nCams; ++c) {
        const double a = 6.283185307179586 * c / nCams, x = std::cos(a), y = std::sin(a);
        const double v[14] = {10 * x, 10 * y, 0, -x, -y, 0, 0, 0, 1, -y, x, 0, 2, 2};
        for (int k = 0; k < 14; ++k) cams[14 * (size_t)c + k] = v[k];
    }
    std::vector<int> camIdx((size_t)n);
    std::vector<double> obs(2 * (size_t)n), rays(6 * (size_t)n);
    for (int i = 0; i < n; ++i) {
        const int j = i % 4 == 3 ? i - 3 : i;   // a repeat of an earlier observation: an equal ray
        camIdx[i] = (j * 7) % nCams;
        obs[2 * (size_t)i] = 0.01 * ((j * 13) % 17 - 8);
        obs[2 * (size_t)i + 1] = 0.01 * ((j * 5) % 11 - 5);
        ray_unproject(cams.data() + 14 * (size_t)camIdx[i], obs[2 * (size_t)i], obs[2 * (size_t)i + 1],
                      *reinterpret_cast<double(*)[6]>(rays.data() + 6 * (size_t)i));
    }

    int where = -1;
    EXPECT(tri_check_offsets(offsets.data(), T, &where) == 0);
    EXPECT(tri_check_cameras(camIdx.data(), n, nCams) == -1);
    EXPECT(tri_check_cameras(camIdx.data(), n, 1) >= 0);

    std::vector<double> pa(3 * (size_t)T), pb(3 * (size_t)T), cost((size_t)T);
    std::vector<int> ca((size_t)T), cb((size_t)T), vis((size_t)T);
    long long rejected[4] = {0, 0, 0, 0};
    const int ka = tri_host_intersect(rays.data(), offsets.data(), T, pa.data(), ca.data(), rejected);
    const int kb = tri_host_triangulate(cams.data(), camIdx.data(), obs.data(), offsets.data(), T, pb.data(), cb.data(),
                                        cost.data(), vis.data());
    EXPECT(ka == kb);
    for (int t = 0; t < T; ++t) {
        EXPECT(ca[t] == cb[t]);
        if (lens[t] < 2) EXPECT(ca[t] == 0 && std::isnan(pa[3 * (size_t)t]) && std::isinf(cost[t]) && vis[t] == 0);
        for (int k = 0; k < 3; ++k)
            EXPECT((std::isnan(pa[3 * (size_t)t + k]) && std::isnan(pb[3 * (size_t)t + k])) ||
                   pa[3 * (size_t)t + k] == pb[3 * (size_t)t + k]);
    }
    EXPECT(ca[4] > 0 && rejected[0] >= cap / 4 - 2);
    // statistics may be left out one at a time
    EXPECT(tri_host_triangulate(cams.data(), camIdx.data(), obs.data(), offsets.data(), T, pb.data(), cb.data(), nullptr,
                                vis.data()) == kb);
    EXPECT(tri_host_triangulate(cams.data(), camIdx.data(), obs.data(), offsets.data(), T, pb.data(), cb.data(),
                                cost.data(), nullptr) == kb);

    // refused offsets: non-zero start, a decrease, one ray over the cap
    std::vector<int> bad = offsets;
    bad[0] = 1;
    EXPECT(tri_check_offsets(bad.data(), T, &where) == 1);
    bad = offsets;
    bad[4] = bad[3] - 1;
    EXPECT(tri_check_offsets(bad.data(), T, &where) == 2 && where == 3);
    bad = offsets;
    for (int t = 5; t <= T; ++t) bad[t] += 1;
    EXPECT(tri_check_offsets(bad.data(), T, &where) == 3 && where == 4);

    // no tracks at all
    const int zero = 0;
    EXPECT(tri_check_offsets(&zero, 0, &where) == 0);
    EXPECT(tri_host_intersect(nullptr, &zero, 0, nullptr, nullptr) == 0);

    if (failures) return 1;
    std::printf("triangulate_asan ok: %d tracks, %d rays, %d pairs kept on the cap track, %lld duplicates\n", T, n,
                ca[4], rejected[0]);
    return 0;
}
