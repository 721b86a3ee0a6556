// Stand-alone sanitizer program for the host side of bundle adjustment with focal groups (ba_ref.h,
// DESIGN §7p): the groups' construction and checks, the chains over a group's cameras and the twin's
// Levenberg-Marquardt loop with the focal blocks. Built by tests/test_bundle_adjust_focal.py with
// -fsanitize=address,undefined and run as a process of its own over the shared cases, which the test
// writes to a text file (argv[1]); every array is allocated at its exact size so an index past an end is
// caught. Prints each case's result for the test to compare with the library's twin, bit for bit.
//
// Input per case, whitespace-separated: nCameras T n hasFixed hasGroup hasFixedFocal focalMode, the six
// configuration values, then the arrays: 14 nCameras camera doubles, nCameras fixed bytes if hasFixed,
// nCameras group values if hasGroup, nCameras fixedFocal bytes if hasFixedFocal, n camera indices, 2 n
// observation doubles, T + 1 offsets, 3 T point doubles. Doubles are C hex floats.
// Output per case: a line "iterations accepted rejected cgIterations usedObservations usedTracks
// termination freeFocalGroups groups", a line of initialCost finalCost, then the cameras and the points,
// one line each, every double as its 64-bit pattern in hex.
#include "ba_ref.h"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

using namespace mcv;

static std::vector<double> read_doubles(std::istream& in, size_t n) {
    std::vector<double> v(n);
    std::string tok;
    for (size_t k = 0; k < n; ++k) {
        in >> tok;
        v[k] = std::strtod(tok.c_str(), nullptr);
    }
    return v;
}

template <class T>
static std::vector<T> read_ints(std::istream& in, size_t n) {
    std::vector<T> v(n);
    for (size_t k = 0; k < n; ++k) {
        long long x = 0;
        in >> x;
        v[k] = (T)x;
    }
    return v;
}

static void print_bits(const double* v, size_t n) {
    for (size_t k = 0; k < n; ++k) {
        uint64_t u;
        std::memcpy(&u, v + k, sizeof(u));
        std::printf("%016" PRIx64 " ", u);
    }
    std::printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    int cases = 0;
    long long nCameras;
    while (in >> nCameras) {
        long long T = 0, n = 0, hasFixed = 0, hasGroup = 0, hasFixedFocal = 0;
        BaFocalConfig cfg;
        in >> T >> n >> hasFixed >> hasGroup >> hasFixedFocal >> cfg.focalMode;
        cfg.pad = 0;
        in >> cfg.base.maxIterations >> cfg.base.maxCgIterations;
        const std::vector<double> cv = read_doubles(in, 4);
        cfg.base.cgTolerance = cv[0];
        cfg.base.initialLambda = cv[1];
        cfg.base.functionTolerance = cv[2];
        cfg.base.huberDelta = cv[3];
        const std::vector<double> cams = read_doubles(in, 14 * (size_t)nCameras);
        const std::vector<uint8_t> fixed = read_ints<uint8_t>(in, hasFixed ? (size_t)nCameras : 0);
        const std::vector<int> group = read_ints<int>(in, hasGroup ? (size_t)nCameras : 0);
        const std::vector<uint8_t> fixedFocal = read_ints<uint8_t>(in, hasFixedFocal ? (size_t)nCameras : 0);
        const std::vector<int> idx = read_ints<int>(in, (size_t)n);
        const std::vector<double> obs = read_doubles(in, 2 * (size_t)n);
        const std::vector<int> off = read_ints<int>(in, (size_t)T + 1);
        const std::vector<double> pts = read_doubles(in, 3 * (size_t)T);
        if (!in || ba_check_config(cfg.base) || off[(size_t)T] != n) return 3;
        int where = 0;
        BaCsr csr;
        BaGroups grp;
        if (tri_check_offsets(off.data(), (int)T, &where) != 0 ||
            ba_build_csr(idx.data(), off.data(), (int)T, (int)nCameras, csr) >= 0 ||
            ba_check_cameras_finite(cams.data(), (int)nCameras) >= 0 ||
            ba_build_groups(cfg.focalMode, hasGroup ? group.data() : nullptr, hasFixedFocal ? fixedFocal.data() : nullptr,
                            cams.data(), (int)nCameras, grp, &where) != 0) {
            std::printf("FAILED checks\n");
            return 1;
        }
        std::vector<double> outC(14 * (size_t)nCameras), outP(3 * (size_t)T);
        BaFocalSummary sm;
        const int groups = grp.nG;
        ba_host_bundle_adjust_focal(cams.data(), (int)nCameras, hasFixed ? fixed.data() : nullptr, idx.data(),
                                    obs.data(), off.data(), (int)T, pts.data(), cfg, csr, grp, outC.data(), outP.data(),
                                    sm);
        std::printf("%d %d %d %d %d %d %d %d %d\n", sm.base.iterations, sm.base.accepted, sm.base.rejected,
                    sm.base.cgIterations, sm.base.usedObservations, sm.base.usedTracks, sm.base.termination,
                    sm.freeFocalGroups, groups);
        const double costs[2] = {sm.base.initialCost, sm.base.finalCost};
        print_bits(costs, 2);
        print_bits(outC.data(), outC.size());
        print_bits(outP.data(), outP.size());
        cases += 1;
    }
    // the groups' checks stop before anything is indexed with the bad entry
    {
        const double cams[28] = {0, 0, 0, 0, 0, 1, 0, 1, 0, 1, 0, 0, 1.5, 1.5, 1, 0, 0, 0, 0, 1, 0, 1, 0, 1, 0, 0, 1.5, 2.5};
        const int high[2] = {0, 2}, neg[2] = {-1, 0}, same[2] = {1, 1};
        const uint8_t ff[2] = {1, 0};
        double bad[28];
        std::memcpy(bad, cams, sizeof(bad));
        bad[12] = -1.0;
        BaGroups g;
        int where = -1;
        if (ba_build_groups(3, nullptr, nullptr, cams, 2, g, &where) != 1 ||
            ba_build_groups(1, high, nullptr, cams, 2, g, &where) != 2 || where != 1 ||
            ba_build_groups(1, neg, nullptr, cams, 2, g, &where) != 2 || where != 0 ||
            ba_build_groups(1, same, nullptr, cams, 2, g, &where) != 3 || where != 1 ||
            ba_build_groups(1, nullptr, nullptr, bad, 2, g, &where) != 4 || where != 0 ||
            ba_build_groups(1, nullptr, ff, bad, 2, g, &where) != 0 || g.nG != 2 ||
            ba_build_groups(0, nullptr, nullptr, bad, 2, g, &where) != 0) {
            std::printf("FAILED refusals\n");
            return 1;
        }
    }
    std::printf("bundle_adjust_focal_asan ok: %d cases\n", cases);
    return 0;
}
