// Stand-alone sanitizer program for the host side of bundle adjustment (ba_ref.h): the camera-side CSR
// and its segments, the summation orders and the twin's Levenberg-Marquardt loop. Built by
// tests/test_bundle_adjust.py with -fsanitize=address,undefined and run as a process of its own over
// the shared cases, which the test writes to a text file (argv[1]); every array is allocated at its
// exact size so an index past an end is caught. Prints each case's result for the test to compare with
// the library's twin, bit for bit.
//
// Input per case, whitespace-separated: nCameras T n hasFixed, the six configuration values, then the
// arrays: 14 nCameras camera doubles, nCameras fixed bytes if hasFixed, n camera indices, 2 n observation
// doubles, T + 1 offsets, 3 T point doubles. Doubles are C hex floats ("nan" and "inf" as such).
// Output per case: a line "iterations accepted rejected cgIterations usedObservations usedTracks
// termination segments", a line of initialCost finalCost, then the cameras and the points, one line
// each, every double as its 64-bit pattern in hex.
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
        long long T = 0, n = 0, hasFixed = 0;
        in >> T >> n >> hasFixed;
        BaConfig cfg;
        in >> cfg.maxIterations >> cfg.maxCgIterations;
        const std::vector<double> cv = read_doubles(in, 4);
        cfg.cgTolerance = cv[0];
        cfg.initialLambda = cv[1];
        cfg.functionTolerance = cv[2];
        cfg.huberDelta = cv[3];
        const std::vector<double> cams = read_doubles(in, 14 * (size_t)nCameras);
        const std::vector<uint8_t> fixed = read_ints<uint8_t>(in, hasFixed ? (size_t)nCameras : 0);
        const std::vector<int> idx = read_ints<int>(in, (size_t)n);
        const std::vector<double> obs = read_doubles(in, 2 * (size_t)n);
        const std::vector<int> off = read_ints<int>(in, (size_t)T + 1);
        const std::vector<double> pts = read_doubles(in, 3 * (size_t)T);
        if (!in || ba_check_config(cfg) || off[(size_t)T] != n) return 3;
        int where = 0;
        BaCsr csr;
        if (tri_check_offsets(off.data(), (int)T, &where) != 0 ||
            ba_build_csr(idx.data(), off.data(), (int)T, (int)nCameras, csr) >= 0 ||
            ba_check_cameras_finite(cams.data(), (int)nCameras) >= 0) {
            std::printf("FAILED checks\n");
            return 1;
        }
        std::vector<double> outC(14 * (size_t)nCameras), outP(3 * (size_t)T);
        BaSummary sm;
        const size_t segments = csr.segCam.size();
        ba_host_bundle_adjust(cams.data(), (int)nCameras, hasFixed ? fixed.data() : nullptr, idx.data(), obs.data(),
                              off.data(), (int)T, pts.data(), cfg, csr, outC.data(), outP.data(), sm);
        std::printf("%d %d %d %d %d %d %d %zu\n", sm.iterations, sm.accepted, sm.rejected, sm.cgIterations,
                    sm.usedObservations, sm.usedTracks, sm.termination, segments);
        const double costs[2] = {sm.initialCost, sm.finalCost};
        print_bits(costs, 2);
        print_bits(outC.data(), outC.size());
        print_bits(outP.data(), outP.size());
        cases += 1;
    }
    // the index check of the CSR pass stops before anything is indexed with the bad entry
    {
        const int off[2] = {0, 2}, bad[2] = {0, 3}, neg[2] = {-1, 0};
        BaCsr csr;
        if (ba_build_csr(bad, off, 1, 3, csr) != 1 || ba_build_csr(neg, off, 1, 3, csr) != 0) {
            std::printf("FAILED refusals\n");
            return 1;
        }
    }
    std::printf("bundle_adjust_asan ok: %d cases\n", cases);
    return 0;
}
