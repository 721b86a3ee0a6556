// Stand-alone sanitizer program for the host side of track building (tracks_ref.h): the argument
// checks, the match CSR -> edge list conversion and the union-find twin. Built by tests/test_tracks.py
// with -fsanitize=address,undefined and run as a process of its own over the shared cases, which the
// test writes to a text file (argv[1]); every array is allocated at its exact size so an index past
// an end is caught. Prints each case's result for the test to compare with the reference.
//
// Input, whitespace-separated integers, per case: nImages, the counts, B, the 2 B image indices, the
// B + 1 offsets, the 2 offsets[B] pair entries, hasMask, the offsets[B] mask bytes if so, minLength.
// Output per case: a line "T nObs oversize conflicts short", then trackOffsets, cameraIdx, featureIdx
// and trackOfFeature, one line each.
#include "tracks_ref.h"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <vector>

using namespace mcv;

static void print(const std::vector<int>& v) {
    for (int x : v) std::printf("%d ", x);
    std::printf("\n");
}

template <class T>
static std::vector<T> read(std::istream& in, size_t n) {
    std::vector<T> v(n);
    for (size_t k = 0; k < n; ++k) {
        long long x = 0;
        in >> x;
        v[k] = (T)x;
    }
    return v;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    int cases = 0;
    long long nImages;
    while (in >> nImages) {
        const std::vector<int> counts = read<int>(in, (size_t)nImages);
        long long B = 0, hasMask = 0, minLength = 0;
        in >> B;
        const std::vector<int> imagePairs = read<int>(in, 2 * (size_t)B);
        const std::vector<int> offsets = read<int>(in, (size_t)B + 1);
        const std::vector<int> pairs = read<int>(in, 2 * (size_t)offsets[(size_t)B]);
        in >> hasMask;
        const std::vector<uint8_t> mask = read<uint8_t>(in, hasMask ? (size_t)offsets[(size_t)B] : 0);
        in >> minLength;
        if (!in) return 3;
        // non-null stand-ins for empty arrays: the checks look at the pointers, never through them
        static const int none[1] = {0};
        std::vector<int> base, edges;
        std::string err;
        long long nEdges = -1;
        const bool ok = trk_prepare("tracks_asan", counts.empty() ? none : counts.data(), (int)nImages,
                                    imagePairs.empty() ? none : imagePairs.data(), (int)B,
                                    pairs.empty() ? none : pairs.data(), offsets.data(),
                                    hasMask ? (mask.empty() ? (const uint8_t*)none : mask.data()) : nullptr,
                                    (int)minLength, none, 0, none, none, 0, base, &edges, &nEdges, err);
        if (!ok) {
            std::printf("FAILED %s\n", err.c_str());
            return 1;
        }
        const std::vector<int> exact(edges.begin(), edges.begin() + 2 * nEdges);   // the kept edges, no slack
        TrkResult R;
        trk_host_build(base.data(), (int)nImages, exact.data(), nEdges, (int)minLength, R);
        std::printf("%zu %zu %lld %lld %lld\n", R.trackOffsets.size() - 1, R.cameraIdx.size(), R.dropped[0],
                    R.dropped[1], R.dropped[2]);
        print(R.trackOffsets);
        print(R.cameraIdx);
        print(R.featureIdx);
        print(R.trackOfFeature);
        cases += 1;
    }
    // refusals: each stops at its check, before anything is indexed
    {
        std::vector<int> base;
        std::string err;
        long long n = 0;
        const int counts[2] = {2, 2}, ip[2] = {0, 1}, off[2] = {0, 1}, good[2] = {1, 1}, bad[2] = {1, 2}, out[1] = {0};
        const int neg[2] = {2, -1}, offBad[2] = {1, 1}, ipBad[2] = {0, 2};
        int refused = 0;
        refused += !trk_prepare("t", counts, 2, ip, 1, bad, off, nullptr, 2, out, 0, out, out, 0, base, nullptr, &n, err);
        refused += !trk_prepare("t", neg, 2, ip, 1, good, off, nullptr, 2, out, 0, out, out, 0, base, nullptr, &n, err);
        refused += !trk_prepare("t", counts, 2, ip, 1, good, offBad, nullptr, 2, out, 0, out, out, 0, base, nullptr, &n, err);
        refused += !trk_prepare("t", counts, 2, ipBad, 1, good, off, nullptr, 2, out, 0, out, out, 0, base, nullptr, &n, err);
        refused += !trk_prepare("t", counts, 2, ip, 1, good, off, nullptr, 1, out, 0, out, out, 0, base, nullptr, &n, err);
        refused += !trk_prepare("t", nullptr, 2, ip, 1, good, off, nullptr, 2, out, 0, out, out, 0, base, nullptr, &n, err);
        if (refused != 6 || !trk_prepare("t", counts, 2, ip, 1, good, off, nullptr, 2, out, 0, out, out, 0, base, nullptr, &n, err) ||
            n != 1) {
            std::printf("FAILED refusals: %d of 6\n", refused);
            return 1;
        }
    }
    std::printf("tracks_asan ok: %d cases\n", cases);
    return 0;
}
