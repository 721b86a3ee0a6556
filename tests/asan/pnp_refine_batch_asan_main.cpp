// Stand-alone sanitizer program for the index code of the batched PnP refinement
// (pnp_refine_batch_index.h): the offsets checks, every problem's selected count and place in the compact
// array, the refusal reasons and the job table, on empty problems first, in the middle and last, masks that
// select nothing, everything, only the first or the last row, bytes other than 1, and a null mask. The
// gather is walked the way the kernel does it (a search of compOff per compact row, then the problem's index
// list). Built by tests/test_batch_pnp_refine.py with -fsanitize=address,undefined and run as a process of
// its own; every array is allocated at its exact size so an index past an end is caught.
#include "pnp_refine_batch_index.h"

#include <cstdio>
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

// mode: 0 all zero, 1 all one, 2 only the first row, 3 only the last row, 4 every third row with bytes 2 / 255,
// 5 null mask
static void walk(const std::vector<int>& sizes, int mode, const std::vector<char>& camOk) {
    const int B = (int)sizes.size();
    std::vector<int> offsets((size_t)B + 1, 0);
    for (int p = 0; p < B; ++p) offsets[p + 1] = offsets[p] + sizes[p];
    int where = -1;
    EXPECT(refine_batch_check_offsets(offsets.data(), B, &where) == 0);
    EXPECT(refine_batch_check_sizes(offsets.data(), B, 1 << 20) == -1);
    const int total = offsets[B];
    std::vector<uint8_t> mask((size_t)total, 0);
    for (int p = 0; p < B; ++p)
        for (int i = 0; i < sizes[p]; ++i) {
            uint8_t v = 0;
            if (mode == 1) v = 1;
            if (mode == 2 && i == 0) v = 1;
            if (mode == 3 && i == sizes[p] - 1) v = 255;
            if (mode == 4 && i % 3 == 0) v = (i % 2) ? 2 : 255;
            mask[(size_t)offsets[p] + i] = v;
        }
    const uint8_t* m = mode == 5 ? nullptr : mask.data();
    std::vector<int> counts((size_t)B, -1), compOff((size_t)B + 1, -1), reason((size_t)B, -1);
    const int largest = refine_batch_layout(offsets.data(), B, m, counts.data(), compOff.data());
    int sum = 0, big = 0, runs = 0;
    for (int p = 0; p < B; ++p) {
        int c = 0;
        for (int i = 0; i < sizes[p]; ++i) c += !m || m[(size_t)offsets[p] + i] ? 1 : 0;
        EXPECT(counts[p] == c && compOff[p] == sum);
        sum += c;
        if (c > big) big = c;
        reason[p] = refine_batch_reason(counts[p], camOk[(size_t)p] != 0);
        EXPECT(reason[p] == (c < kRefineMinRows ? kRefineTooFew : (camOk[(size_t)p] ? kRefineRuns : kRefineBadCamera)));
        runs += reason[p] == kRefineRuns;
    }
    EXPECT(compOff[B] == sum && largest == big && sum <= total);
    // the compact index lists (mcv_mask_compact per problem) and the gather's walk
    std::vector<int> idx((size_t)total, -1);
    for (int p = 0; p < B; ++p) {
        int k = 0;
        for (int i = 0; i < sizes[p]; ++i)
            if (!m || m[(size_t)offsets[p] + i]) idx[(size_t)offsets[p] + k++] = i;
    }
    std::vector<int> src((size_t)sum, -1);
    for (int g = 0; g < sum; ++g) {
        int lo = 0, hi = B;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (compOff[(size_t)mid] <= g) lo = mid;
            else hi = mid;
        }
        EXPECT(compOff[(size_t)lo] <= g && g < compOff[(size_t)lo] + counts[(size_t)lo]);
        const int i = idx[(size_t)offsets[lo] + (g - compOff[(size_t)lo])];
        EXPECT(i >= 0 && i < sizes[lo]);
        src[(size_t)g] = offsets[lo] + i;
    }
    for (int g = 1; g < sum; ++g) EXPECT(src[(size_t)g] > src[(size_t)g - 1]);   // index order, problems in order
    for (int g = 0; g < sum; ++g) EXPECT(!m || m[(size_t)src[(size_t)g]] != 0);
    // the job table, over the compact array and over the rows
    for (int gathered = 0; gathered < 2; ++gathered) {
        int jl = -1;
        std::vector<RefineBatchJob> all((size_t)B);
        const int n = refine_batch_jobs(offsets.data(), B, counts.data(), compOff.data(), reason.data(), gathered != 0,
                                        all.data(), &jl);
        EXPECT(n == runs);
        int prev = -1, jbig = 0;
        for (int j = 0; j < n; ++j) {
            const RefineBatchJob& J = all[(size_t)j];
            EXPECT(J.prob > prev && J.prob < B && reason[(size_t)J.prob] == kRefineRuns);
            EXPECT(J.N == counts[(size_t)J.prob] && J.N >= kRefineMinRows);
            EXPECT(J.ptOff == (gathered ? compOff[(size_t)J.prob] : offsets[J.prob]));
            EXPECT(J.ptOff >= 0 && J.ptOff + J.N <= (gathered ? sum : total));
            prev = J.prob;
            if (J.N > jbig) jbig = J.N;
        }
        EXPECT(jl == jbig);
    }
}

int main() {
    const std::vector<std::vector<int>> cases = {
        {0, 1, 2, 3, 31, 32, 33, 255, 256, 257},
        {257, 0, 3, 0, 0, 2, 1024, 1, 0},
        {0},
        {5},
        {},
        {0, 0, 0},
        {3, 3, 3, 2, 2, 4},
    };
    for (const auto& sizes : cases)
        for (int mode = 0; mode < 6; ++mode) {
            std::vector<char> ok(sizes.size(), 1), mixed(sizes.size(), 1);
            for (size_t p = 0; p < mixed.size(); p += 2) mixed[p] = 0;
            walk(sizes, mode, ok);
            walk(sizes, mode, mixed);
        }
    // the refusals of the offsets
    int where = -1;
    const int bad0[] = {1, 2, 3};
    EXPECT(refine_batch_check_offsets(bad0, 2, &where) == 1);
    const int bad1[] = {0, 5, 4, 9};
    EXPECT(refine_batch_check_offsets(bad1, 3, &where) == 2 && where == 1);
    const int big[] = {0, 5, 105, 106};
    EXPECT(refine_batch_check_sizes(big, 3, 99) == 1 && refine_batch_check_sizes(big, 3, 100) == -1);
    const int none[] = {0};
    EXPECT(refine_batch_check_offsets(none, 0, &where) == 0);
    if (failures) {
        std::printf("pnp_refine_batch_asan: %d failures\n", failures);
        return 1;
    }
    std::printf("pnp_refine_batch_asan ok\n");
    return 0;
}
