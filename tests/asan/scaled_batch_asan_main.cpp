// Stand-alone sanitizer program for the index code of the batched findScaled (scaled_batch_index.h):
// the CSR and setIdx checks, every problem's slice of the row, candidate and block spaces, and the
// sweep's work list, on empty sets first, in the middle and last, shared sets, one-row sets and sizes
// at the block edges. Built by tests/test_batch_scaled.py with -fsanitize=address,undefined and run as
// a process of its own; every array is allocated at its exact size so an index past an end is caught.
#include "scaled_batch_index.h"

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

// Lays the batch out, builds the work list and walks it the way the sweep does: every block names a
// non-empty problem, its candidates lie inside the problem's slice, its clamped tile rows inside the
// problem's set, and together the blocks cover every candidate exactly once.
static void walk(const std::vector<int>& sizes, const std::vector<int>& setIdx, bool nullIdx) {
    const int S = (int)sizes.size(), P = nullIdx ? S : (int)setIdx.size();
    std::vector<int> offsets((size_t)S + 1, 0);
    for (int s = 0; s < S; ++s) offsets[s + 1] = offsets[s] + sizes[s];
    const int* idx = nullIdx ? nullptr : setIdx.data();
    int where = -1;
    EXPECT(scaled_batch_check_offsets(offsets.data(), S, &where) == 0);
    EXPECT(scaled_batch_check_sets(idx, P, S) == -1);
    std::vector<ScaledBatchProb> probs((size_t)P);
    long long cands = -1, blocks = -1;
    int live = -1;
    EXPECT(scaled_batch_layout(offsets.data(), idx, P, probs.data(), &cands, &blocks, &live));
    std::vector<int> list((size_t)blocks, -1);
    scaled_batch_work_list(probs.data(), P, list.data());
    std::vector<char> rows((size_t)offsets[S], 0), hit((size_t)cands, 0);
    long long expectCands = 0;
    int expectLive = 0;
    for (int p = 0; p < P; ++p) {
        const int n = sizes[nullIdx ? p : setIdx[p]];
        EXPECT(probs[p].N == n && probs[p].candOff == expectCands);
        EXPECT(probs[p].rowOff == offsets[nullIdx ? p : setIdx[p]]);
        expectCands += 2ll * n;
        expectLive += n > 0;
    }
    EXPECT(cands == expectCands && live == expectLive);
    for (long long b = 0; b < blocks; ++b) {
        const int p = list[(size_t)b];
        EXPECT(p >= 0 && p < P);
        if (p < 0 || p >= P) continue;
        const ScaledBatchProb& pd = probs[p];
        EXPECT(pd.N > 0 && b >= pd.blockOff && b < pd.blockOff + scaled_batch_blocks(pd.N));
        const int nCand = 2 * pd.N;
        for (int lane = 0; lane < kScaledBatchCands; ++lane) {
            const int c = (int)(b - pd.blockOff) * kScaledBatchCands + lane;
            const int cc = c < nCand ? c : nCand - 1;       // the sweep's clamp of idle lanes
            EXPECT(cc >= 0 && cc < nCand);
            (void)hit[(size_t)pd.candOff + cc];             // the read of the clamped lane: inside the array
            if (c < nCand) hit[(size_t)pd.candOff + c] += 1;
        }
        for (int t = 0; t * 32 < pd.N; ++t)                 // observation tiles of 32, the tail clamped
            for (int l = 0; l < 32; ++l) {
                const int j0 = t * 32 + l, j = j0 < pd.N ? j0 : pd.N - 1;
                rows[(size_t)pd.rowOff + j] = 1;
            }
    }
    for (long long c = 0; c < cands; ++c) EXPECT(hit[(size_t)c] == 1);
    for (int p = 0; p < P; ++p)                             // every row of a problem's set was staged
        for (int j = 0; j < probs[p].N; ++j) EXPECT(rows[(size_t)probs[p].rowOff + j] == 1);
}

int main() {
    // empty sets first, in the middle and last; one-row sets; 31..33 and 63..65 observations around
    // the 64-candidate block (32 observations) and its double; a larger odd size
    const std::vector<int> sizes = {0, 1, 31, 32, 33, 0, 63, 64, 65, 1, 1001, 0};
    std::vector<int> own;
    for (int s = 0; s < (int)sizes.size(); ++s) own.push_back(s);
    walk(sizes, own, true);                                    // setIdx = null, S == P
    walk(sizes, own, false);
    walk(sizes, {0, 10, 3, 3, 3, 3, 5, 1, 9, 9, 2, 8, 11}, false);   // shared sets, set 4, 6, 7 unused
    walk(sizes, {11, 0, 5}, false);                            // nothing but empty problems: no block
    walk({}, {}, true);                                        // no sets, no problems
    walk({1}, {0}, false);
    walk({0}, {0}, false);

    // refused inputs
    int where = -1;
    std::vector<int> off = {0, 2, 5, 5, 9};
    EXPECT(scaled_batch_check_offsets(off.data(), 4, &where) == 0);
    off[0] = 1;
    EXPECT(scaled_batch_check_offsets(off.data(), 4, &where) == 1);
    off = {0, 2, 5, 4, 9};
    EXPECT(scaled_batch_check_offsets(off.data(), 4, &where) == 2 && where == 2);
    const std::vector<int> badIdx = {0, 3, 4, -1};
    EXPECT(scaled_batch_check_sets(badIdx.data(), 2, 4) == -1);
    EXPECT(scaled_batch_check_sets(badIdx.data(), 3, 4) == 2);
    const std::vector<int> negIdx = {0, -1};
    EXPECT(scaled_batch_check_sets(negIdx.data(), 2, 4) == 1);

    // the candidate cap: 2^27 rows used once fit exactly, used twice do not, and nothing overflows
    const std::vector<int> big = {0, 1 << 27};
    const std::vector<int> twice = {0, 0, 0};
    std::vector<ScaledBatchProb> probs(3);
    long long cands = 0, blocks = 0;
    int live = 0;
    EXPECT(scaled_batch_layout(big.data(), twice.data(), 1, probs.data(), &cands, &blocks, &live));
    EXPECT(cands == kScaledBatchMax && blocks == (1 << 22) && live == 1);
    EXPECT(!scaled_batch_layout(big.data(), twice.data(), 3, probs.data(), &cands, &blocks, &live));

    if (failures) return 1;
    std::printf("scaled_batch_asan ok\n");
    return 0;
}
