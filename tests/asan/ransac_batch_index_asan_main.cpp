// Stand-alone sanitizer program for the index code of the batched RANSAC calls (ransac_batch_index.h): the
// check of the offsets, the layout of a call and the plan of a hypothesis round, walked round by round the way
// the driver does it (the active list carried along, the replay's part played by a callback): a budget split
// over rounds, a budget lowered after the first round, a stopped problem, a smaller first round, one problem,
// every problem stopped and an empty active list. Built by tests/test_batch.py with
// -fsanitize=address,undefined and run as a process of its own; every array is allocated at its exact size so
// an index past an end is caught.
#include "ransac_batch_index.h"

#include <cstdio>
#include <functional>
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

struct State { int64_t niters; int stopped; };
typedef std::vector<std::vector<int>> Counts;

// Rounds of the given sizes from begin = 0 on. Returns every round's hypothesis counts.
static Counts walk(const std::vector<int>& sizes, std::vector<State> st, const std::vector<int64_t>& rounds,
                   std::function<void(int, std::vector<State>&)> after, std::vector<int>* left = nullptr) {
    const int D = (int)sizes.size();
    std::vector<BatchProblem> prob((size_t)D);
    int off = 0;
    for (int d = 0; d < D; ++d) {
        prob[(size_t)d] = BatchProblem{off, sizes[(size_t)d], (int64_t)d * 10};
        off += sizes[(size_t)d];
    }
    std::vector<int> active((size_t)D);
    for (int d = 0; d < D; ++d) active[(size_t)d] = d;
    Counts seen;
    int64_t begin = 0;
    for (size_t r = 0; r < rounds.size(); ++r) {
        const std::vector<int> before = active;
        std::vector<BatchDesc> desc(active.size());   // exactly the entries a round may fill
        const BatchRound R = batch_round(prob.data(), st.data(), active, begin, rounds[r],
                                         [&](size_t j, int) -> BatchDesc& { return desc.at(j); });
        EXPECT(R.n == (int)active.size() && R.n <= (int)before.size());
        std::vector<int> cnt;
        int stride = 0;
        size_t k = 0;
        for (int d : before) {   // the definition, problem by problem
            const int64_t rest = st[(size_t)d].niters - begin;
            if (st[(size_t)d].stopped || rest <= 0) continue;
            EXPECT(k < active.size() && active[k] == d);
            if (k >= active.size()) break;
            const BatchDesc& X = desc[k];
            EXPECT(X.ptOff == prob[(size_t)d].ptOff && X.N == prob[(size_t)d].N && X.rowOff == prob[(size_t)d].rowOff);
            EXPECT(X.hypBegin == begin && X.hypCount == (rest < rounds[r] ? rest : rounds[r]) && X.hypCount >= 1);
            stride = X.hypCount > stride ? X.hypCount : stride;
            cnt.push_back(X.hypCount);
            ++k;
        }
        EXPECT(k == active.size() && R.stride == stride);
        for (int j = 0; j < R.n; ++j) {   // the slots of the round are disjoint and inside n * stride
            EXPECT(desc[(size_t)j].slotOff == (int64_t)j * stride);
            EXPECT(desc[(size_t)j].slotOff + desc[(size_t)j].hypCount <= (int64_t)R.n * stride);
        }
        seen.push_back(cnt);
        begin += rounds[r];
        if (after) after((int)r, st);
    }
    if (left) *left = active;
    return seen;
}

int main() {
    const std::vector<int> three = {30, 7, 64};
    const std::vector<State> fresh(3, State{10, 0});
    std::vector<int> left;
    EXPECT((walk(three, fresh, {4, 4, 4, 4}, nullptr, &left) == Counts{{4, 4, 4}, {4, 4, 4}, {2, 2, 2}, {}}));
    EXPECT(left.empty());
    auto lower = [](int r, std::vector<State>& st) {
        if (r == 0) st[1].niters = 5;
    };
    EXPECT((walk(three, fresh, {4, 4, 4}, lower, &left) == Counts{{4, 4, 4}, {4, 1, 4}, {2, 2}}));
    EXPECT((left == std::vector<int>{0, 2}));
    std::vector<State> one_stopped = fresh;
    one_stopped[1].stopped = 1;
    EXPECT((walk(three, one_stopped, {4, 4}, nullptr, &left) == Counts{{4, 4}, {4, 4}}));
    EXPECT((left == std::vector<int>{0, 2}));
    EXPECT((walk(three, fresh, {2, 4, 4, 4}, nullptr) == Counts{{2, 2, 2}, {4, 4, 4}, {4, 4, 4}, {}}));
    EXPECT((walk({9}, {State{10, 0}}, {4, 4, 4, 4}, nullptr) == Counts{{4}, {4}, {2}, {}}));
    EXPECT((walk(three, std::vector<State>(3, State{10, 1}), {4, 4}, nullptr) == Counts{{}, {}}));
    EXPECT((walk({}, {}, {4}, nullptr) == Counts{{}}));
    // a budget past 2^31 keeps the count at the round's size
    EXPECT((walk({9}, {State{(int64_t)1 << 40, 0}}, {1 << 30}, nullptr) == Counts{{1 << 30}}));
    // the layout: the device problems, per and the rounds, as mcvHostBatchLayout reports them
    const int offs[] = {0, 50, 53, 113, 183};
    BatchLayout L;
    batch_layout(offs, 4, 4, 1000, 2999, L);
    EXPECT((L.dev == std::vector<int>{0, 2, 3}) && L.per == 999 && L.rounds == 2 && L.iters == 1000);
    EXPECT(L.slotOff.size() == 4 && L.slotOff[1] == -1 && L.slotOff[3] == 2 * 999 && L.rowOff[2] == 1000);
    batch_layout(offs, 0, 4, 0, 0, L);
    EXPECT(L.dev.empty() && L.rounds == 0 && L.iters == 1 && L.slotOff.empty());
    // the refusals of the offsets
    int where = -1;
    const int bad0[] = {1, 2, 3};
    EXPECT(batch_check_offsets(bad0, 2, &where) == 1);
    const int bad1[] = {0, 5, 4, 9};
    EXPECT(batch_check_offsets(bad1, 3, &where) == 2 && where == 1);
    const int none[] = {0};
    EXPECT(batch_check_offsets(none, 0, &where) == 0 && batch_check_offsets(offs, 4, &where) == 0);
    if (failures) {
        std::printf("ransac_batch_index_asan: %d failures\n", failures);
        return 1;
    }
    std::printf("ransac_batch_index_asan ok\n");
    return 0;
}
