"""The survivor lists of the staged homography sweep are pushed with one atomic per block (h_list_push_block): the
compaction in blocks of 16 waves, the two bound passes in blocks of 4. The lists are documented as "any order", so
what must hold is their content. test_lists_equal_the_host_twins_sets reads the four lists back (mcvTestHListPush:
the box pass's two lists, the second pass's appends, a compaction through a list and one over every slot) and
compares each, sorted, with the set the host twins keep: a wrong write position (block base, wave offset or ballot
rank) leaves a duplicate, a hole or a wrong slot there. The other tests check what does not see a position: the
lists' lengths, UB, bitmaps and `left` of the hooks' device passes against their host twins, the staged call's key
against the unstaged path's and the oracle's, and the same staging figures from call to call. Staging and the bound
are forced on by the hooks, so small shapes take the path."""
import functools

import numpy as np
import pytest

import _h_cell as HC
import _h_cell_rel as HR
import _oracle
from minicv_amd import native as N
from _h_stage import OFF, ON, PRUNED, THR, THR2, evaluate, models_of, oracle_key, pack, problem

pytestmark = pytest.mark.gpu

# (N, seed, outlier share, first hypothesis, hypotheses): 4099 = 4 x 1024 + 3 slots, so the compaction without a
# source list ends on a block of three; the live lists' lengths fall wherever the data puts them
SHAPES = [(3001, 42, 0.4, 12345, 4099), (20000, 10, 0.5, 0, 4096), (129, 3, 0.5, 0, 4096), (5000, 7, 0.5, 0, 1025)]


@functools.lru_cache(maxsize=None)
def reference(i):
    """The point set on the device and the keys a staged evaluate must return, once per shape: the oracle's, and the
    unstaged path's (the same call with a counts tensor, whose counts are the oracle's)."""
    n, seed, share, begin, count = SHAPES[i]
    src, dst = problem(n, seed, share)
    pts = pack(src, dst)
    key_o, ref = oracle_key(src, dst, seed, begin, count, THR)
    key_u, st, _, full = evaluate(pts, n, seed, begin, count, THR, 1, ON, counts=True)
    assert st[0] == 5                                       # a counts tensor: the call does not stage
    np.testing.assert_array_equal(full, ref)
    assert key_u == key_o
    return pts, key_u


def staged(i, cell, second=0):
    n, seed, _, begin, count = SHAPES[i]
    pts, _ = reference(i)
    prev = N.lib().mcvTestHCellSecondPass(second)
    try:
        key, st, cs, _ = evaluate(pts, n, seed, begin, count, THR, 1, cell)
    finally:
        N.lib().mcvTestHCellSecondPass(prev)
    return key, st, cs


@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_key_over_the_staged_forms(gpu, shape):
    """Both bound passes and three compactions; the box pass alone (one list, two compactions); no bound (the first
    compaction has no source list): the key of each is the unstaged path's and the oracle's."""
    _, key_u = reference(shape)
    key_2, st_2, cs_2 = staged(shape, ON)
    key_1, st_1, cs_1 = staged(shape, ON, second=2)
    key_0, st_0, cs_0 = staged(shape, OFF)
    print(f"{SHAPES[shape]}: both passes: reason {st_2[0]}, B {st_2[1]}, alive {st_2[10:15]}; box pass alone "
          f"{st_1[10:14]}; no bound {st_0[10:14]}")
    assert (cs_2[0], cs_1[0], cs_0[0]) == (1, 1, 0) and (st_2[2], st_1[2], st_0[2]) == (5, 4, 4)
    assert key_2 == key_u and key_1 == key_u and key_0 == key_u
    # the second pass only drops more than the box pass alone, at the boundaries they share
    assert all(a <= b for a, b in zip(st_2[11:12] + st_2[13:15], st_1[11:14]))
    if shape in (0, 1):
        assert st_2[0] == PRUNED and 1 <= st_2[14] < st_2[11]       # not vacuous: the lists shrink, the winner stays
    if st_0[0] == PRUNED:
        assert 1 <= st_0[13] <= st_0[12] <= st_0[11] == SHAPES[shape][4]


@pytest.mark.parametrize("shape", [0, 1])
def test_same_figures_from_call_to_call(gpu, shape):
    """The order of a list may change from run to run, its content may not: the same call three times gives the same
    key and the same B, boundaries and alive counts."""
    runs = [staged(shape, ON)[:2] for _ in range(3)]
    assert runs[0] == runs[1] == runs[2]
    assert runs[0][0] == reference(shape)[1]


@functools.lru_cache(maxsize=None)
def push_problem():
    n, seed = 2000, 7
    src, dst = problem(n, seed)
    pts4 = _oracle.pack4(src, dst)
    models = models_of(n, seed, 1100)
    assert len(models) >= 1025
    cnt, _ = HC.masks(_oracle, pts4, models[:64], THR2)
    cand = int(np.argmax(cnt))
    return pts4, models, models[cand].copy(), int(cnt[cand])


@pytest.mark.parametrize("k", [1, 255, 256, 257, 1025])
def test_block_level_pushes(gpu, k):
    """One atomic per block of 4 waves: a partial last wave, a partial last block and more than one block. The
    device passes' alive (the list's length), UB, bitmaps and `left` equal the host twins'."""
    pts4, models, cand, B = push_problem()
    L = N.lib()
    dev, host = (HC.run(L, pts4, cand, models[:k], THR2, B, device=d) for d in (1, 0))
    for f in ("alive", "ub", "bits", "cell", "sizes"):
        np.testing.assert_array_equal(dev[f], host[f], err_msg=f)
    assert host["alive"] == int((host["ub"] >= B).sum())
    bounds = HR.boundaries(len(pts4))
    dev, host = (HR.run(L, pts4, cand, models[:k], THR2, B, bounds, device=d) for d in (1, 0))
    for f in ("alive", "ub", "bits", "left"):
        np.testing.assert_array_equal(dev[f], host[f], err_msg=f)
    assert host["alive"] == int((host["ub"] >= B).sum())
    if k >= 255:
        assert 0 < host["alive"] < k                          # not vacuous: some slots are kept, some dropped


REL_BASE = 4 ** 4    # first cell of the candidate's inliers (the 4-D grid comes first)


def host_sets(pts4, cand, models, B, bound, counts):
    """The four lists as sets (boolean masks over the slots), from the host twins of the two bound passes and the
    compaction's test: [0] the slots the relative test can still drop, [1] stage 1's list, [2] its compaction with
    the per-slot `left`, [3] the compaction of every slot with the points not yet processed."""
    L, n = N.lib(), len(pts4)
    box = HC.run(L, pts4, cand, models, THR2, B, device=0)
    rel = HR.run(L, pts4, cand, models, THR2, B, [bound], device=0)
    have = counts >= 0
    open_rel = (box["sizes"][None, REL_BASE:] * ~box["cert"][:, REL_BASE:]).sum(1)
    keep = have & (box["ub"] >= B)
    second = keep & (box["ub"] - open_rel < B)
    stage1 = (keep & ~second) | (second & (rel["ub"] >= B))
    rest = n - min(2 * bound, n)
    left = np.where(second, rel["left"][0], rest)
    return [second, stage1, stage1 & (counts + left >= B), have & (counts + rest >= B)]


def device_lists(pts4, cand, models, B, bound, counts):
    k = len(models)
    lists, lens = np.full((4, k), -7, np.int32), np.full(4, -7, np.int32)
    ok = N.lib().mcvTestHListPush(pts4.ctypes.data, len(pts4), cand.ctypes.data, models.ctypes.data, k,
                                  np.float32(THR2), int(B), 4, 12, int(bound), counts.ctypes.data, lists.ctypes.data,
                                  lens.ctypes.data)
    assert ok == 1, N.last_error()
    return lists, lens


# (slots, B: 0 = the candidate's count, the compactions' boundary as a share of the pairs). 1 .. 1025: a partial
# wave, a partial block of 4 waves, more than one block. With the candidate's B every kept slot goes through the
# second pass's list; with B = 400 the box pass fills both of its lists in one call (about half each), and with
# B = 1 everything goes straight to stage 1's list. 4500 slots (the models repeated): the compaction through a list
# of about 4000 runs four live blocks of 1024, the last one partial, and the one over every slot five; with the
# larger B the lists are shorter than the grid and whole blocks return early.
CASES = [(1, 0, 0.5), (255, 0, 0.5), (256, 0, 0.5), (257, 0, 0.5), (1025, 0, 0.5), (1025, 400, 0.5), (4500, 400, 0.5),
         (4500, 1, 1.0), (4500, 0, 0.5)]


@pytest.mark.parametrize("k,b,share", CASES)
def test_lists_equal_the_host_twins_sets(gpu, k, b, share):
    pts4, models, cand, B = push_problem()
    B = b if b else B
    models = np.ascontiguousarray(np.tile(models, (-(-k // len(models)), 1))[:k])
    bound = int((len(pts4) + 1) // 2 * share)
    rng = np.random.default_rng(k + b)
    counts = rng.integers(0, B + 1, k).astype(np.int32)
    counts[rng.random(k) < 0.1] = rng.integers(-3, 0, k)[0]                  # statuses: never listed
    if k == 1:
        counts[:] = B
    want = host_sets(pts4, cand, models, B, bound, counts)
    lists, lens = device_lists(pts4, cand, models, B, bound, counts)
    print(f"{k} slots, B {B}: lengths {lens.tolist()}, host {[int(w.sum()) for w in want]}")
    for j, name in enumerate(("second pass's list", "stage 1's list", "compaction of the list", "compaction of all")):
        got = lists[j, :max(int(lens[j]), 0)]
        np.testing.assert_array_equal(np.sort(got), np.nonzero(want[j])[0], err_msg=name)   # so: no duplicate, no hole
        assert (lists[j, len(got):] == -1).all(), name                       # nothing written past the length
    if k >= 255:
        assert 0 < want[2].sum() < want[1].sum() < k and 0 < want[3].sum() < k      # not vacuous
    if k >= 255 and b != 1:
        assert 0 < (want[1] & want[0]).sum() < want[0].sum()                 # the second pass keeps some, drops some
    if b == 400:
        assert (want[1] & ~want[0]).sum() > 100 and want[0].sum() > 100      # both of the box pass's lists fill
