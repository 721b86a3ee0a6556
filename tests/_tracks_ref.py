"""Track building: an independent pure-Python reference (a dict-based union-find, sets and sorts; no
union-by-smaller-id, no counting sort, nothing of tracks_ref.h's structure), the case list shared by
tests/test_tracks.py and tests/test_gpu_tracks.py, and the ctypes call with sentinel-filled outputs.
Every case's reference answer is computed once and never modified."""
import functools
from collections import defaultdict

import numpy as np

from minicv_amd import native as N

MAX_LEN = 4096
SENTINEL = -77
RANDOM_SEED = 11   # the random scene: see random_scene()


class Case:
    """One call's inputs, from a list of problems (i, j, [(a, b), ...], mask bytes or None), or from the
    call's own arrays (from_arrays: the large scenes, which never exist as Python tuples)."""

    def __init__(self, counts, problems, minLength=2, use_mask=None):
        self.counts = np.ascontiguousarray(counts, np.int32)
        self._problems = [(int(i), int(j), [tuple(map(int, m)) for m in ms],
                           None if mk is None else [int(b) for b in mk]) for i, j, ms, mk in problems]
        self.minLength = minLength
        self.use_mask = any(p[3] is not None for p in self._problems) if use_mask is None else use_mask
        self.imagePairs = np.array([[p[0], p[1]] for p in self._problems], np.int32).reshape(-1, 2)
        self.pairs = np.array([m for p in self._problems for m in p[2]], np.int32).reshape(-1, 2)
        self.offsets = np.concatenate([[0], np.cumsum([len(p[2]) for p in self._problems])]).astype(np.int32)
        self.mask = (np.array([b for p in self._problems for b in (p[3] if p[3] is not None else [1] * len(p[2]))],
                              np.uint8) if self.use_mask else None)
        self.nodes = int(self.counts.sum())

    @classmethod
    def from_arrays(cls, counts, imagePairs, pairs, offsets, mask=None, minLength=2):
        c = cls.__new__(cls)
        c.counts = np.ascontiguousarray(counts, np.int32)
        c._problems = None
        c.minLength, c.use_mask = minLength, mask is not None
        c.imagePairs = np.ascontiguousarray(imagePairs, np.int32).reshape(-1, 2)
        c.pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        c.offsets = np.ascontiguousarray(offsets, np.int32)
        c.mask = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        c.nodes = int(c.counts.sum())
        assert len(c.offsets) == len(c.imagePairs) + 1 and c.offsets[0] == 0 and c.offsets[-1] == len(c.pairs)
        assert c.mask is None or len(c.mask) == len(c.pairs)
        return c

    @property
    def problems(self):
        if self._problems is None:
            o, pr = self.offsets.tolist(), self.pairs.tolist()
            mk = None if self.mask is None else self.mask.tolist()
            self._problems = [(i, j, [tuple(m) for m in pr[o[q]:o[q + 1]]], None if mk is None else mk[o[q]:o[q + 1]])
                              for q, (i, j) in enumerate(self.imagePairs.tolist())]
        return self._problems

    def permuted(self, seed):
        """The same graph with the problems, and the matches of each problem with their mask bytes, reordered."""
        rng = np.random.default_rng(seed)
        if self._problems is None:   # the same reordering on the arrays
            B, n = len(self.imagePairs), len(self.pairs)
            q = rng.permutation(B)
            rank = np.empty(B, np.int64)
            rank[q] = np.arange(B)
            prob = np.repeat(np.arange(B), np.diff(self.offsets))
            order = np.lexsort((rng.random(n), rank[prob]))
            lens = np.diff(self.offsets)[q]
            return Case.from_arrays(self.counts, self.imagePairs[q], self.pairs[order],
                                    np.concatenate([[0], np.cumsum(lens)]),
                                    None if self.mask is None else self.mask[order], self.minLength)
        probs = []
        for q in rng.permutation(len(self.problems)):
            i, j, ms, mk = self.problems[q]
            o = rng.permutation(len(ms))
            probs.append((i, j, [ms[k] for k in o], None if mk is None else [mk[k] for k in o]))
        return Case(self.counts, probs, self.minLength, self.use_mask)


class Result:
    def __init__(self, T, trackOffsets, cameraIdx, featureIdx, trackOfFeature, dropped):
        self.T, self.trackOffsets, self.cameraIdx, self.featureIdx = T, trackOffsets, cameraIdx, featureIdx
        self.trackOfFeature, self.dropped = trackOfFeature, dropped


def reference(case) -> Result:
    """The definition, read off the issue: components of the kept edges over the touched nodes, each
    dropped by the first rule that applies (oversize, conflict, short), the others ordered by their
    smallest node, their nodes ascending."""
    base = np.concatenate([[0], np.cumsum(case.counts.astype(np.int64))])
    up = {}

    def root(x):
        path = []
        while up.setdefault(x, x) != x:
            path.append(x)
            x = up[x]
        for y in path:
            up[y] = x
        return x

    for i, j, ms, mk in case.problems:
        for k, (a, b) in enumerate(ms):
            if case.use_mask and mk is not None and not mk[k]:
                continue
            ra, rb = root(int(base[i]) + a), root(int(base[j]) + b)
            if ra != rb:
                up[ra] = rb   # whichever: the order of the roots plays no part in the definition
    comps = defaultdict(list)
    for x in list(up):
        comps[root(x)].append(x)
    toff, cam, feat = [0], [], []
    tof = np.full(case.nodes, -1, np.int32)
    dropped = [0, 0, 0]
    for nodes in sorted((sorted(c) for c in comps.values()), key=lambda c: c[0]):
        images = [int(np.searchsorted(base, g, side="right")) - 1 for g in nodes]
        if len(nodes) > MAX_LEN:
            dropped[0] += 1
        elif len(set(images)) < len(nodes):
            dropped[1] += 1
        elif len(nodes) < case.minLength:
            dropped[2] += 1
        else:
            for g, i in zip(nodes, images):
                tof[g] = len(toff) - 1
                cam.append(i)
                feat.append(g - int(base[i]))
            toff.append(len(cam))
    return Result(len(toff) - 1, np.array(toff, np.int32), np.array(cam, np.int32), np.array(feat, np.int32), tof,
                  np.array(dropped, np.int64))


# ---- the shared cases

def path(L, order="ascending", minLength=2):
    """One feature in each of L images, image k matched to image k + 1."""
    ks = list(range(L - 1))
    if order == "descending":
        ks = ks[::-1]
    elif order == "shuffled":
        ks = [int(k) for k in np.random.default_rng(L).permutation(L - 1)]
    return Case([1] * L, [(k, k + 1, [(0, 0)], None) for k in ks], minLength)


def random_scene(seed=RANDOM_SEED):
    """64 images of 500 features, 200 image pairs, matches from shared 3-D point ids (1500 points, each
    image sees 500 of them in a shuffled feature order), 5 % of the matches wrong (a random feature of the
    second image), 10 % masked out, minLength 3. Seed 11: the reference counts are pinned by
    tests/test_tracks.py::test_random_scene_has_every_drop_class."""
    rng = np.random.default_rng(seed)
    nImg, nFeat, nPts, nPairs = 64, 500, 1500, 200
    seen = [rng.permutation(nPts)[:nFeat] for _ in range(nImg)]   # seen[i][f] = the point of feature f
    slot = []
    for s in seen:
        m = np.full(nPts, -1)
        m[s] = np.arange(nFeat)
        slot.append(m)
    chosen = set()
    while len(chosen) < nPairs:
        i, j = (int(v) for v in rng.integers(0, nImg, 2))
        if i != j:
            chosen.add((min(i, j), max(i, j)))
    probs = []
    for i, j in sorted(chosen):
        shared = np.nonzero((slot[i] >= 0) & (slot[j] >= 0))[0]
        ms = []
        for p in shared:
            b = int(slot[j][p])
            if rng.random() < 0.05:
                b = int(rng.integers(0, nFeat))
            ms.append((int(slot[i][p]), b))
        probs.append((i, j, ms, [int(rng.random() >= 0.10) for _ in ms]))
    return Case([nFeat] * nImg, probs, minLength=3)


def _lengths_scene(minLength):
    """Paths of 2, 3, 4, 5 and 6 images side by side: feature k of the first k + 2 images."""
    probs = [(i, i + 1, [(k, k) for k in range(5) if i + 1 < k + 2], None) for i in range(5)]
    return Case([5] * 6, probs, minLength)


def _zigzag(n):
    """Two images: A.f0 - B.f0 - A.f1 - B.f1 - ...: one component of 2 n nodes over 2 images."""
    ms = [(k, k) for k in range(n)] + [(k + 1, k) for k in range(n - 1)]
    return Case([n, n], [(0, 1, ms, None)])


def _long_conflict():
    """A path through 50 images (a long component, within nImages) with a second feature of image 20."""
    probs = [(k, k + 1, [(0, 0)], None) for k in range(49)] + [(30, 20, [(0, 1)], None)]
    return Case([2] * 50, probs)


PATH_LENGTHS = list(range(2, 41)) + [63, 64, 65, 130, 600, 4096, 4097]

CASES = {
    "B0": lambda: Case([3, 4], []),
    "no_images": lambda: Case([], []),
    "empty_problems": lambda: Case([3, 3, 3], [(0, 1, [], None), (1, 2, [], None), (0, 2, [], None)]),
    "empty_problems_around_one": lambda: Case([3, 0, 3], [(0, 1, [], None), (2, 0, [(1, 2)], None), (1, 1, [], None)]),
    "all_masked": lambda: Case([3, 3], [(0, 1, [(0, 0), (1, 1)], [0, 0]), (1, 0, [(2, 2)], [0])]),
    "one_edge": lambda: Case([2, 2], [(0, 1, [(1, 0)], None)]),
    **{f"path_L{L}": (lambda L=L: path(L)) for L in PATH_LENGTHS},
    **{f"path_L600_{o}": (lambda o=o: path(600, o)) for o in ("descending", "shuffled")},
    "path_L4096_descending": lambda: path(4096, "descending"),
    "star": lambda: Case([1] * 51, [(0, k, [(0, 0)], None) for k in range(1, 51)]),
    "star_inward": lambda: Case([2] * 9, [(k, 8, [(1, 1)], None) for k in range(8)]),
    "joined_by_the_last_edge": lambda: Case([1] * 8, [(0, 1, [(0, 0)], None), (1, 2, [(0, 0)], None),
                                                     (4, 5, [(0, 0)], None), (5, 6, [(0, 0)], None),
                                                     (7, 6, [(0, 0)], None), (6, 2, [(0, 0)], None)]),
    "duplicate_edges": lambda: Case([2, 2, 2], [(0, 1, [(0, 1), (0, 1), (1, 0)], None), (1, 0, [(1, 0)], None),
                                                (1, 2, [(1, 1), (1, 1)], None)]),
    "same_image_and_self_loop": lambda: Case([5, 3], [(0, 0, [(1, 1), (2, 3)], None), (0, 1, [(4, 0)], None)]),
    "self_loop_on_a_track": lambda: Case([2, 2], [(0, 0, [(0, 0)], None), (0, 1, [(0, 1)], None)]),
    "conflict_through_a_third_image": lambda: Case([2, 1, 2, 1], [(0, 1, [(0, 0)], None), (1, 0, [(0, 1)], None),
                                                                 (2, 3, [(1, 0)], None)]),
    "zigzag_over_two_images": lambda: _zigzag(7),
    "zigzag_long": lambda: _zigzag(40),
    "long_conflict": _long_conflict,
    **{f"min_length_{m}": (lambda m=m: _lengths_scene(m)) for m in (2, 3, 5)},
    **{f"wave_edge_{n}": (lambda n=n: Case([n - 32, 32], [(0, 1, [(k, k) for k in range(min(n - 32, 32))], None)]))
       for n in (63, 64, 65)},
    "masked_half": lambda: Case([6, 6], [(0, 1, [(k, k) for k in range(6)], [1, 0, 1, 0, 2, 255])]),
    "random_scene": random_scene,
}


# ---- the edges of the scan blocks (kTrkScanItems nodes each, eight nodes per thread of mcv_trk_place)

SCAN = N.TRK_SCAN_ITEMS
SCAN_NODES = (SCAN - 1, SCAN, SCAN + 1, 2 * SCAN, 2 * SCAN + 1)


def _cut_case(nNodes, tracks):
    """nNodes nodes and the given tracks (tuples of ascending node ids, disjoint), every other node
    untouched: a new image begins at every node of a track but its first, so a track has one node per image."""
    cuts = sorted({0} | {v for t in tracks for v in t[1:]})
    counts = np.diff(cuts + [nNodes])
    where = lambda g: (int(np.searchsorted(cuts, g, side="right")) - 1, g - cuts[int(np.searchsorted(cuts, g, side="right")) - 1])
    probs = []
    for t in tracks:
        assert all(0 <= u < v < nNodes for u, v in zip(t, t[1:]))
        for u, v in zip(t, t[1:]):
            (i, a), (j, b) = where(u), where(v)
            probs.append((i, j, [(a, b)], None))
    return Case(counts, probs)


def _scan_tracks(n, kind):
    S = SCAN
    if kind == "ends":      # nodes 0 and n - 1 in one track; the root S - 1 with its partner S
        return [(0, n - 1)] + ([(S - 1, S)] if S < n - 1 else [])
    if kind == "root_S":    # the root S; a track whose last member is n - 1
        return [(S, S + 1), (5, n - 1)]
    return [(n - 2, n - 1)]  # "tail": the only root is the partner of n - 1, every earlier node untouched


SCAN_CASES = {f"scan_{n}_{kind}": (lambda n=n, kind=kind: _cut_case(n, _scan_tracks(n, kind)))
              for n in SCAN_NODES for kind in ("ends", "root_S", "tail") if kind != "root_S" or n > SCAN + 2}
CASES.update(SCAN_CASES)


# ---- the large scenes: built with numpy from components of known membership, answered by construction

def expected_by_construction(c, node, label) -> Result:
    """The answer from the membership the generator laid down: node[k] belongs to component label[k]
    (every touched node once). The three drop rules and the ordering with numpy sorts; no union-find."""
    F = c.counts.astype(np.int64)
    base = np.concatenate([[0], np.cumsum(F)])
    node, label = np.asarray(node, np.int64), np.asarray(label, np.int64)
    assert len(np.unique(node)) == len(node)
    o = np.lexsort((node, label))
    node, label = node[o], label[o]
    first = np.concatenate([[True], label[1:] != label[:-1]])
    start = np.nonzero(first)[0]
    size = np.diff(np.concatenate([start, [len(node)]]))
    comp = np.cumsum(first) - 1                                   # 0 .. C - 1 in label order
    img = np.searchsorted(base, node, side="right") - 1
    same_img = np.concatenate([[False], (img[1:] == img[:-1]) & ~first[1:]])   # nodes ascending within a component
    conflict = np.bincount(comp, same_img, len(size)) > 0
    over = size > MAX_LEN
    conf = ~over & conflict
    short = ~over & ~conf & (size < c.minLength)
    keep = ~(over | conf | short)
    root = node[start]
    order = np.argsort(root[keep], kind="stable")                 # tracks by their smallest node
    track_of_comp = np.full(len(size), -1, np.int64)
    track_of_comp[np.nonzero(keep)[0][order]] = np.arange(int(keep.sum()))
    t = track_of_comp[comp]
    sel = t >= 0
    o2 = np.lexsort((node[sel], t[sel]))
    tn, ti = node[sel][o2], img[sel][o2]
    tof = np.full(c.nodes, -1, np.int32)
    tof[node[sel]] = t[sel]
    toff = np.concatenate([[0], np.cumsum(size[keep][order])])
    return Result(int(keep.sum()), toff.astype(np.int32), ti.astype(np.int32), (tn - base[ti]).astype(np.int32), tof,
                  np.array([over.sum(), conf.sum(), short.sum()], np.int64))


def _assemble(rng, counts, ia, fa, ib, fb, mask, minLength):
    """Edges (image, feature) - (image, feature) in a seeded random order, grouped into one problem per
    ordered image pair, the problems in a seeded random order too."""
    nImg = len(counts)
    key = ia.astype(np.int64) * nImg + ib
    keys, inv = np.unique(key, return_inverse=True)
    rank = rng.permutation(len(keys))
    order = np.lexsort((rng.random(len(key)), rank[inv]))
    lens = np.bincount(rank[inv], minlength=len(keys))
    kk = np.empty(len(keys), np.int64)
    kk[rank] = keys
    return Case.from_arrays(counts, np.stack([kk // nImg, kk % nImg], axis=1),
                            np.stack([fa, fb], axis=1)[order], np.concatenate([[0], np.cumsum(lens)]),
                            mask[order], minLength)


def _random_tree(rng, nodes):
    """A random spanning tree over the given nodes (shuffled; each hangs on a random earlier one)."""
    v = rng.permutation(nodes)
    up = (rng.random(len(v) - 1) * np.arange(1, len(v))).astype(np.int64)
    return v[1:], v[up]


OVERSIZE = MAX_LEN + 904
SCALE_CONFLICTS = 300 + 32   # of scale_scene(): the zigzags and the same-image pairs


def scale_scene(div=1, seed=21):
    """40 images of 52,500 / div features, minLength 2 (-> the case, the nodes, their components):
    features [0, 2100 / div) are full 40-image paths (long candidates), the next 30,000 / div are matched
    inside the 20 disjoint image pairs (0, 1), (2, 3), ..., then 300 / div four-node zigzags over images
    0 and 1 and 32 / div same-image pairs at the end of the last image (conflicts), one oversize component (a random spanning tree over OVERSIZE nodes spread over
    all images), the rest untouched. 10 % of the matches are masked-out decoys between random features,
    which would join components if kept. div = 40 is the sub-scene the pure-Python reference judges."""
    rng = np.random.default_rng(seed)
    nImg, F = 40, 52500 // div
    nLong, nPair, nZig, nTail = 2100 // div, 30000 // div, max(300 // div, 3), max(32 // div, 2)
    perImg = -(-OVERSIZE // nImg)
    z0 = nLong + nPair
    o0 = z0 + 2 * nZig
    assert o0 + perImg < F - 2 * nTail
    gid = lambda i, f: np.asarray(i, np.int64) * F + f
    E, node, label = [], [], []            # edges as (global node, global node); membership
    f = np.arange(nLong)
    for i in range(nImg - 1):
        E.append((gid(i, f), gid(i + 1, f)))
    node.append(gid(np.repeat(np.arange(nImg), nLong), np.tile(f, nImg)))
    label.append(np.tile(f, nImg))
    f = nLong + np.arange(nPair)
    for p in range(nImg // 2):
        E.append((gid(2 * p, f), gid(2 * p + 1, f)))
        node += [gid(2 * p, f), gid(2 * p + 1, f)]
        label += [nLong + p * nPair + np.arange(nPair)] * 2
    nl = nLong + (nImg // 2) * nPair
    k = np.arange(nZig)
    a0, a1, b0, b1 = gid(0, z0 + 2 * k), gid(0, z0 + 2 * k + 1), gid(1, z0 + 2 * k), gid(1, z0 + 2 * k + 1)
    E += [(a0, b0), (a1, b0), (a1, b1)]    # A.f0 - B.f0 - A.f1 - B.f1
    node += [a0, a1, b0, b1]
    label += [nl + k] * 4
    # two-node components inside the last image, at its end (conflicts): the only candidates whose roots
    # lie in the last scan blocks, beyond the first chunk of mcv_trk_scan (every other root has a partner
    # in a later image, so it lies in an earlier one: no kept track is rooted there, and the second scan's
    # carry shows only in offsets[T] and T, written at the last node)
    k = np.arange(nTail)
    t0, t1 = gid(nImg - 1, F - 2 * nTail + 2 * k), gid(nImg - 1, F - 2 * nTail + 2 * k + 1)
    E.append((t0, t1))
    node += [t0, t1]
    label += [nl + nZig + 1 + k] * 2
    big = gid(np.repeat(np.arange(nImg), perImg), np.tile(o0 + np.arange(perImg), nImg))[:OVERSIZE]
    E.append(_random_tree(rng, big))
    node.append(big)
    label.append(np.full(OVERSIZE, nl + nZig))
    u, v = np.concatenate([e[0] for e in E]), np.concatenate([e[1] for e in E])
    flip = rng.random(len(u)) < 0.5         # the order of an edge's two ends plays no part either
    u, v = np.where(flip, v, u), np.where(flip, u, v)
    nDecoy = len(u) // 9
    du, dv = rng.integers(0, nImg * F, nDecoy), rng.integers(0, nImg * F, nDecoy)
    mask = np.concatenate([rng.choice(np.array([1, 1, 1, 2, 255], np.uint8), len(u)), np.zeros(nDecoy, np.uint8)])
    u, v = np.concatenate([u, du]), np.concatenate([v, dv])
    c = _assemble(rng, [F] * nImg, u // F, u % F, v // F, v % F, mask, 2)
    return c, np.concatenate(node), np.concatenate(label)


def contended_scene(seed=22):
    """50 images of 2,100 features, minLength 2: one component of 100,000 nodes (2,000 seeded features of
    every image; a random spanning tree plus two extra random edges per node, about 300k edges in random
    order), dropped as oversize, beside 1,000 three-image bystander tracks on features between its own."""
    rng = np.random.default_rng(seed)
    nImg, F, nBig, nBy = 50, 2100, 2000, 1000
    pick = np.stack([rng.permutation(F) for _ in range(nImg)])           # [:, :nBig] the big component's
    big = (np.arange(nImg)[:, None] * F + pick[:, :nBig]).reshape(-1)
    free = np.sort(pick[:, nBig:], axis=1)
    tu, tv = _random_tree(rng, big)
    xu, xv = np.repeat(big, 2), big[rng.integers(0, len(big), 2 * len(big))]
    b = np.arange(nBy)
    g, k = b % 16, b // 16
    by = [(3 * g + d) * F + free[3 * g + d, k] for d in range(3)]
    u = np.concatenate([tu, xu, by[0], by[1]])
    v = np.concatenate([tv, xv, by[1], by[2]])
    c = _assemble(rng, [F] * nImg, u // F, u % F, v // F, v % F, np.ones(len(u), np.uint8), 2)
    return c, np.concatenate([big] + by), np.concatenate([np.full(len(big), nBy), b, b, b])


LARGE = {"scale": scale_scene, "contended": contended_scene, "scale_sub40": lambda: scale_scene(div=40)}


@functools.lru_cache(maxsize=None)
def _large(name):
    c, node, label = LARGE[name]()
    return c, expected_by_construction(c, node, label)


@functools.lru_cache(maxsize=None)
def case(name) -> Case:
    return _large(name)[0] if name in LARGE else CASES[name]()


@functools.lru_cache(maxsize=None)
def expected(name) -> Result:
    return _large(name)[1] if name in LARGE else reference(case(name))


# ---- the native call

def capacities(c):
    """The capacities the header documents as always enough."""
    maxObs = min(2 * int(c.offsets[-1]), c.nodes)
    return maxObs // 2, maxObs


def run(export, c, maxTracks=None, maxObs=None, want_tof=True, want_dropped=True, null=(), **override):
    """-> (return value, Result over the sentinel-filled buffers trimmed to the result, untouched).
    override replaces a scalar or an input array (counts, imagePairs, pairs, offsets, mask, nImages, B,
    minLength); null names pointers to pass as NULL."""
    mt, mo = capacities(c)
    maxTracks = mt if maxTracks is None else maxTracks
    maxObs = mo if maxObs is None else maxObs
    a = {"counts": c.counts, "imagePairs": c.imagePairs, "pairs": c.pairs, "offsets": c.offsets, "mask": c.mask}
    for k in list(override):
        if k in a:
            a[k] = override.pop(k)
    a = {k: (None if v is None else np.ascontiguousarray(v, np.uint8 if k == "mask" else np.int32)) for k, v in a.items()}
    nImages = override.pop("nImages", a["counts"].size)
    B = override.pop("B", a["offsets"].size - 1)
    minLength = override.pop("minLength", c.minLength)
    assert not override, override
    nodes = int(np.maximum(a["counts"], 0).astype(np.int64).sum())
    if nodes > 1 << 26:
        nodes = 0   # a call that is refused for its size: no buffer of that size is made for it
    out = {"trackOffsets": np.full(max(maxTracks, 0) + 1, SENTINEL, np.int32),
           "cameraIdx": np.full(max(maxObs, 0) + 1, SENTINEL, np.int32),
           "featureIdx": np.full(max(maxObs, 0) + 1, SENTINEL, np.int32),
           "trackOfFeature": np.full(nodes + 1, SENTINEL, np.int32),
           "dropped": np.full(3, SENTINEL, np.int64)}

    def ptr(name, arr, optional=False):
        if name in null or arr is None or optional:
            return None
        return (arr if arr.size else np.zeros(2, arr.dtype)).ctypes.data
    keep = [a[k] if a[k] is None or a[k].size else np.zeros(2, a[k].dtype) for k in a]   # alive during the call
    T = getattr(N.lib(), export)(ptr("counts", keep[0]), nImages, ptr("imagePairs", keep[1]), B, ptr("pairs", keep[2]),
                                 ptr("offsets", keep[3]), ptr("mask", keep[4]), minLength,
                                 ptr("trackOffsets", out["trackOffsets"]), maxTracks,
                                 ptr("cameraIdx", out["cameraIdx"]), ptr("featureIdx", out["featureIdx"]), maxObs,
                                 ptr("trackOfFeature", out["trackOfFeature"], not want_tof),
                                 ptr("dropped", out["dropped"], not want_dropped))
    untouched = all(np.all(v == SENTINEL) for v in out.values())
    if T < 0:
        return T, None, untouched
    n = int(out["trackOffsets"][T])
    # nothing beyond the result is written
    assert np.all(out["trackOffsets"][T + 1:] == SENTINEL) and np.all(out["cameraIdx"][n:] == SENTINEL)
    assert np.all(out["featureIdx"][n:] == SENTINEL) and out["trackOfFeature"][nodes] == SENTINEL
    return T, Result(T, out["trackOffsets"][:T + 1], out["cameraIdx"][:n], out["featureIdx"][:n],
                     out["trackOfFeature"][:nodes], out["dropped"]), untouched


def assert_same(got: Result, want: Result, what, tof=True, dropped=True):
    assert got.T == want.T, (what, got.T, want.T)
    for f in ("trackOffsets", "cameraIdx", "featureIdx") + (("trackOfFeature",) if tof else ()) + \
            (("dropped",) if dropped else ()):
        assert np.array_equal(getattr(got, f), getattr(want, f)), (what, f)
    if not tof:
        assert np.all(got.trackOfFeature == SENTINEL), what
    if not dropped:
        assert np.all(got.dropped == SENTINEL), what
