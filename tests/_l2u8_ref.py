"""Reference of the uint8 L2 matcher for the tests: BFMatcher(NORM_L2).knnMatch(k = 2) on uint8 rows
restated in int64 numpy. d^2 = sum (q_k - t_k)^2 exactly, order (d^2, train index), dist =
float32(sqrt(float64(d^2))); a missing place is index -1 / distance +inf (cvMatchL2's convention)."""
import numpy as np


def match_l2_u8(q, t, block=512):
    q = np.ascontiguousarray(q, dtype=np.uint8).astype(np.int64)
    t = np.ascontiguousarray(t, dtype=np.uint8).astype(np.int64)
    nq, nt = q.shape[0], t.shape[0]
    idx = np.full(nq, -1, np.int32)
    idx2 = np.full(nq, -1, np.int32)
    d = np.full(nq, np.inf, np.float64)
    d2 = np.full(nq, np.inf, np.float64)
    if nt > 0:
        tn = (t * t).sum(axis=1)
        rows = np.arange(nq)
        for b in range(0, nq, block):
            qb = q[b:b + block]
            m = (qb * qb).sum(axis=1)[:, None] + tn[None, :] - 2 * (qb @ t.T)     # exact int64
            r = rows[:len(qb)]
            i1 = np.argmin(m, axis=1)                 # first occurrence: the lowest index of a tie
            idx[b:b + block] = i1
            d[b:b + block] = m[r, i1]
            if nt > 1:
                m[r, i1] = np.iinfo(np.int64).max
                i2 = np.argmin(m, axis=1)
                idx2[b:b + block] = i2
                d2[b:b + block] = m[r, i2]
    return idx, np.sqrt(d).astype(np.float32), idx2, np.sqrt(d2).astype(np.float32)


def assert_same(got, ref):
    """All four outputs equal; the distances bit for bit as float32."""
    gi, gd, gi2, gd2 = got
    ri, rd, ri2, rd2 = ref
    np.testing.assert_array_equal(np.asarray(gi), np.asarray(ri))
    np.testing.assert_array_equal(np.asarray(gi2), np.asarray(ri2))
    for g, r in ((gd, rd), (gd2, rd2)):
        g = np.ascontiguousarray(g, dtype=np.float32)
        r = np.ascontiguousarray(np.asarray(r).astype(np.float32))
        np.testing.assert_array_equal(g.view(np.uint32), r.view(np.uint32))


def random_u8(nq, nt, dim, seed, high=256):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, high, size=(nq, dim), dtype=np.uint8),
            rng.integers(0, high, size=(nt, dim), dtype=np.uint8))
