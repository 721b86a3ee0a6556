#!/usr/bin/env python3
"""Kernel time of the LMedS rank selection (lmeds.hip) against the exact scalar count sweep
(launch_h_verify, op-by-op error) on the same homography models and points, from HIP events
(mcvProfileEnable): N correspondences x K fixed hypotheses, once on a RANSAC-like problem and once with
N copies of one correspondence (all errors equal: the LDS-atomic contention worst case).
Prints one JSON line per case."""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from minicv_amd import native as N, synthetic as S  # noqa: E402


def event_ms(name, fn, reps):
    L = N.lib()
    fn()   # warm-up (module load, allocations)
    L.mcvProfileReset()
    L.mcvProfileEnable(1)
    for _ in range(reps):
        fn()
    ms = C.c_double(0)
    k = L.mcvProfileRead(name.encode(), C.addressof(ms))
    L.mcvProfileEnable(0)
    L.mcvProfileReset()
    if k != reps:
        raise RuntimeError(f"{name}: {k} timed launches, expected {reps}")
    return ms.value / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--hyps", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    L = N.lib()
    src, dst, _ = S.homography_problem(a.n, 1)
    pts = np.ascontiguousarray(np.concatenate([src, dst], axis=1).astype(np.float32))
    models = np.zeros((a.hyps, 8), dtype=np.float32)
    m9, mf, idx = np.zeros(9), np.zeros(9, dtype=np.float32), np.zeros(4, dtype=np.int32)
    for h in range(a.hyps):   # the host twin's hypotheses (status 1 models only; others keep the zero model)
        if L.mcvHostHypothesis(N.MODEL_HOMOGRAPHY, pts.ctypes.data, a.n, 1, h, m9.ctypes.data, mf.ctypes.data,
                               idx.ctypes.data) == 1:
            models[h] = mf[:8]
    vals = np.zeros(a.hyps, dtype=np.float32)
    counts = np.zeros(a.hyps, dtype=np.int32)
    for tag, p in (("ransac-like", pts), ("all-equal", np.ascontiguousarray(np.tile(pts[:1], (a.n, 1))))):
        def select():
            ok = L.mcvTestErrorRank(N.MODEL_HOMOGRAPHY, p.ctypes.data, a.n, models.ctypes.data, a.hyps, 0, a.n // 2,
                                    vals.ctypes.data)
            N.check(ok == 1, "mcvTestErrorRank")

        def sweep():
            ok = L.mcvTestHomographySweep(p.ctypes.data, a.n, models.ctypes.data, a.hyps, 2.5e-5, 0, counts.ctypes.data)
            N.check(ok == 1, "mcvTestHomographySweep")

        sel = event_ms("lmeds_select", select, a.reps)
        swp = event_ms("h_verify_scalar", sweep, a.reps)
        print(json.dumps({"case": tag, "n": a.n, "hyps": a.hyps, "select_ms": round(sel, 3),
                          "scalar_sweep_ms": round(swp, 3), "ratio": round(sel / swp, 2)}), flush=True)


if __name__ == "__main__":
    main()
