#!/usr/bin/env python3
"""Batched findScaled (cvFindScaledPoseBatch) against the loop of cvFindScaledPose calls on one MI355X.

Workloads (synthetic.scaled_problem per set: its own seed, focal length, outlier share and true scale):
  sfm200    256 sets of 200 observations, 4 candidate poses each (R / R2 with +-t): P = 1024
  sfm1000   256 sets of 1000 observations, 4 candidate poses each:                  P = 1024
  one500    one set of 500 observations, one pose:                                 P = 1
Per workload, both legs on host arrays (wall clock, staging copies included), after --warmup runs the
median and p10 - p90 of --reps runs of
  batch   one cvFindScaledPoseBatch call
  loop    P cvFindScaledPose calls, one per problem, on the same inputs (this project's path before
          the batch existed)
Every leg's costs, scales and evaluated counts are compared bit for bit with the loop's. One more
profiled batch call gives the sweep kernel's own duration (mcvProfileRead "scaled_batch_costs").
Writes profiles/batch_scaled_bench.json. --small shrinks the SfM workloads to 16 sets (a dry run)."""
import argparse
import ctypes as C
import datetime
import json
import platform
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from minicv_amd import camera as CM, native as N, synthetic as S  # noqa: E402


def stats(v):
    v = np.sort(np.array(v)) * 1e3
    return {"median_ms": round(float(np.median(v)), 4), "p10_ms": round(float(v[int(0.1 * (len(v) - 1))]), 4),
            "p90_ms": round(float(v[int(np.ceil(0.9 * (len(v) - 1)))]), 4)}


def problems(n_sets, n_obs, poses_per_set, seed0):
    """-> cams (P, 14), rots (P, 9), trans (P, 3), setIdx (P,), world (R, 3), obs (R, 2), offsets (S + 1,)"""
    cams, rots, trans, idx, world, obs = [], [], [], [], [], []
    for s in range(n_sets):
        src, pose, W, O, _ = S.scaled_problem(n_obs, seed=seed0 + s, outlier_frac=0.2 + 0.1 * (s % 4), sigma=1e-3,
                                              true_scale=1.5 + 0.01 * s, focal=(1.0 + 0.002 * s, 1.0 + 0.001 * s))
        R2 = S.rotation([1.0, -0.4, 0.2], np.deg2rad(3.0)) @ pose.Rotation
        for k in range(poses_per_set):
            cams.append(np.concatenate([src.location, src.forward, src.up, src.right, src.focal]))
            rots.append((R2 if k & 2 else pose.Rotation).reshape(9))
            trans.append(-pose.Translation if k & 1 else pose.Translation)
            idx.append(s)
        world.append(W)
        obs.append(O)
    off = np.zeros(n_sets + 1, np.int32)
    off[1:] = np.cumsum([w.shape[0] for w in world])
    c = np.ascontiguousarray
    return (c(np.array(cams, np.float64)), c(np.array(rots, np.float64)), c(np.array(trans, np.float64)),
            c(np.array(idx, np.int32)), c(np.concatenate(world)), c(np.concatenate(obs)), off)


def run(name, n_sets, n_obs, poses_per_set, warmup, reps, seed0):
    L = N.lib()
    cams, rots, trans, idx, world, obs, off = problems(n_sets, n_obs, poses_per_set, seed0)
    P = len(idx)
    out = {"workload": name, "sets": n_sets, "observations_per_set": n_obs, "problems": P,
           "candidate_observation_terms": int(sum(2 * int(off[s + 1] - off[s]) ** 2 for s in idx))}

    bc, bs, be = np.empty(P), np.empty(P), np.empty(P, np.int32)
    batch_args = (cams.ctypes.data, rots.ctypes.data, trans.ctypes.data, idx.ctypes.data, P, world.ctypes.data,
                  obs.ctypes.data, off.ctypes.data, n_sets, bc.ctypes.data, bs.ctypes.data, be.ctypes.data)
    lc, ls, le = np.empty(P), np.empty(P), np.empty(P, np.int32)
    loop_args = [(0.01, cams[p].ctypes.data, world[off[idx[p]]:].ctypes.data, obs[off[idx[p]]:].ctypes.data,
                  int(off[idx[p] + 1] - off[idx[p]]), rots[p].ctypes.data, trans[p].ctypes.data,
                  lc[p:].ctypes.data, ls[p:].ctypes.data) for p in range(P)]

    def batch():
        if L.cvFindScaledPoseBatch(*batch_args) < 0:
            raise RuntimeError(N.last_error())

    def loop():
        f = L.cvFindScaledPose
        for p, a in enumerate(loop_args):
            k = f(*a)
            if k < 0:
                raise RuntimeError(N.last_error())
            le[p] = k

    for leg, fn in (("loop", loop), ("batch", batch)):
        times = []
        for r in range(warmup + reps):
            t0 = time.perf_counter()
            fn()
            if r >= warmup:
                times.append(time.perf_counter() - t0)
        out[leg] = stats(times)
    out["batch_equals_loop_bit_for_bit"] = bool(np.array_equal(bc.view(np.uint64), lc.view(np.uint64)) and
                                                np.array_equal(bs.view(np.uint64), ls.view(np.uint64)) and
                                                np.array_equal(be, le))
    out["problems_with_finite_cost"] = int(np.isfinite(bc).sum())
    out["loop_over_batch"] = round(out["loop"]["median_ms"] / out["batch"]["median_ms"], 2)
    st = (C.c_longlong * 8)()
    L.mcvTestScaledBatchStats(st)
    out["launches_syncs_copies_memsets"], out["device_problems_tiles"] = list(st)[:4], list(st)[4:6]

    L.mcvProfileReset()
    L.mcvProfileEnable(1)
    batch()
    ms = C.c_double(0)
    c = L.mcvProfileRead(b"scaled_batch_costs", C.addressof(ms))
    L.mcvProfileEnable(0)
    L.mcvProfileReset()
    out["sweep_kernel"] = {"launches": c, "ms": round(ms.value, 4)}
    if ms.value > 0:
        out["sweep_terms_per_second"] = round(out["candidate_observation_terms"] / (ms.value * 1e-3), 1)
    if not out["batch_equals_loop_bit_for_bit"]:
        raise SystemExit(f"bench_batch_scaled: {name}: the batch differs from the loop of single calls")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "batch_scaled_bench.json"))
    a = ap.parse_args()
    if N.lib().mcvDeviceCount() <= 0:
        raise SystemExit("bench_batch_scaled: no HIP device visible")
    import torch
    sets = 16 if a.small else 256
    res = {"date": datetime.date.today().isoformat(), "box": f"{torch.cuda.get_device_name(0)} ({platform.node()})",
           "library": N.lib().mcvVersion().decode(), "warmup": a.warmup, "reps": a.reps,
           "workloads": [run("sfm200", sets, 200, 4, a.warmup, a.reps, 1000),
                         run("sfm1000", sets, 1000, 4, a.warmup, a.reps, 2000),
                         run("one500", 1, 500, 1, a.warmup, a.reps, 3000)]}
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
