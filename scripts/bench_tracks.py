#!/usr/bin/env python3
"""Track building (cvBuildTracks) timings on one MI355X against the host twin on the same box.

Two seeded workloads; each image sees nFeat of 3 nFeat world points in a shuffled feature order, the
matches of a pair are the shared points, 2 % of them wrong (a random feature of the second image):
  small   64 images x 2000 features, each image paired with its next 4
  large  256 images x 8192 features, each image paired with its next 8 (a few million matches)
Per workload, after --warmup calls, the median and p10 - p90 of --reps calls (wall clock) of
  export  cvBuildTracks on host arrays (checks, edge list, copies, kernels, copies back)
  twin    mcvHostBuildTracks on one thread
and, from one more profiled call, the durations of the kernels and of the two groups of copies on the
stream (mcvProfileRead). Every leg's outputs must equal the twin's before a number is recorded.
Writes profiles/tracks_bench.json. --small-only runs the small workload alone (a dry run)."""
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
from minicv_amd import native as N  # noqa: E402

KERNELS = ("trk_init", "trk_hook", "trk_flatten", "trk_layout", "trk_scatter", "trk_short", "trk_long",
           "trk_compact", "trk_copy")
COPIES = ("trk_upload", "trk_download")


def stats(v):
    v = np.sort(np.array(v)) * 1e3
    return {"median_ms": round(float(np.median(v)), 4), "p10_ms": round(float(v[int(0.1 * (len(v) - 1))]), 4),
            "p90_ms": round(float(v[int(np.ceil(0.9 * (len(v) - 1)))]), 4)}


def workload(nImg, nFeat, span, wrong, seed):
    rng = np.random.default_rng(seed)
    nPts = 3 * nFeat
    slot = np.full((nImg, nPts), -1, np.int32)   # slot[i, p] = the feature of point p in image i
    for i in range(nImg):
        slot[i, rng.permutation(nPts)[:nFeat]] = np.arange(nFeat, dtype=np.int32)
    imagePairs, pairs, offsets = [], [], [0]
    for i in range(nImg):
        for d in range(1, span + 1):
            j = (i + d) % nImg
            shared = np.nonzero((slot[i] >= 0) & (slot[j] >= 0))[0]
            a, b = slot[i, shared], slot[j, shared].copy()
            w = rng.random(len(shared)) < wrong
            b[w] = rng.integers(0, nFeat, int(w.sum()))
            imagePairs.append((i, j))
            pairs.append(np.stack([a, b], axis=1))
            offsets.append(offsets[-1] + len(shared))
    return (np.full(nImg, nFeat, np.int32), np.array(imagePairs, np.int32), np.ascontiguousarray(np.concatenate(pairs)),
            np.array(offsets, np.int32))


def run(name, nImg, nFeat, span, warmup, reps, seed):
    L = N.lib()
    counts, ip, pr, off = workload(nImg, nFeat, span, 0.02, seed)
    B, E, nodes = len(ip), int(off[-1]), nImg * nFeat
    maxObs = min(2 * E, nodes)
    maxTracks = maxObs // 2

    def buffers():
        return (np.empty(maxTracks + 1, np.int32), np.empty(maxObs, np.int32), np.empty(maxObs, np.int32),
                np.empty(nodes, np.int32), np.zeros(3, np.int64))

    def call(f, o):
        return f(counts.ctypes.data, nImg, ip.ctypes.data, B, pr.ctypes.data, off.ctypes.data, None, 2,
                 o[0].ctypes.data, maxTracks, o[1].ctypes.data, o[2].ctypes.data, maxObs, o[3].ctypes.data,
                 o[4].ctypes.data)

    def timed(f, o, n):
        times = []
        for r in range(n):
            t0 = time.perf_counter()
            T = call(f, o)
            times.append(time.perf_counter() - t0)
            if T < 0:
                raise RuntimeError(N.last_error())
        return T, times

    tw, dv = buffers(), buffers()
    Tt, t_twin = timed(L.mcvHostBuildTracks, tw, 1 + max(3, reps // 2))
    Td, t_dev = timed(L.cvBuildTracks, dv, warmup + reps)
    n = int(tw[0][Tt])

    def same(o):
        return bool(Td == Tt and np.array_equal(o[0][:Tt + 1], tw[0][:Tt + 1]) and np.array_equal(o[1][:n], tw[1][:n])
                    and np.array_equal(o[2][:n], tw[2][:n]) and np.array_equal(o[3], tw[3])
                    and np.array_equal(o[4], tw[4]))
    if not same(dv):
        raise RuntimeError(f"{name}: cvBuildTracks differs from the host twin")
    st = (C.c_longlong * 8)()
    L.mcvTestTracksStats(st)
    out = {"workload": name, "images": nImg, "features_per_image": nFeat, "pairs": B, "matches": E, "nodes": nodes,
           "seed": seed, "tracks": Tt, "observations": n, "dropped_oversize_conflicts_short": tw[4].tolist(),
           "launches_syncs_copies_memsets": list(st)[:4], "candidates_long": list(st)[4:6],
           "export_host_arrays": stats(t_dev[warmup:]), "host_twin_1_thread": stats(t_twin[1:])}
    out["twin_over_export"] = round(out["host_twin_1_thread"]["median_ms"] / out["export_host_arrays"]["median_ms"], 3)

    pv = dv   # pages already touched: a fresh buffer's first-touch faults are no part of the call
    for o in pv:
        o.fill(-5)
    L.mcvProfileReset()
    L.mcvProfileEnable(1)
    t0 = time.perf_counter()
    Td = call(L.cvBuildTracks, pv)
    wall = (time.perf_counter() - t0) * 1e3
    L.mcvProfileEnable(0)
    if not same(pv):
        raise RuntimeError(f"{name}: the profiled cvBuildTracks call differs from the host twin")
    ms = C.c_double(0)
    prof = {}
    for k in KERNELS + COPIES:
        c = L.mcvProfileRead(k.encode(), C.addressof(ms))
        prof[k] = {"launches_timed": c, "ms": round(ms.value, 4)}
    L.mcvProfileReset()
    kern, cop = sum(prof[k]["ms"] for k in KERNELS), sum(prof[k]["ms"] for k in COPIES)
    out["profiled_call"] = {"wall_ms": round(wall, 4), "stages": prof, "kernels_ms": round(kern, 4),
                            "copies_ms": round(cop, 4), "host_side_ms": round(wall - kern - cop, 4),
                            "copies_share_of_call": round(cop / wall, 3), "kernels_share_of_call": round(kern / wall, 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "tracks_bench.json"))
    a = ap.parse_args()
    if N.lib().mcvDeviceCount() <= 0:
        raise SystemExit("bench_tracks: no HIP device visible")
    import torch
    loads = [run("small", 64, 2000, 4, a.warmup, a.reps, 201)]
    if not a.small_only:
        loads.append(run("large", 256, 8192, 8, a.warmup, a.reps, 202))
    res = {"date": datetime.date.today().isoformat(), "box": f"{torch.cuda.get_device_name(0)} ({platform.node()})",
           "library": N.lib().mcvVersion().decode(), "warmup": a.warmup, "reps": a.reps, "workloads": loads}
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
