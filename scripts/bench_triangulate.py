#!/usr/bin/env python3
"""Track triangulation (cvTriangulateTracks / mcvTriangulateTracksDevice) timings on one MI355X.

Two seeded workloads (synthetic.track_problem, 256 cameras, sigma 1e-3, 5 % wrong observations):
  short  T = 2^20 tracks of 2..12 observations (the lane-per-track kernel)
  long   T = 2^14 tracks of 64 observations    (the workgroup-per-track kernel)
Per workload, after --warmup calls, the median and p10 - p90 of --reps calls of
  device   mcvTriangulateTracksDevice on device-resident arrays, between two device events
  host     cvTriangulateTracks on host arrays (wall clock: staging copies included)
  twin     mcvHostTriangulateTracks over 16 threads (ctypes releases the GIL; tracks in 64 chunks)
and, from one more profiled device call, the kernels' own durations (mcvProfileRead). From those:
  short  algorithmic bytes (20 B read per observation, 4 B per offset, 28 B written per track, cost and
         visible 12 B more) over the kernels' time, against 6.3 TB/s achievable: an HBM-streaming figure
         (the ray buffer's 48 B written and read back per observation is traffic the algorithm does not need);
  long   pairs per second over the kernels' time (pairs of the deduplicated rays, rejected ones included).
Writes profiles/triangulate_bench.json. --small shrinks both workloads 16x (a dry run of the script)."""
import argparse
import ctypes as C
import datetime
import json
import platform
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from minicv_amd import native as N, synthetic as S  # noqa: E402

HBM_ACHIEVABLE = 6.3e12
KERNELS = ("tri_unproject", "tri_short", "tri_long", "tri_stats")


def stats(v):
    v = np.sort(np.array(v)) * 1e3
    return {"median_ms": round(float(np.median(v)), 4), "p10_ms": round(float(v[int(0.1 * (len(v) - 1))]), 4),
            "p90_ms": round(float(v[int(np.ceil(0.9 * (len(v) - 1)))]), 4)}


def twin_chunks(cams, idx, obs, off, T, nchunks=64):
    """The host twin's calls over contiguous track ranges, each with its own rebased offsets."""
    L = N.lib()
    calls, keep = [], []
    for a, b in zip(np.linspace(0, T, nchunks + 1).astype(int)[:-1], np.linspace(0, T, nchunks + 1).astype(int)[1:]):
        if a == b:
            continue
        o = np.ascontiguousarray(off[a:b + 1] - off[a], np.int32)
        i, ob = np.ascontiguousarray(idx[off[a]:off[b]]), np.ascontiguousarray(obs[off[a]:off[b]])
        pts, cnt, cost, vis = np.empty((b - a, 3)), np.empty(b - a, np.int32), np.empty(b - a), np.empty(b - a, np.int32)
        keep.append((o, i, ob, pts, cnt, cost, vis))
        calls.append((cams.ctypes.data, len(cams), i.ctypes.data, ob.ctypes.data, o.ctypes.data, b - a, pts.ctypes.data,
                      cnt.ctypes.data, cost.ctypes.data, vis.ctypes.data))
    return calls, keep, L.mcvHostTriangulateTracks


def run(name, T, lengths, warmup, reps, seed):
    import torch
    L = N.lib()
    cams, idx, obs, off, _ = S.track_problem(T, seed, lengths=lengths, n_cameras=256, sigma=1e-3, wrong_frac=0.05)
    n = int(off[-1])
    R = np.diff(off).astype(np.int64)
    out = {"workload": name, "tracks": T, "observations": n, "cameras": 256, "seed": seed}

    d = [torch.from_numpy(a).cuda() for a in (cams, idx, obs, off)]
    pts, cnt = torch.empty((T, 3), dtype=torch.float64, device="cuda"), torch.empty(T, dtype=torch.int32, device="cuda")
    cost, vis = torch.empty(T, dtype=torch.float64, device="cuda"), torch.empty(T, dtype=torch.int32, device="cuda")
    dev_args = (d[0].data_ptr(), 256, d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), T, pts.data_ptr(),
                cnt.data_ptr(), cost.data_ptr(), vis.data_ptr())
    torch.cuda.synchronize()
    times, k = [], 0
    for r in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        k = L.mcvTriangulateTracksDevice(*dev_args)
        b.record()
        b.synchronize()
        if k < 0:
            raise RuntimeError(N.last_error())
        if r >= warmup:
            times.append(a.elapsed_time(b) * 1e-3)
    out["device_call"] = stats(times)
    out["tracks_with_point"] = k
    st = (C.c_longlong * 8)()
    L.mcvTestTriangulateStats(st)
    out["launches_syncs_copies_memsets"], out["short_long_tracks"] = list(st)[:4], list(st)[4:6]

    L.mcvProfileReset()
    L.mcvProfileEnable(1)
    L.mcvTriangulateTracksDevice(*dev_args)
    kern, ms = {}, C.c_double(0)
    for kname in KERNELS:
        c = L.mcvProfileRead(kname.encode(), C.addressof(ms))
        kern[kname] = {"launches": c, "ms": round(ms.value, 4)}
    L.mcvProfileEnable(0)
    L.mcvProfileReset()
    out["kernels"] = kern
    ksec = sum(v["ms"] for v in kern.values()) * 1e-3
    if name == "short":
        alg = 20 * n + 4 * (T + 1) + 28 * T + 12 * T
        out["algorithmic_bytes"] = alg
        out["algorithmic_TBps_over_kernel_time"] = round(alg / ksec / 1e12, 4)
        out["fraction_of_6.3TBps_hbm_streaming"] = round(alg / ksec / HBM_ACHIEVABLE, 4)
    else:
        pairs = int((R * (R - 1) // 2).sum())   # an upper bound when rays repeat; track_problem has no repeats here
        out["pairs"] = pairs
        out["pairs_per_second_over_kernel_time"] = round(pairs / ksec, 1)

    hp, hc, hcost, hvis = np.empty((T, 3)), np.empty(T, np.int32), np.empty(T), np.empty(T, np.int32)
    host_args = (cams.ctypes.data, 256, idx.ctypes.data, obs.ctypes.data, off.ctypes.data, T, hp.ctypes.data,
                 hc.ctypes.data, hcost.ctypes.data, hvis.ctypes.data)
    times = []
    for r in range(warmup + reps):
        t0 = time.perf_counter()
        if L.cvTriangulateTracks(*host_args) < 0:
            raise RuntimeError(N.last_error())
        if r >= warmup:
            times.append(time.perf_counter() - t0)
    out["host_pointer_call"] = stats(times)

    calls, keep, f = twin_chunks(cams, idx, obs, off, T)
    times = []
    with ThreadPoolExecutor(16) as ex:
        for r in range(1 + max(3, reps // 4)):
            t0 = time.perf_counter()
            got = sum(ex.map(lambda c: f(*c), calls))
            if r >= 1:
                times.append(time.perf_counter() - t0)
    out["host_twin_16_threads"] = stats(times)
    twin_pts = np.concatenate([x[3] for x in keep])
    out["equal_to_host_twin"] = bool(got == k and np.array_equal(twin_pts.view(np.uint64), hp.view(np.uint64))
                                     and np.array_equal(pts.cpu().numpy().view(np.uint64), hp.view(np.uint64)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "triangulate_bench.json"))
    a = ap.parse_args()
    if N.lib().mcvDeviceCount() <= 0:
        raise SystemExit("bench_triangulate: no HIP device visible")
    import torch
    sh = 4 if a.small else 0
    rng = np.random.default_rng(7)
    res = {"date": datetime.date.today().isoformat(), "box": f"{torch.cuda.get_device_name(0)} ({platform.node()})",
           "library": N.lib().mcvVersion().decode(), "warmup": a.warmup, "reps": a.reps,
           "workloads": [run("short", 1 << (20 - sh), rng.integers(2, 13, size=4096).tolist(), a.warmup, a.reps, 101),
                         run("long", 1 << (14 - sh), [64], a.warmup, a.reps, 102)]}
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
