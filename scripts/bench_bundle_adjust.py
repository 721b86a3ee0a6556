#!/usr/bin/env python3
"""Bundle adjustment (cvBundleAdjust) timings on one MI355X against the host twin on the same box.

Two seeded workloads: cameras on a ring looking at the origin, world points in [-1, 1]^3, every track
seen by 2 - 12 neighbouring cameras with 5e-4 of noise on the observations; the first two cameras are
fixed, the others start 2e-3 rad and 5e-3 units off, the points 0.02 off (a triangulation's error):
  small   64 cameras x  20 000 tracks
  large  256 cameras x 200 000 tracks
Both run at most 10 LM iterations with the other settings at their defaults. Per workload, after
--warmup calls, the median and p10 - p90 of --reps calls (wall clock) of
  export  cvBundleAdjust on host arrays (checks, camera-side CSR, copies, kernels, copies back)
  twin    mcvHostBundleAdjust on one thread (--twin-reps calls after one warm-up)
and, from one more profiled call, the durations of the stages on the stream (mcvProfileRead). The
export's cameras, points and summary must equal the twin's bit for bit before a number is recorded.
Writes profiles/bundle_adjust_bench.json. --small-only runs the small workload alone (a dry run)."""
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
from minicv_amd import camera as CM  # noqa: E402
from minicv_amd import native as N  # noqa: E402

STAGES = ("ba_upload", "ba_setup", "ba_cost", "ba_linearize", "ba_system", "ba_cg_iteration", "ba_trial_update",
          "ba_download")
# device bytes per observation: A, B, r (20 doubles), the observation, cameraIdx, obsTrack, camObs, the used byte
BYTES_PER_OBSERVATION = 20 * 8 + 16 + 3 * 4 + 1
# per track: two copies of the point, V, h, Vinv, t, y, the offsets and queue entries, the used byte
BYTES_PER_TRACK = (2 * 3 + 6 + 3 + 6 + 3 + 3) * 8 + 2 * 4 + 1
# per camera: two copies, U, g, L, b, x, r, z, p, q, p.q, the segment pointer, the fixed and active bytes
BYTES_PER_CAMERA = (2 * 14 + 21 + 6 + 21 + 6 + 5 * 6 + 1) * 8 + 4 + 2


def stats(v):
    v = np.sort(np.array(v)) * 1e3
    return {"median_ms": round(float(np.median(v)), 4), "p10_ms": round(float(v[int(0.1 * (len(v) - 1))]), 4),
            "p90_ms": round(float(v[int(np.ceil(0.9 * (len(v) - 1)))]), 4)}


def cayley(w):
    a = np.asarray(w, float) / 2
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + (2 / (1 + a @ a)) * (K + K @ K)


def workload(nCam, T, seed):
    rng = np.random.default_rng(seed)
    cams = CM.cameras_array([CM.lookAt((8 * np.cos(a), 8 * np.sin(a), 1.5), (0, 0, 0), (0, 0, 1), (2.0, 2.0))
                             for a in 2 * np.pi * np.arange(nCam) / nCam])
    world = rng.uniform(-1, 1, (T, 3))
    lens = rng.integers(2, 13, T)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    trk = np.repeat(np.arange(T), lens)
    within = np.arange(off[-1]) - off[trk]
    idx = ((rng.integers(0, nCam, T)[trk] + within) % nCam).astype(np.int32)
    c = cams[idx]
    d = world[trk] - c[:, 0:3]
    pc = np.stack([(d * c[:, 9:12]).sum(1), (d * c[:, 6:9]).sum(1), (d * c[:, 3:6]).sum(1)], axis=1)
    obs = c[:, 12:14] * pc[:, :2] / pc[:, 2:3] + rng.normal(0, 5e-4, (len(idx), 2))
    start = cams.copy()
    for j in range(2, nCam):
        R = cayley(rng.normal(0, 2e-3, 3)) @ np.stack([cams[j, 9:12], cams[j, 6:9], cams[j, 3:6]])
        start[j, 9:12], start[j, 6:9], start[j, 3:6] = R[0], R[1], R[2]
        start[j, 0:3] += rng.normal(0, 5e-3, 3)
    fixed = np.zeros(nCam, np.uint8)
    fixed[:2] = 1
    return start, fixed, idx, np.ascontiguousarray(obs), off, world + rng.normal(0, 0.02, world.shape)


def run(name, nCam, T, warmup, reps, twin_reps, seed):
    L = N.lib()
    cams, fixed, idx, obs, off, pts = workload(nCam, T, seed)
    cfg = N.BaConfig.default(maxIterations=10)

    def call(f, o):
        return f(cams.ctypes.data, nCam, fixed.ctypes.data, idx.ctypes.data, obs.ctypes.data, off.ctypes.data, T,
                 pts.ctypes.data, C.addressof(cfg), o[0].ctypes.data, o[1].ctypes.data, C.addressof(o[2]))

    def timed(f, o, n):
        times = []
        for r in range(n):
            t0 = time.perf_counter()
            k = call(f, o)
            times.append(time.perf_counter() - t0)
            if k < 0:
                raise RuntimeError(N.last_error())
        return times

    def buffers():
        return np.empty_like(cams), np.empty_like(pts), N.BaSummary()

    tw, dv = buffers(), buffers()
    t_twin = timed(L.mcvHostBundleAdjust, tw, 1 + twin_reps)
    t_dev = timed(L.cvBundleAdjust, dv, warmup + reps)

    def same(o):
        return bool(np.array_equal(o[0].view(np.uint64), tw[0].view(np.uint64)) and
                    np.array_equal(o[1].view(np.uint64), tw[1].view(np.uint64)) and bytes(o[2]) == bytes(tw[2]))
    if not same(dv):
        raise RuntimeError(f"{name}: cvBundleAdjust differs from the host twin")
    st = (C.c_longlong * 8)()
    L.mcvTestBundleAdjustStats(st)
    n = int(off[-1])
    out = {"workload": name, "cameras": nCam, "tracks": T, "observations": n, "seed": seed,
           "config": {k: getattr(cfg, k) for k, _ in cfg._fields_}, "summary": tw[2].as_dict(),
           "launches_syncs_copies_memsets": list(st)[:4], "linearizations_trials_chunks_segments": list(st)[4:8],
           "export_host_arrays": stats(t_dev[warmup:]), "host_twin_1_thread": stats(t_twin[1:]),
           "device_bytes_per_observation": BYTES_PER_OBSERVATION,
           "device_bytes": BYTES_PER_OBSERVATION * n + BYTES_PER_TRACK * T + BYTES_PER_CAMERA * nCam + 27 * 8 * int(st[7])}
    out["twin_over_export"] = round(out["host_twin_1_thread"]["median_ms"] / out["export_host_arrays"]["median_ms"], 3)

    pv = dv   # pages already touched: a fresh buffer's first-touch faults are no part of the call
    pv[0].fill(-5)
    pv[1].fill(-5)
    L.mcvProfileReset()
    L.mcvProfileEnable(1)
    t0 = time.perf_counter()
    call(L.cvBundleAdjust, pv)
    wall = (time.perf_counter() - t0) * 1e3
    L.mcvProfileEnable(0)
    if not same(pv):
        raise RuntimeError(f"{name}: the profiled cvBundleAdjust call differs from the host twin")
    ms = C.c_double(0)
    prof = {}
    for k in STAGES:
        c = L.mcvProfileRead(k.encode(), C.addressof(ms))
        prof[k] = {"launches_timed": c, "ms": round(ms.value, 4)}
    L.mcvProfileReset()
    dev = sum(p["ms"] for p in prof.values())
    out["profiled_call"] = {"wall_ms": round(wall, 4), "stages": prof, "stream_ms": round(dev, 4),
                            "host_side_ms": round(wall - dev, 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--twin-reps", type=int, default=3, help="timed twin calls after one warm-up (a large call takes a minute)")
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bundle_adjust_bench.json"))
    a = ap.parse_args()
    if N.lib().mcvDeviceCount() <= 0:
        raise SystemExit("bench_bundle_adjust: no HIP device visible")
    import torch
    loads = [run("small", 64, 20000, a.warmup, a.reps, a.twin_reps, 301)]
    if not a.small_only:
        loads.append(run("large", 256, 200000, a.warmup, a.reps, a.twin_reps, 302))
    res = {"date": datetime.date.today().isoformat(), "box": f"{torch.cuda.get_device_name(0)} ({platform.node()})",
           "library": N.lib().mcvVersion().decode(), "warmup": a.warmup, "reps": a.reps, "twin_reps": a.twin_reps, "workloads": loads}
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
