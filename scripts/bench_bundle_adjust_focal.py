#!/usr/bin/env python3
"""Bundle adjustment with focal groups (cvBundleAdjustFocal) timings on one MI355X.

The two seeded workloads of bench_bundle_adjust.py (small: 64 cameras x 20 000 tracks, large: 256 cameras
x 200 000 tracks; at most 10 LM iterations, the other settings at their defaults). Per workload, after
--warmup calls, the median and p10 - p90 of --reps calls (wall clock, host arrays in and out) of
  1. cvBundleAdjust of this library and, with --parent-lib, of the parent commit's library, in turns
     within one loop: they must agree within the spread the loop reports;
  2. cvBundleAdjustFocal with focalMode 0, which runs cvBundleAdjust's kernels: the same criterion;
  3. focalMode 1 and 2, with one group for all cameras and with null groups: time per call, PCG
     iterations, and the stream time of one PCG iteration from one more profiled call (mcvProfileRead).
Every variant's cameras, points and summary must equal its host twin's bit for bit before a number is
recorded (focalMode 0 and the parent's library: cvBundleAdjust's twin). Writes
profiles/bundle_adjust_focal_bench.json. --small-only runs the small workload alone."""
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
sys.path.insert(0, str(Path(__file__).resolve().parent))
from bench_bundle_adjust import stats, workload  # noqa: E402
from minicv_amd import native as N  # noqa: E402


def bits_equal(a, b):
    return bool(np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and
                np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64)))


def run(name, nCam, T, warmup, reps, seed, parent):
    L = N.lib()
    cams, fixed, idx, obs, off, pts = workload(nCam, T, seed)
    base_cfg = N.BaConfig.default(maxIterations=10)
    one = np.zeros(nCam, np.int32)

    def plain(lib):
        def f(o):
            return lib.cvBundleAdjust(cams.ctypes.data, nCam, fixed.ctypes.data, idx.ctypes.data, obs.ctypes.data,
                                      off.ctypes.data, T, pts.ctypes.data, C.addressof(base_cfg), o[0].ctypes.data,
                                      o[1].ctypes.data, C.addressof(o[2]))
        return f

    def focal(export, mode, group):
        cfg = N.BaFocalConfig.default(mode, maxIterations=10)

        def f(o):
            return getattr(L, export)(cams.ctypes.data, nCam, fixed.ctypes.data, None if group is None else group.ctypes.data,
                                      None, idx.ctypes.data, obs.ctypes.data, off.ctypes.data, T, pts.ctypes.data,
                                      C.addressof(cfg), o[0].ctypes.data, o[1].ctypes.data, C.addressof(o[2]))
        return f

    def buffers(summary):
        return np.empty_like(cams), np.empty_like(pts), summary()

    def once(f, o):
        t0 = time.perf_counter()
        k = f(o)
        dt = time.perf_counter() - t0
        if k < 0:
            raise RuntimeError(N.last_error())
        return dt

    # the twins, once each
    tw_plain = buffers(N.BaSummary)
    once(lambda o: L.mcvHostBundleAdjust(cams.ctypes.data, nCam, fixed.ctypes.data, idx.ctypes.data, obs.ctypes.data,
                                         off.ctypes.data, T, pts.ctypes.data, C.addressof(base_cfg), o[0].ctypes.data,
                                         o[1].ctypes.data, C.addressof(o[2])), tw_plain)
    variants = {"cvBundleAdjust": (plain(L), N.BaSummary, tw_plain)}
    if parent is not None:
        variants["cvBundleAdjust_parent"] = (plain(parent), N.BaSummary, tw_plain)
    variants["focalMode0"] = (focal("cvBundleAdjustFocal", 0, one), N.BaFocalSummary, tw_plain)
    for mode in (1, 2):
        for gname, group in (("one_group", one), ("null_groups", None)):
            tw = buffers(N.BaFocalSummary)
            once(focal("mcvHostBundleAdjustFocal", mode, group), tw)
            variants[f"focalMode{mode}_{gname}"] = (focal("cvBundleAdjustFocal", mode, group), N.BaFocalSummary, tw)

    out, times, bufs = {}, {k: [] for k in variants}, {k: buffers(v[1]) for k, v in variants.items()}
    for r in range(warmup + reps):          # the variants in turns, so a drift of the box reaches all of them
        for k, (f, _, _) in variants.items():
            dt = once(f, bufs[k])
            if r >= warmup:
                times[k].append(dt)
    for k, (f, _, tw) in variants.items():
        o = bufs[k]
        if not bits_equal(o, tw):
            raise RuntimeError(f"{name}: {k} differs from its host twin")
        sm = o[2].as_dict()
        want = tw[2].as_dict()
        if {q: sm[q] for q in want} != want:
            raise RuntimeError(f"{name}: {k}'s summary differs from its host twin's")
        stage = "ba_cg_iteration" if k.startswith("cvBundleAdjust") or k == "focalMode0" else "baf_cg_iteration"
        ms = C.c_double(0)
        prof_ms = None
        if k != "cvBundleAdjust_parent":     # the profile hooks read this library's scopes
            L.mcvProfileReset()
            L.mcvProfileEnable(1)
            once(f, o)
            L.mcvProfileEnable(0)
            L.mcvProfileRead(stage.encode(), C.addressof(ms))
            prof_ms = ms.value
            L.mcvProfileReset()
        out[k] = dict(stats(times[k]), iterations=sm["iterations"], cgIterations=sm["cgIterations"],
                      finalCost=sm["finalCost"], freeFocalGroups=sm.get("freeFocalGroups"),
                      cg_stream_ms=None if prof_ms is None else round(prof_ms, 4),
                      cg_iteration_us=None if prof_ms is None or not sm["cgIterations"] else
                      round(1e3 * prof_ms / sm["cgIterations"], 3))
    ref = out["cvBundleAdjust"]
    spread = ref["p90_ms"] - ref["p10_ms"]
    for k, v in out.items():
        v["over_cvBundleAdjust"] = round(v["median_ms"] / ref["median_ms"], 4)
        v["median_minus_cvBundleAdjust_ms"] = round(v["median_ms"] - ref["median_ms"], 4)
    return {"workload": name, "cameras": nCam, "tracks": T, "observations": int(off[-1]), "seed": seed,
            "cvBundleAdjust_p10_p90_spread_ms": round(spread, 4), "variants": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--parent-lib", default=None, help="libMiniCVNative.so built from the parent commit")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bundle_adjust_focal_bench.json"))
    a = ap.parse_args()
    if N.lib().mcvDeviceCount() <= 0:
        raise SystemExit("bench_bundle_adjust_focal: no HIP device visible")
    parent = None
    if a.parent_lib:
        parent = C.CDLL(a.parent_lib)
        parent.cvBundleAdjust.restype, parent.cvBundleAdjust.argtypes = N.SIGNATURES["cvBundleAdjust"]
    import torch
    loads = [run("small", 64, 20000, a.warmup, a.reps, 301, parent)]
    if not a.small_only:
        loads.append(run("large", 256, 200000, a.warmup, a.reps, 302, parent))
    res = {"date": datetime.date.today().isoformat(), "box": f"{torch.cuda.get_device_name(0)} ({platform.node()})",
           "library": N.lib().mcvVersion().decode(), "parent_library": bool(a.parent_lib), "warmup": a.warmup,
           "reps": a.reps, "workloads": loads}
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
