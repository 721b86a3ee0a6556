#!/usr/bin/env python3
"""Batched SIFT detection (cvDetectFeaturesBatch) against a loop of cvDetectFeatures calls over the same
images, in one process on one MI355X.

Seeded smoothed-noise textures from host arrays, default configuration (byte descriptors). Three batches:
256 images of 320 x 240, 64 of 640 x 480 and 16 of 1920 x 1080, and one image of each size. Per batch,
after --warmup rounds, the median and p10 - p90 of --reps rounds (wall clock) of
  batch   one cvDetectFeaturesBatch call and its cvFreeFeaturesBatch
  loop    cvDetectFeatures and cvFreeFeatures on every image in turn
their ratio (loop over batch: above 1 the batch is faster), the batch's stats8 (launches, synchronisations,
copies, memsets, candidates, refined, oriented, returned), the workspace bytes of its plan and, from one
more profiled call, the durations of its stages on the stream (mcvProfileRead). Every image's result of the
batch must equal the single call's, every bit; equals_single records it. Writes
profiles/sift_batch_bench.json. --small-only runs 8 images of 160 x 120 alone (a dry run)."""
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
sys.path.insert(0, str(ROOT / "scripts"))
from minicv_amd import native as N, opencv  # noqa: E402
from bench_sift import stats, texture  # noqa: E402

STAGES = ("sift_batch_pyramid", "sift_batch_extrema", "sift_batch_refine", "sift_batch_orient", "sift_batch_order",
          "sift_batch_describe")


def run(b, w, h, warmup, reps, seed):
    L = N.lib()
    imgs = [texture(w, h, seed + i) for i in range(b)]
    ims = (N.mcvImage * b)(*[N.mcvImage(a.ctypes.data, w, h, 1, 0) for a in imgs])
    res = (N.DetectorResult * b)()
    got = opencv.detectFeaturesBatch(imgs)
    equal = all(np.array_equal(g.keypoints, o.keypoints) and np.array_equal(g.descriptors, o.descriptors)
                for g, o in zip(got, (opencv.detectFeatures(a) for a in imgs)))

    def batch_call():
        total = L.cvDetectFeaturesBatch(C.addressof(ims), b, N.FEATURE_SIFT, None, C.addressof(res))
        if total < 0:
            raise RuntimeError(N.last_error())
        L.cvFreeFeaturesBatch(C.addressof(res), b)
        return total

    def loop_calls():
        total = 0
        for a in imgs:
            p = L.cvDetectFeatures(a.ctypes.data, w, h, 1, N.FEATURE_SIFT, None)
            if not p:
                raise RuntimeError(N.last_error())
            total += C.cast(p, C.POINTER(N.DetectorResult)).contents.PointCount
            L.cvFreeFeatures(p)
        return total

    tb, tl = [], []
    for _ in range(warmup + reps):   # the two alternate, so a drift of the box falls on both
        t0 = time.perf_counter()
        nb = batch_call()
        t1 = time.perf_counter()
        nl = loop_calls()
        t2 = time.perf_counter()
        tb.append(t1 - t0)
        tl.append(t2 - t1)
    assert nb == nl == sum(len(g) for g in got)
    batch_call()
    st = (C.c_longlong * 8)()
    L.mcvTestSiftBatchStats(st)
    plan = (C.c_longlong * 8)()
    assert L.mcvTestSiftBatchPlan(C.addressof(ims), b, N.FEATURE_SIFT, None, plan) == 0
    out = {"images": b, "width": w, "height": h, "seed": seed, "octaves": N.sift_octaves(w, h), "keypoints": int(nb),
           "equals_single": bool(equal), "batch": stats(tb[warmup:]), "loop_of_single_calls": stats(tl[warmup:]),
           "launches_syncs_copies_memsets": list(st)[:4], "candidates_refined_oriented_returned": list(st)[4:],
           "loop_launches": b * N.sift_launches(w, h), "loop_syncs": b * N.SIFT_SYNCS,
           "workspace_bytes": int(plan[6])}
    out["loop_over_batch"] = round(out["loop_of_single_calls"]["median_ms"] / out["batch"]["median_ms"], 3)
    L.mcvProfileReset()
    L.mcvProfileEnable(1)
    t0 = time.perf_counter()
    batch_call()
    wall = (time.perf_counter() - t0) * 1e3
    L.mcvProfileEnable(0)
    ms = C.c_double(0)
    prof = {}
    for k in STAGES:
        c = L.mcvProfileRead(k.encode(), C.addressof(ms))
        prof[k] = {"scopes_timed": c, "ms": round(ms.value, 4)}
    L.mcvProfileReset()
    kern = sum(p["ms"] for p in prof.values())
    out["profiled_call"] = {"wall_ms": round(wall, 4), "stages": prof, "kernels_ms": round(kern, 4),
                            "rest_of_call_ms": round(wall - kern, 4),
                            "dominant_stage": max(prof, key=lambda k: prof[k]["ms"])}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sift_batch_bench.json"))
    a = ap.parse_args()
    if N.lib().mcvDeviceCount() <= 0:
        raise SystemExit("bench_sift_batch: no HIP device visible")
    import torch
    shapes = [(8, 160, 120, 400)] if a.small_only else [(256, 320, 240, 1000), (64, 640, 480, 2000),
                                                        (16, 1920, 1080, 3000), (1, 320, 240, 1000),
                                                        (1, 640, 480, 2000), (1, 1920, 1080, 3000)]
    loads = [run(b, w, h, a.warmup, a.reps, seed) for b, w, h, seed in shapes]
    res = {"date": datetime.date.today().isoformat(), "box": f"{torch.cuda.get_device_name(0)} ({platform.node()})",
           "library": N.lib().mcvVersion().decode(), "warmup": a.warmup, "reps": a.reps,
           "config": "default: {0, 3, 0.04, 10.0, 1.6, uint8}",
           "loop_over_batch": "median of the loop of single calls / median of the batch call; above 1 the batch is faster",
           "batches": loads}
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
