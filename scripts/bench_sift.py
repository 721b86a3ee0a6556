#!/usr/bin/env python3
"""SIFT detection (cvDetectFeatures mode 4) timings on one MI355X against the host twin on the same box.

Seeded smoothed-noise textures at 1920 x 1080 and 4000 x 3000, default configuration (byte descriptors).
Per size, after --warmup calls, the median and p10 - p90 of --reps calls (wall clock) of
  export  cvDetectFeatures on a host array (checks, copies, kernels, three counter reads, copies back)
  twin    mcvHostDetectFeatures on one thread (once: it takes most of a minute at the large size)
and, from one more profiled call, the durations of the stages on the stream (mcvProfileRead): pyramid
(grey + doubling, blurs, downsampling), extrema (DoG + 26 neighbours), refine, orient, order (the row
buckets) and describe. For the pyramid and extrema stages the bytes the passes move over the stage's time
is the achieved rate, to set against the HBM rate. The export's result must equal the twin's, every bit,
before a number is recorded. Writes profiles/sift_bench.json. --small-only runs 640 x 480 alone (a dry run)."""
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
from minicv_amd import native as N, opencv  # noqa: E402

STAGES = ("sift_pyramid", "sift_extrema", "sift_refine", "sift_orient", "sift_order", "sift_describe")


def stats(v):
    v = np.sort(np.array(v)) * 1e3
    return {"median_ms": round(float(np.median(v)), 4), "p10_ms": round(float(v[int(0.1 * (len(v) - 1))]), 4),
            "p90_ms": round(float(v[int(np.ceil(0.9 * (len(v) - 1)))]), 4)}


def box(a, k):
    p = np.pad(a, k // 2, mode="edge")
    c = np.pad(np.cumsum(np.cumsum(p, axis=0), axis=1), ((1, 0), (1, 0)))
    h, w = a.shape
    return (c[k:k + h, k:k + w] - c[:h, k:k + w] - c[k:k + h, :w] + c[:h, :w]) / (k * k)


def texture(w, h, seed):
    a = box(box(np.random.default_rng(seed).standard_normal((h, w)), 5), 5)
    return np.clip(np.rint(128.0 + 192.0 * a / a.std()), 0, 255).astype(np.uint8)


def pass_bytes(w, h, nl=3):
    """Bytes the pyramid and the extrema passes read and write (4-byte floats), from the sizes alone."""
    n_oct = N.sift_octaves(w, h)
    pyr = w * h + 4 * w * h * 4            # grey + doubling: the bytes in, the doubled image out
    pyr += 4 * (4 * w * h * 4)             # the base blur: two passes, each one read and one write
    ext = 0
    ow, oh = 2 * w, 2 * h
    for o in range(n_oct):
        plane = ow * oh * 4
        if o:
            pyr += 2 * plane               # downsampling: a quarter of the source read, the base written
        pyr += (nl + 2) * 4 * plane        # nl + 2 blurs
        ext += (nl + 3) * plane            # every Gaussian image once
        ow, oh = ow // 2, oh // 2
    return pyr, ext


def run(w, h, warmup, reps, seed):
    L = N.lib()
    img = texture(w, h, seed)
    t0 = time.perf_counter()
    twin = opencv._detect_features("mcvHostDetectFeatures", img, N.FEATURE_SIFT, None)
    t_twin = time.perf_counter() - t0
    times = []
    for _ in range(warmup + reps):
        t0 = time.perf_counter()
        got = opencv.detectFeatures(img)
        times.append(time.perf_counter() - t0)
    if not (np.array_equal(got.keypoints, twin.keypoints) and np.array_equal(got.descriptors, twin.descriptors)):
        raise RuntimeError(f"{w} x {h}: cvDetectFeatures differs from the host twin")
    st = (C.c_longlong * 8)()
    L.mcvTestSiftStats(st)
    out = {"width": w, "height": h, "seed": seed, "octaves": N.sift_octaves(w, h),
           "launches_syncs_copies_memsets": list(st)[:4],
           "candidates_refined_oriented_returned": list(st)[4:], "equals_host_twin": True,
           "export_host_array": stats(times[warmup:]), "host_twin_1_thread_ms": round(t_twin * 1e3, 1)}
    out["twin_over_export"] = round(out["host_twin_1_thread_ms"] / out["export_host_array"]["median_ms"], 1)
    L.mcvProfileReset()
    L.mcvProfileEnable(1)
    t0 = time.perf_counter()
    opencv.detectFeatures(img)
    wall = (time.perf_counter() - t0) * 1e3
    L.mcvProfileEnable(0)
    ms = C.c_double(0)
    prof = {}
    for k in STAGES:
        c = L.mcvProfileRead(k.encode(), C.addressof(ms))
        prof[k] = {"scopes_timed": c, "ms": round(ms.value, 4)}
    L.mcvProfileReset()
    kern = sum(p["ms"] for p in prof.values())
    pyr, ext = pass_bytes(w, h)
    out["profiled_call"] = {"wall_ms": round(wall, 4), "stages": prof, "kernels_ms": round(kern, 4),
                            "rest_of_call_ms": round(wall - kern, 4),
                            "dominant_stage": max(prof, key=lambda k: prof[k]["ms"])}
    out["pass_bytes"] = {"pyramid_GB": round(pyr / 1e9, 4), "extrema_GB": round(ext / 1e9, 4),
                         "pyramid_GB_per_s": round(pyr / 1e6 / max(prof["sift_pyramid"]["ms"], 1e-9), 1),
                         "extrema_GB_per_s": round(ext / 1e6 / max(prof["sift_extrema"]["ms"], 1e-9), 1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sift_bench.json"))
    a = ap.parse_args()
    if N.lib().mcvDeviceCount() <= 0:
        raise SystemExit("bench_sift: no HIP device visible")
    import torch
    sizes = [(640, 480, 300)] if a.small_only else [(1920, 1080, 301), (4000, 3000, 302)]
    loads = [run(w, h, a.warmup, a.reps, seed) for w, h, seed in sizes]
    res = {"date": datetime.date.today().isoformat(), "box": f"{torch.cuda.get_device_name(0)} ({platform.node()})",
           "library": N.lib().mcvVersion().decode(), "warmup": a.warmup, "reps": a.reps,
           "config": "default: {0, 3, 0.04, 10.0, 1.6, uint8}", "images": loads}
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
