#!/usr/bin/env python3
"""Evaluate time of the affine family (MCV_MODEL_AFFINE, MCV_MODEL_SIMILARITY) beside the homography
evaluate of the same build, and the affine sweep kernel beside the homography's certified sweep.

One process, one MI355X, device-resident points (N correspondences), --hyps fixed hypotheses from the
Philox sampler in one mcvRansacEvaluate call (generate + sweep + best key), HIP events around each
call on one stream, --warmup calls per leg, then --reps calls per leg with the legs alternating. The
homography leg runs with mcvTestHStaging(2): the single full certified sweep. A second pass of --reps
alternating calls under mcvProfileEnable reads each call's sweep kernel alone ("a_verify", "h_verify").
The LMedS selection kernel is measured once (mean of 3 launches after a warm-up) on --rank-hyps host-twin
models of the affine and of the homography scene. Reports medians and p10 - p90, and writes one JSON
document (--out)."""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from minicv_amd import device as D, native as N, opencv, synthetic as S  # noqa: E402


def stats(v):
    v = np.sort(np.array(v))
    return {"median_ms": round(float(np.median(v)), 4), "p10_ms": round(float(v[int(0.1 * (len(v) - 1))]), 4),
            "p90_ms": round(float(v[int(np.ceil(0.9 * (len(v) - 1)))]), 4), "min_ms": round(float(v[0]), 4),
            "max_ms": round(float(v[-1]), 4)}


def profile_read(name):
    ms = C.c_double(0)
    k = N.lib().mcvProfileRead(name.encode(), C.addressof(ms))
    return k, ms.value


def host_models(model, pts, hyps, width):
    L = N.lib()
    out = np.zeros((hyps, width), dtype=np.float32)
    m9, mf, idx = np.zeros(9), np.zeros(9, dtype=np.float32), np.zeros(4, dtype=np.int32)
    for h in range(hyps):
        if L.mcvHostHypothesis(model, pts.ctypes.data, pts.shape[0], 1, h, m9.ctypes.data, mf.ctypes.data,
                               idx.ctypes.data) == 1:
            out[h] = mf[:width]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--hyps", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rank-hyps", type=int, default=4096)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "affine_bench.json"))
    a = ap.parse_args()
    L = N.lib()
    if L.mcvDeviceCount() <= 0:
        raise SystemExit("bench_affine: no HIP device (this measurement has no CPU form)")
    import torch
    dev = torch.device("cuda:0")
    n, hyps = a.n, a.hyps
    scenes = {}
    src, dst, _, _ = S.affine_problem(n, 1, outlier_frac=0.5)
    scenes["affine"] = (N.MODEL_AFFINE, np.ascontiguousarray(np.concatenate([src, dst], 1).astype(np.float32)), 2.0)
    src, dst, _, _ = S.affine_problem(n, 2, outlier_frac=0.5, similarity=True)
    scenes["similarity"] = (N.MODEL_SIMILARITY, np.ascontiguousarray(np.concatenate([src, dst], 1).astype(np.float32)),
                            2.0)
    src, dst, _ = S.homography_problem(n, 1)
    scenes["homography"] = (N.MODEL_HOMOGRAPHY, np.ascontiguousarray(np.concatenate([src, dst], 1).astype(np.float32)),
                            5e-3)
    prev_staging = L.mcvTestHStaging(2, None)
    legs, keys = {}, {}
    for name, (model, pts, thr) in scenes.items():
        plan = D.RansacPlan(model, n, hyps)
        d_pts = torch.from_numpy(pts).to(dev)
        key = torch.zeros(2, dtype=torch.int64, device=dev)
        cfg = opencv.RansacParams(threshold=thr, max_iters=hyps, seed=7, fixed_iters=True).to_c()
        legs[name] = (lambda plan=plan, d_pts=d_pts, cfg=cfg, key=key: plan.evaluate(d_pts, n, cfg, 0, hyps, key))
        keys[name] = (plan, d_pts, key)
    for _ in range(a.warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in legs}
    for _ in range(a.reps):
        for name, fn in legs.items():          # alternating
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    # the sweep kernels alone: one profiled call at a time, legs alternating
    scope = {"affine": "a_verify", "similarity": "a_verify", "homography": "h_verify"}
    kms = {name: [] for name in legs}
    L.mcvProfileEnable(1)
    for _ in range(a.reps):
        for name, fn in legs.items():
            L.mcvProfileReset()
            fn()
            torch.cuda.synchronize()
            k, total = profile_read(scope[name])
            if k != 1:
                raise RuntimeError(f"{scope[name]}: {k} timed launches in one evaluate, expected 1")
            kms[name].append(total)
    L.mcvProfileEnable(0)
    L.mcvProfileReset()
    L.mcvTestHStaging(prev_staging, None)
    doc = {"bench": "affine", "device": torch.cuda.get_device_name(0), "n": n, "hyps": hyps, "reps": a.reps,
           "warmup": a.warmup, "sampler": "philox", "timing": "HIP events, one stream, legs alternating",
           "legs": {"affine": "mcvRansacEvaluate MCV_MODEL_AFFINE", "similarity": "mcvRansacEvaluate MCV_MODEL_SIMILARITY",
                    "homography": "mcvRansacEvaluate MCV_MODEL_HOMOGRAPHY, mcvTestHStaging(2) (unstaged certified sweep)"},
           "evaluate": {}, "sweep_kernel": {}, "best": {}}
    for name in legs:
        doc["evaluate"][name] = stats(ms[name])
        doc["sweep_kernel"][name] = dict(stats(kms[name]), scope=scope[name])
        c, h = D.unpack_key(int(keys[name][2].cpu()[0]))
        doc["best"][name] = {"count": int(c), "hypothesis": int(h)}
    hk = doc["sweep_kernel"]["homography"]["median_ms"]
    doc["a_verify_over_h_verify"] = {name: round(doc["sweep_kernel"][name]["median_ms"] / hk, 4)
                                     for name in ("affine", "similarity")}
    # LMedS selection kernel, once: the affine rank model beside the homography's on the same build
    rank = {}
    for name, width in (("affine", 6), ("homography", 8)):
        model, pts, _ = scenes[name]
        models = host_models(model, pts, a.rank_hyps, width)
        vals = np.zeros(a.rank_hyps, dtype=np.float32)

        def select():
            ok = L.mcvTestErrorRank(model, pts.ctypes.data, n, models.ctypes.data, a.rank_hyps, 0, n // 2,
                                    vals.ctypes.data)
            N.check(ok == 1, "mcvTestErrorRank")

        select()
        L.mcvProfileReset()
        L.mcvProfileEnable(1)
        for _ in range(3):
            select()
        k, total = profile_read("lmeds_select")
        L.mcvProfileEnable(0)
        L.mcvProfileReset()
        if k != 3:
            raise RuntimeError(f"lmeds_select: {k} timed launches, expected 3")
        rank[name] = round(total / 3, 4)
    doc["lmeds_select"] = {"n": n, "slots": a.rank_hyps, "error": "op by op", "mean_of": 3, "ms": rank,
                           "affine_over_homography": round(rank["affine"] / rank["homography"], 4)}
    print(json.dumps(doc), flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
