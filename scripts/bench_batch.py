#!/usr/bin/env python3
"""cvFindModelBatch against the loop of single calls it replaces: wall clock per model family.

One process, one MI355X. Per model (homography, fundamental, affine, similarity), N correspondences per
problem (--n, default 200 and 1000) and B problems (--b, default 1, 16, 256, 1024), every problem its
own scene: the wall clock of ONE cvFindModelBatch over the B problems against a Python loop of B calls of
the model's single export on the same data, both with the export's default configuration (cfg NULL:
RANSAC, threshold 3, 2000 iterations, OpenCV's sample stream). The two legs alternate; --warmup rounds
(default 2), then the median and p10 - p90 of --reps rounds (default 11; at least 10). Beside them: the
batch's kernel launches and stream synchronisations, its host share (point conversion, OpenCV sample
tables, from mcvTestBatchStats), and the same batch with the Philox sampler (no tables to draw).

--parent-lib PATH: the loop at B = 256 once more in a child process that loads another build of the
library (the parent commit's), as a check that the loop figure is the parent's own.
--loop-only: that child (prints one JSON line)."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from minicv_amd import synthetic as S  # noqa: E402

MODELS = {"homography": 0, "fundamental": 1, "affine": 4, "similarity": 5}
SINGLE = {"homography": "cvFindHomography", "fundamental": "cvFindFundamentalMat", "affine": "cvEstimateAffine2D",
          "similarity": "cvEstimateAffinePartial2D"}
PIXELS = 500.0   # the homography / fundamental scenes are in [-1, 1]: scaled to pixels for the threshold of 3


def scenes(name, n, B):
    out = []
    for k in range(B):
        seed = 1000 + k
        if name == "homography":
            src, dst, _ = S.homography_problem(n, seed, outlier_frac=0.4)
            src, dst = src * PIXELS, dst * PIXELS
        elif name == "fundamental":
            src, dst, _, _ = S.fundamental_problem(n, seed, outlier_frac=0.4)
            src, dst = src * PIXELS, dst * PIXELS
        else:
            src, dst, _, _ = S.affine_problem(n, seed, outlier_frac=0.4, similarity=name == "similarity")
        out.append((np.ascontiguousarray(src, dtype=np.float64), np.ascontiguousarray(dst, dtype=np.float64)))
    return out


def stats(v):
    v = np.sort(np.array(v)) * 1e3
    return {"median_ms": round(float(np.median(v)), 4), "p10_ms": round(float(v[int(0.1 * (len(v) - 1))]), 4),
            "p90_ms": round(float(v[int(np.ceil(0.9 * (len(v) - 1)))]), 4)}


def single_fn(lib, name):
    f = getattr(lib, SINGLE[name])
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return f


def make_loop(lib, name, probs):
    f = single_fn(lib, name)
    M = np.zeros(9)
    masks = [np.zeros(len(s), dtype=np.uint8) for s, _ in probs]
    args = [(s.ctypes.data, d.ctypes.data, len(s), None, M.ctypes.data, m.ctypes.data) for (s, d), m in zip(probs, masks)]

    def loop():
        ok = 0
        for a in args:
            ok += f(*a) > 0
        return ok
    loop.buffers = (probs, M, masks)   # args holds raw addresses: the arrays behind them must outlive make_loop
    return loop


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def loop_only(a):
    lib = C.CDLL(a.loop_only)
    name, n, B = a.model, a.n[0], a.b[0]
    loop = make_loop(lib, name, scenes(name, n, B))
    for _ in range(a.warmup):
        loop()
    ts = [timed(loop)[0] for _ in range(a.reps)]
    print(json.dumps(dict(stats(ts), model=name, n=n, B=B, lib=a.loop_only)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[200, 1000])
    ap.add_argument("--b", type=int, nargs="+", default=[1, 16, 256, 1024])
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--models", nargs="+", default=list(MODELS))
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--loop-only", default=None)
    ap.add_argument("--model", default="homography")
    ap.add_argument("--date", default=time.strftime("%Y-%m-%d"))
    ap.add_argument("--out", default=str(ROOT / "profiles" / "batch_bench.json"))
    a = ap.parse_args()
    if a.loop_only:
        return loop_only(a)
    from minicv_amd import native as N, opencv
    L = N.lib()
    if L.mcvDeviceCount() <= 0:
        raise SystemExit("bench_batch: no HIP device (this measurement has no CPU form)")
    import torch
    doc = {"bench": "batch", "device": torch.cuda.get_device_name(0), "date": a.date, "reps": a.reps,
           "warmup": a.warmup, "config": "cfg NULL (each export's defaults: RANSAC, threshold 3, 2000 iterations, "
           "OpenCV's sample stream)", "timing": "time.perf_counter around the call(s), legs alternating, one process",
           "cases": [], "parent_loop": []}
    st = np.zeros(16, dtype=np.int64)
    for name in a.models:
        model = MODELS[name]
        for n in a.n:
            allp = scenes(name, n, max(a.b))
            for B in a.b:
                probs = allp[:B]
                srcs, dsts = [s for s, _ in probs], [d for _, d in probs]
                offsets = np.zeros(B + 1, dtype=np.int32)
                offsets[1:] = np.cumsum([len(s) for s in srcs])
                pa, pb = np.ascontiguousarray(np.concatenate(srcs)), np.ascontiguousarray(np.concatenate(dsts))
                models, counts = np.zeros((B, 9)), np.zeros(B, dtype=np.int32)
                mask = np.zeros(int(offsets[-1]), dtype=np.uint8)
                philox = opencv.RansacParams(threshold=3.0, confidence=0.995 if name == "homography" else 0.99,
                                             max_iters=2000, seed=1).to_c()

                def batch(cfg=None):
                    return L.cvFindModelBatch(model, pa.ctypes.data, pb.ctypes.data, offsets.ctypes.data, B, cfg,
                                              models.ctypes.data, mask.ctypes.data, counts.ctypes.data)

                def batch_philox():
                    return batch(C.addressof(philox))

                loop = make_loop(L, name, probs)
                legs = {"batch": batch, "loop": loop, "batch_philox": batch_philox}
                ts = {k: [] for k in legs}
                host = {"batch": [], "batch_philox": []}
                info = {}
                for r in range(a.warmup + a.reps):
                    for k, fn in legs.items():          # alternating
                        t, ok = timed(fn)
                        if k != "loop":
                            L.mcvTestBatchStats(st.ctypes.data)
                            info[k] = dict(launches=int(st[0]), syncs=int(st[1]), rounds=int(st[2]),
                                           lm_rounds=int(st[3]), single_path=int(st[4]))
                        if r >= a.warmup:
                            ts[k].append(t)
                            if k != "loop":
                                host[k].append((int(st[6]) * 1e-6, int(st[7]) * 1e-6))
                        info.setdefault("ok", {})[k] = int(ok)
                case = {"model": name, "n": n, "B": B, "solved": info["ok"]}
                for k in legs:
                    case[k] = stats(ts[k])
                for k in host:
                    case[k].update(info[k])
                    case[k]["host_pack_ms"] = round(float(np.median([h[0] for h in host[k]])) * 1e3, 4)
                    case[k]["host_cv_tables_ms"] = round(float(np.median([h[1] for h in host[k]])) * 1e3, 4)
                case["loop_over_batch"] = round(case["loop"]["median_ms"] / case["batch"]["median_ms"], 3)
                case["loop_over_batch_philox"] = round(case["loop"]["median_ms"] / case["batch_philox"]["median_ms"], 3)
                doc["cases"].append(case)
                print(json.dumps(case), flush=True)
    if a.parent_lib:
        for name in a.models:
            cmd = [sys.executable, __file__, "--loop-only", a.parent_lib, "--model", name, "--n", "1000", "--b", "256",
                   "--reps", str(a.reps), "--warmup", str(a.warmup)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=300,
                               env=dict(os.environ, PYTHONPATH=str(ROOT)))
            if r.returncode != 0:
                doc["parent_loop"].append({"model": name, "error": r.stderr[-300:]})
                continue
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            rec["lib"] = "parent commit build"
            here = [c for c in doc["cases"] if c["model"] == name and c["n"] == 1000 and c["B"] == 256]
            if here:
                rec["this_build_loop_median_ms"] = here[0]["loop"]["median_ms"]
            doc["parent_loop"].append(rec)
            print(json.dumps(rec), flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
