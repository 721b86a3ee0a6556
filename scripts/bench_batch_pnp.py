#!/usr/bin/env python3
"""cvSolvePnPRansacBatch against the loop of single calls it replaces: wall clock.

One process, one MI355X. N correspondences per problem (--n, default 200 and 1000) and B problems (--b,
default 1, 16, 256, 1024), every problem its own scene (synthetic.pnp_problem, 50 % outliers, its own seed).
Per solver kind (EPNP, Iterative, AP3P) two legs, alternating: ONE cvSolvePnPRansacBatch against a Python loop
of B cvSolvePnPRansac calls on the same data, both at the reference's defaults (100 iterations, 8 px, 0.99,
OpenCV's sample stream). --warmup rounds (default 2), then the median and p10 - p90 of --reps rounds (default
11). Beside them: the batch's kernel launches, stream synchronisations and copies, its host share (staging the
points, OpenCV's sample tables, from mcvTestBatchStats) and, from one more profiled call, the device time of
its generate and its sweep.

--parent-lib PATH: the Iterative loop at B = 256, N = 1000 once more in a child process that loads another
build of the library (the parent commit's), as a check that the loop figure is the parent's own.
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

KINDS = {"EPNP": 1, "Iterative": 0, "AP3P": 5}
ITERS, THR, CONF = 100, 8.0, 0.99


class M33d(C.Structure):
    _fields_ = [("M", C.c_double * 9)]


def scenes(n, B):
    out = []
    for k in range(B):
        img, W, _, K, d, _, _ = S.pnp_problem(n, seed=3000 + k, outlier_frac=0.5)
        out.append((np.ascontiguousarray(img, dtype=np.float64), np.ascontiguousarray(W, dtype=np.float64),
                    np.ascontiguousarray(K, dtype=np.float64).reshape(9), np.ascontiguousarray(d, dtype=np.float64)))
    return out


def stats(v):
    v = np.sort(np.array(v)) * 1e3
    return {"median_ms": round(float(np.median(v)), 4), "p10_ms": round(float(v[int(0.1 * (len(v) - 1))]), 4),
            "p90_ms": round(float(v[int(np.ceil(0.9 * (len(v) - 1)))]), 4)}


def make_loop(lib, probs, kind):
    f = lib.cvSolvePnPRansac
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, M33d, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_double,
                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    t, r = np.zeros(3), np.zeros(3)
    cnt = np.zeros(1, dtype=np.int32)
    idx = [np.zeros(len(p[0]), dtype=np.int32) for p in probs]
    Ks = [M33d((C.c_double * 9)(*p[2])) for p in probs]
    args = [(p[0].ctypes.data, p[1].ctypes.data, len(p[0]), k, p[3].ctypes.data, kind, ITERS, THR, CONF,
             t.ctypes.data, r.ctypes.data, cnt.ctypes.data, i.ctypes.data) for p, k, i in zip(probs, Ks, idx)]

    def loop():
        ok = 0
        for x in args:
            ok += f(*x) != 0
        return ok
    loop.buffers = (probs, t, r, cnt, idx, Ks)   # args holds raw addresses: the arrays behind them must outlive it
    return loop


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def loop_only(a):
    lib = C.CDLL(a.loop_only)
    n, B = a.n[0], a.b[0]
    loop = make_loop(lib, scenes(n, B), KINDS["Iterative"])
    for _ in range(a.warmup):
        loop()
    ts = [timed(loop)[0] for _ in range(a.reps)]
    print(json.dumps(dict(stats(ts), n=n, B=B, kind="Iterative", lib=a.loop_only)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[200, 1000])
    ap.add_argument("--b", type=int, nargs="+", default=[1, 16, 256, 1024])
    ap.add_argument("--kinds", nargs="+", default=list(KINDS))
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--loop-only", default=None)
    ap.add_argument("--date", default=time.strftime("%Y-%m-%d"))
    ap.add_argument("--out", default=str(ROOT / "profiles" / "batch_pnp_bench.json"))
    a = ap.parse_args()
    if a.loop_only:
        return loop_only(a)
    from minicv_amd import native as N
    L = N.lib()
    if L.mcvDeviceCount() <= 0:
        raise SystemExit("bench_batch_pnp: no HIP device (this measurement has no CPU form)")
    import torch
    doc = {"bench": "batch_pnp", "device": torch.cuda.get_device_name(0), "date": a.date, "reps": a.reps,
           "warmup": a.warmup,
           "config": f"{ITERS} iterations, {THR} px, confidence {CONF}, OpenCV's sample stream (the reference's "
                     "defaults); scenes: pnp_problem, 50 % outliers, one seed per problem, no distortion",
           "timing": "time.perf_counter around the call(s), legs alternating, one process",
           "cases": [], "parent_loop": []}
    st = np.zeros(16, dtype=np.int64)
    for n in a.n:
        allp = scenes(n, max(a.b))
        for B in a.b:
            probs = allp[:B]
            offsets = np.zeros(B + 1, dtype=np.int32)
            offsets[1:] = np.cumsum([len(p[0]) for p in probs])
            img = np.ascontiguousarray(np.concatenate([p[0] for p in probs]))
            world = np.ascontiguousarray(np.concatenate([p[1] for p in probs]))
            Ks = np.ascontiguousarray(np.stack([p[2] for p in probs]))
            ds = np.ascontiguousarray(np.stack([p[3] for p in probs]))
            ts3, rs3 = np.zeros((B, 3)), np.zeros((B, 3))
            counts = np.zeros(B, dtype=np.int32)
            mask = np.zeros(int(offsets[-1]), dtype=np.uint8)
            for name in a.kinds:
                cfg = N.RansacConfig(THR, CONF, ITERS, N.METHOD_RANSAC, 0, 1, N.FLAG_CV_SAMPLER, 0, KINDS[name])

                def batch():
                    return L.cvSolvePnPRansacBatch(img.ctypes.data, world.ctypes.data, offsets.ctypes.data, B,
                                                   Ks.ctypes.data, ds.ctypes.data, C.addressof(cfg), ts3.ctypes.data,
                                                   rs3.ctypes.data, mask.ctypes.data, counts.ctypes.data)

                legs = {"batch": batch, "loop": make_loop(L, probs, KINDS[name])}
                ts = {k: [] for k in legs}
                host, info, solved = [], {}, {}
                for r in range(a.warmup + a.reps):
                    for k, fn in legs.items():          # alternating
                        dt, ok = timed(fn)
                        if k == "batch":
                            L.mcvTestBatchStats(st.ctypes.data)
                            info = dict(launches=int(st[0]), syncs=int(st[1]), rounds=int(st[2]), lm_rounds=int(st[3]),
                                        single_path=int(st[4]), copies=int(st[9]))
                        if r >= a.warmup:
                            ts[k].append(dt)
                            if k == "batch":
                                host.append((int(st[6]) * 1e-6, int(st[7]) * 1e-6))
                        solved[k] = int(ok)
                case = {"n": n, "B": B, "kind": name, "solved": solved}
                for k in legs:
                    case[k] = stats(ts[k])
                case["batch"].update(info)
                case["batch"]["host_stage_ms"] = round(float(np.median([h[0] for h in host])) * 1e3, 4)
                case["batch"]["host_cv_tables_ms"] = round(float(np.median([h[1] for h in host])) * 1e3, 4)
                # the device time of the generate and the sweep, from one more call with the event timers on
                L.mcvProfileReset()
                L.mcvProfileEnable(1)
                batch()
                L.mcvProfileEnable(0)
                for scope in ("batch_pnp_generate", "batch_pnp_sweep"):
                    ms = C.c_double(0)
                    nl = L.mcvProfileRead(scope.encode(), C.addressof(ms))
                    case["batch"][scope + "_ms"] = round(ms.value, 4) if nl > 0 else None
                L.mcvProfileReset()
                case["loop_over_batch"] = round(case["loop"]["median_ms"] / case["batch"]["median_ms"], 3)
                doc["cases"].append(case)
                print(json.dumps(case), flush=True)
    if a.parent_lib:
        cmd = [sys.executable, __file__, "--loop-only", a.parent_lib, "--n", "1000", "--b", "256", "--reps", str(a.reps),
               "--warmup", str(a.warmup)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, PYTHONPATH=str(ROOT)))
        if r.returncode != 0:
            doc["parent_loop"].append({"error": r.stderr[-300:]})
        else:
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            rec["lib"] = "parent commit build"
            here = [c for c in doc["cases"] if c["n"] == 1000 and c["B"] == 256 and c["kind"] == "Iterative"]
            if here:
                rec["this_build_loop_median_ms"] = here[0]["loop"]["median_ms"]
            doc["parent_loop"].append(rec)
            print(json.dumps(rec), flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
