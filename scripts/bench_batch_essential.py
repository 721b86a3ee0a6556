#!/usr/bin/env python3
"""cvRecoverPoseBatch / cvFindEssentialMatBatch against the loops of single calls they replace: wall clock.

One process, one MI355X. N correspondences per problem (--n, default 200 and 1000) and B problems (--b,
default 1, 16, 256, 1024), every problem its own scene (synthetic.essential_problem, 40 % outliers, its own
seed). Two pairs of legs, all four alternating:
  pose:   ONE cvRecoverPoseBatch against a Python loop of B cvRecoverPose calls on the same data, with the
          default RecoverPoseConfig (probability 0.999, threshold 0.005) scaled to pixels (focal 800);
  philox: ONE cvFindEssentialMatBatch with the Philox sampler against a loop of B cvFindEssentialMat calls
          with the same configuration (threshold 4 px, confidence 0.999, 1000 iterations, seed 1).
--warmup rounds (default 2), then the median and p10 - p90 of --reps rounds (default 11). Beside them: the
batch's kernel launches and stream synchronisations, its host share (staging the points, OpenCV's sample
tables, from mcvTestBatchStats) and, from one more profiled call, the device time of its generate and its sweep.

--parent-lib PATH: the cvRecoverPose loop at B = 256, N = 1000 once more in a child process that loads
another build of the library (the parent commit's), as a check that the loop figure is the parent's own.
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

FOCAL, PP = 800.0, (640.0, 360.0)
PROB, THR = 0.999, 0.005 * FOCAL   # RecoverPoseConfig.Default, the threshold scaled to pixels


class V2d(C.Structure):
    _fields_ = [("X", C.c_double), ("Y", C.c_double)]


class RecoverPoseConfig(C.Structure):
    _fields_ = [("FocalLength", C.c_double), ("PrincipalPoint", V2d), ("Probability", C.c_double),
                ("InlierThreshold", C.c_double)]


def scenes(n, B):
    out = []
    for k in range(B):
        a, b, *_ = S.essential_problem(n, seed=2000 + k, outlier_frac=0.4, focal=FOCAL, pp=PP)
        out.append((np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)))
    return out


def stats(v):
    v = np.sort(np.array(v)) * 1e3
    return {"median_ms": round(float(np.median(v)), 4), "p10_ms": round(float(v[int(0.1 * (len(v) - 1))]), 4),
            "p90_ms": round(float(v[int(np.ceil(0.9 * (len(v) - 1)))]), 4)}


def make_pose_loop(lib, probs):
    f = lib.cvRecoverPose
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    cfg = RecoverPoseConfig(FOCAL, V2d(*PP), PROB, THR)
    R, t = np.zeros(9), np.zeros(3)
    masks = [np.zeros(len(a), dtype=np.uint8) for a, _ in probs]
    args = [(C.addressof(cfg), len(a), a.ctypes.data, b.ctypes.data, R.ctypes.data, t.ctypes.data, m.ctypes.data)
            for (a, b), m in zip(probs, masks)]

    def loop():
        ok = 0
        for x in args:
            ok += f(*x) > 0
        return ok
    loop.buffers = (probs, cfg, R, t, masks)   # args holds raw addresses: the arrays behind them must outlive it
    return loop


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def loop_only(a):
    lib = C.CDLL(a.loop_only)
    n, B = a.n[0], a.b[0]
    loop = make_pose_loop(lib, scenes(n, B))
    for _ in range(a.warmup):
        loop()
    ts = [timed(loop)[0] for _ in range(a.reps)]
    print(json.dumps(dict(stats(ts), n=n, B=B, lib=a.loop_only)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[200, 1000])
    ap.add_argument("--b", type=int, nargs="+", default=[1, 16, 256, 1024])
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--loop-only", default=None)
    ap.add_argument("--date", default=time.strftime("%Y-%m-%d"))
    ap.add_argument("--out", default=str(ROOT / "profiles" / "batch_essential_bench.json"))
    a = ap.parse_args()
    if a.loop_only:
        return loop_only(a)
    from minicv_amd import native as N, opencv
    L = N.lib()
    if L.mcvDeviceCount() <= 0:
        raise SystemExit("bench_batch_essential: no HIP device (this measurement has no CPU form)")
    import torch
    doc = {"bench": "batch_essential", "device": torch.cuda.get_device_name(0), "date": a.date, "reps": a.reps,
           "warmup": a.warmup,
           "config": f"pose legs: RecoverPoseConfig(focal {FOCAL}, pp {PP}, probability {PROB}, threshold {THR} px), "
                     "OpenCV's sample stream, 1000 iterations; philox legs: the same threshold and confidence, "
                     "1000 iterations, Philox seed 1; scenes: essential_problem, 40 % outliers, one seed per problem",
           "timing": "time.perf_counter around the call(s), legs alternating, one process",
           "cases": [], "parent_loop": []}
    st = np.zeros(16, dtype=np.int64)
    philox = opencv.RansacParams(threshold=THR, confidence=PROB, max_iters=1000, seed=1).to_c()
    for n in a.n:
        allp = scenes(n, max(a.b))
        for B in a.b:
            probs = allp[:B]
            offsets = np.zeros(B + 1, dtype=np.int32)
            offsets[1:] = np.cumsum([len(x) for x, _ in probs])
            pa = np.ascontiguousarray(np.concatenate([x for x, _ in probs]))
            pb = np.ascontiguousarray(np.concatenate([y for _, y in probs]))
            cfgs = (N.RecoverPoseConfig * B)(*[N.RecoverPoseConfig(FOCAL, N.V2d(*PP), PROB, THR) for _ in range(B)])
            focal = np.full(B, FOCAL)
            pps = np.tile(np.array(PP, dtype=np.float64), (B, 1))
            M, t3 = np.zeros((B, 9)), np.zeros((B, 3))
            counts = np.zeros(B, dtype=np.int32)
            mask = np.zeros(int(offsets[-1]), dtype=np.uint8)

            def pose_batch():
                return L.cvRecoverPoseBatch(C.addressof(cfgs), pa.ctypes.data, pb.ctypes.data, offsets.ctypes.data, B,
                                            M.ctypes.data, t3.ctypes.data, mask.ctypes.data, counts.ctypes.data)

            def find_batch():
                return L.cvFindEssentialMatBatch(pa.ctypes.data, pb.ctypes.data, offsets.ctypes.data, B,
                                                 focal.ctypes.data, pps.ctypes.data, C.addressof(philox),
                                                 M.ctypes.data, mask.ctypes.data, counts.ctypes.data)

            E1 = N.M33d()
            masks = [np.zeros(len(x), dtype=np.uint8) for x, _ in probs]

            def find_loop():
                ok = 0
                for (x, y), m in zip(probs, masks):
                    ok += L.cvFindEssentialMat(x.ctypes.data, y.ctypes.data, len(x), FOCAL, N.V2d(*PP),
                                               C.addressof(philox), C.addressof(E1), m.ctypes.data) > 0
                return ok

            legs = {"pose_batch": pose_batch, "pose_loop": make_pose_loop(L, probs), "philox_batch": find_batch,
                    "philox_loop": find_loop}
            ts = {k: [] for k in legs}
            host = {"pose_batch": [], "philox_batch": []}
            info = {}
            for r in range(a.warmup + a.reps):
                for k, fn in legs.items():          # alternating
                    dt, ok = timed(fn)
                    if k in host:
                        L.mcvTestBatchStats(st.ctypes.data)
                        info[k] = dict(launches=int(st[0]), syncs=int(st[1]), rounds=int(st[2]),
                                       single_path=int(st[4]), problem_rounds=int(st[8]))
                    if r >= a.warmup:
                        ts[k].append(dt)
                        if k in host:
                            host[k].append((int(st[6]) * 1e-6, int(st[7]) * 1e-6))
                    info.setdefault("ok", {})[k] = int(ok)
            case = {"n": n, "B": B, "solved": info["ok"]}
            for k in legs:
                case[k] = stats(ts[k])
            for k in host:
                case[k].update(info[k])
                case[k]["host_stage_ms"] = round(float(np.median([h[0] for h in host[k]])) * 1e3, 4)
                case[k]["host_cv_tables_ms"] = round(float(np.median([h[1] for h in host[k]])) * 1e3, 4)
                # the device time of the generate and the sweep, from one more call with the event timers on
                L.mcvProfileReset()
                L.mcvProfileEnable(1)
                legs[k]()
                L.mcvProfileEnable(0)
                for scope in ("batch_e_generate", "batch_e_sweep"):
                    ms = C.c_double(0)
                    nl = L.mcvProfileRead(scope.encode(), C.addressof(ms))
                    case[k][scope + "_ms"] = round(ms.value, 4) if nl > 0 else None
                L.mcvProfileReset()
            case["pose_loop_over_batch"] = round(case["pose_loop"]["median_ms"] / case["pose_batch"]["median_ms"], 3)
            case["philox_loop_over_batch"] = round(case["philox_loop"]["median_ms"] /
                                                   case["philox_batch"]["median_ms"], 3)
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
            here = [c for c in doc["cases"] if c["n"] == 1000 and c["B"] == 256]
            if here:
                rec["this_build_loop_median_ms"] = here[0]["pose_loop"]["median_ms"]
            doc["parent_loop"].append(rec)
            print(json.dumps(rec), flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
