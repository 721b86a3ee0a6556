#!/usr/bin/env python
"""cvRefinePnPBatch / cvSolvePnPRansacRefineBatch against what a caller had before them
-> profiles/batch_pnp_refine_bench.json.

Host arrays in, host arrays out, wall clock around the call(s), legs alternating in one process, --warmup
untimed rounds, then the median and p10 / p90 of --reps. Every leg's poses are compared bit for bit with the
loop's before anything is timed.

Cases (--cases picks some; the records of the others stay in the output file):
  refine  B = 256 cameras at 200 and at 1000 selected points (a mask selects them from 1.5 x as many rows), LM
          and VVS: cvRefinePnPBatch against the loop of cvRefinePnPLM / cvRefinePnPVVS on arrays gathered
          beforehand (the gather is not timed: it favours the loop)
  b1      B = 1 through the batch against the single call (recorded, no requirement)
  fused   cvSolvePnPRansacRefineBatch against cvSolvePnPRansacBatch + cvRefinePnPBatch, kind EPNP, the
          reference's defaults (100 iterations, 8 px, 0.99, OpenCV's sample stream), B = 256
Acceptance (refine): the batch's p90 below the loop's p10 on every leg; the script exits 1 otherwise.

Run each case under its own time limit, chained:
  timeout 300 python scripts/bench_batch_pnp_refine.py --cases refine && \\
  timeout 120 python scripts/bench_batch_pnp_refine.py --cases b1 && \\
  timeout 300 python scripts/bench_batch_pnp_refine.py --cases fused"""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from minicv_amd import synthetic as S  # noqa: E402

REFINE = {"LM": 0, "VVS": 1}
ITERS, THR, CONF = 100, 8.0, 0.99


def rvec_of(R):
    ang = np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return w / (2 * np.sin(ang)) * ang


def stats(v):
    v = np.sort(np.array(v)) * 1e3
    return {"median_ms": round(float(np.median(v)), 4), "p10_ms": round(float(v[int(0.1 * (len(v) - 1))]), 4),
            "p90_ms": round(float(v[int(np.ceil(0.9 * (len(v) - 1)))]), 4)}


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


class Batch:
    """B problems as the segmented arrays of the batch exports, plus each problem's gathered arrays."""

    def __init__(self, n_sel, B, outliers=0.0):
        rng = np.random.default_rng(n_sel + B)
        rows = n_sel * 3 // 2 if outliers == 0 else n_sel
        imgs, worlds, masks, self.gathered, r0, t0, Ks = [], [], [], [], [], [], []
        for k in range(B):
            img, W, _, K, _, R, t = S.pnp_problem(rows, seed=5000 + k, outlier_frac=outliers, sigma=0.3)
            m = np.zeros(rows, dtype=np.uint8)
            m[np.sort(rng.choice(rows, n_sel, replace=False))] = 1
            imgs.append(img)
            worlds.append(W)
            masks.append(m)
            sel = np.flatnonzero(m)
            self.gathered.append((np.ascontiguousarray(img[sel]), np.ascontiguousarray(W[sel])))
            r0.append(rvec_of(S.rotation([1, 0, 0], 0.05) @ R))
            t0.append(t + np.array([0.05, -0.03, 0.2]))
            Ks.append(np.asarray(K, dtype=np.float64).reshape(9))
        self.B = B
        self.offsets = np.zeros(B + 1, dtype=np.int32)
        self.offsets[1:] = np.cumsum([len(x) for x in imgs])
        self.img = np.ascontiguousarray(np.concatenate(imgs))
        self.world = np.ascontiguousarray(np.concatenate(worlds))
        self.mask = np.ascontiguousarray(np.concatenate(masks))
        self.K = np.ascontiguousarray(np.stack(Ks))
        self.dist = np.zeros((B, 4))
        self.r0, self.t0 = np.ascontiguousarray(r0), np.ascontiguousarray(t0)


def refine_legs(N, L, b, kind):
    """-> (batch leg, loop leg); each returns (rvecs, tvecs)."""
    fn = L.cvRefinePnPVVS if kind else L.cvRefinePnPLM
    Ks = []
    for k in range(b.B):
        m = N.M33d()
        m.M[:] = b.K[k].tolist()
        Ks.append(m)
    r, t = np.zeros((b.B, 3)), np.zeros((b.B, 3))
    lr, lt = np.zeros((b.B, 3)), np.zeros((b.B, 3))

    def batch():
        r[:], t[:] = b.r0, b.t0
        k = L.cvRefinePnPBatch(b.img.ctypes.data, b.world.ctypes.data, b.offsets.ctypes.data, b.B, b.K.ctypes.data,
                               b.dist.ctypes.data, b.mask.ctypes.data, kind, t.ctypes.data, r.ctypes.data, None)
        assert k == b.B, N.last_error()
        return r, t

    def loop():
        lr[:], lt[:] = b.r0, b.t0
        for k in range(b.B):
            gi, gw = b.gathered[k]
            fn(gi.ctypes.data, gw.ctypes.data, len(gi), Ks[k], b.dist[k].ctypes.data, lt[k].ctypes.data,
               lr[k].ctypes.data)
        return lr, lt
    return batch, loop


def run_legs(legs, a, after=None):
    ts = {k: [] for k in legs}
    info = {}
    for rep in range(a.warmup + a.reps):
        for k, fn in legs.items():   # alternating
            dt, _ = timed(fn)
            if after and k in after:
                info[k] = after[k]()
            if rep >= a.warmup:
                ts[k].append(dt)
    out = {k: stats(v) for k, v in ts.items()}
    for k, v in info.items():
        out[k].update(v)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["refine", "b1", "fused"], choices=["refine", "b1", "fused"])
    ap.add_argument("--n", type=int, nargs="+", default=[200, 1000])
    ap.add_argument("--b", type=int, default=256)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--date", default=time.strftime("%Y-%m-%d"))
    ap.add_argument("--out", default=str(ROOT / "profiles" / "batch_pnp_refine_bench.json"))
    a = ap.parse_args()
    from minicv_amd import native as N
    L = N.lib()
    if L.mcvDeviceCount() <= 0:
        raise SystemExit("bench_batch_pnp_refine: no HIP device (this measurement has no CPU form)")
    import torch
    out = Path(a.out)
    doc = json.loads(out.read_text()) if out.exists() else {}
    doc.update({"bench": "batch_pnp_refine", "device": torch.cuda.get_device_name(0), "date": a.date, "reps": a.reps,
                "warmup": a.warmup,
                "scenes": "pnp_problem, sigma 0.3 px, no distortion, one seed per problem; refine / b1: no outliers, "
                          "a mask selecting n of 1.5 n rows, start = the truth rotated 0.05 rad and moved "
                          "(0.05, -0.03, 0.2); fused: 50 % outliers, n rows",
                "timing": "time.perf_counter around the call(s), legs alternating, one process; every leg's poses "
                          "bit-equal to the loop's before timing"})
    st = np.zeros(16, dtype=np.int64)

    def batch_stats():
        L.mcvTestBatchStats(st.ctypes.data)
        return dict(launches=int(st[0]), syncs=int(st[1]), steps=int(st[3]), copies=int(st[9]))

    accepted = True
    for case in a.cases:
        recs = []
        if case in ("refine", "b1"):
            B = a.b if case == "refine" else 1
            for n in a.n:
                b = Batch(n, B)
                for name, kind in REFINE.items():
                    batch, loop = refine_legs(N, L, b, kind)
                    (r, t), (lr, lt) = batch(), loop()
                    assert np.array_equal(bits(r), bits(lr)) and np.array_equal(bits(t), bits(lt)), (case, n, name)
                    rec = {"selected": n, "B": B, "refine": name}
                    rec.update(run_legs({"batch": batch, "loop": loop}, a, {"batch": batch_stats}))
                    rec["loop_over_batch"] = round(rec["loop"]["median_ms"] / rec["batch"]["median_ms"], 3)
                    rec["batch_ms_per_step"] = round(rec["batch"]["median_ms"] / max(rec["batch"]["steps"], 1), 4)
                    if case == "refine":
                        rec["batch_p90_below_loop_p10"] = bool(rec["batch"]["p90_ms"] < rec["loop"]["p10_ms"])
                        accepted = accepted and rec["batch_p90_below_loop_p10"]
                    recs.append(rec)
                    print(json.dumps(rec), flush=True)
        else:
            B = a.b
            for n in a.n:
                b = Batch(n, B, outliers=0.5)
                cfg = N.RansacConfig(THR, CONF, ITERS, N.METHOD_RANSAC, 0, 1, N.FLAG_CV_SAMPLER, 0, 1)   # EPNP
                for name, kind in REFINE.items():
                    o = {k: (np.zeros((B, 3)), np.zeros((B, 3)), np.zeros(len(b.mask), np.uint8),
                             np.zeros(B, np.int32)) for k in ("fused", "two_calls")}

                    def fused():
                        t, r, m, c = o["fused"]
                        k = L.cvSolvePnPRansacRefineBatch(b.img.ctypes.data, b.world.ctypes.data,
                                                          b.offsets.ctypes.data, B, b.K.ctypes.data,
                                                          b.dist.ctypes.data, C.addressof(cfg), kind, t.ctypes.data,
                                                          r.ctypes.data, m.ctypes.data, c.ctypes.data)
                        assert k >= 0, N.last_error()
                        return k

                    def two_calls():
                        t, r, m, c = o["two_calls"]
                        k = L.cvSolvePnPRansacBatch(b.img.ctypes.data, b.world.ctypes.data, b.offsets.ctypes.data, B,
                                                    b.K.ctypes.data, b.dist.ctypes.data, C.addressof(cfg),
                                                    t.ctypes.data, r.ctypes.data, m.ctypes.data, c.ctypes.data)
                        assert k >= 0, N.last_error()
                        k2 = L.cvRefinePnPBatch(b.img.ctypes.data, b.world.ctypes.data, b.offsets.ctypes.data, B,
                                                b.K.ctypes.data, b.dist.ctypes.data, m.ctypes.data, kind,
                                                t.ctypes.data, r.ctypes.data, None)
                        assert k2 == k, N.last_error()
                        return k

                    solved = fused()
                    assert solved == two_calls()
                    for x, y in zip(o["fused"], o["two_calls"]):
                        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), ("fused", n, name)
                    rec = {"n": n, "B": B, "kind": "EPNP", "refine": name, "solved": int(solved)}
                    rec.update(run_legs({"fused": fused, "two_calls": two_calls}, a, {"fused": batch_stats}))
                    rec["two_calls_over_fused"] = round(rec["two_calls"]["median_ms"] / rec["fused"]["median_ms"], 3)
                    recs.append(rec)
                    print(json.dumps(rec), flush=True)
        doc[case] = recs
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(doc, indent=1) + "\n")
    if not accepted:
        raise SystemExit("bench_batch_pnp_refine: a batch leg's p90 is not below its loop's p10")


if __name__ == "__main__":
    main()
