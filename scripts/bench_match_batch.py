#!/usr/bin/env python3
"""cvMatchFeaturesBatch against the loop of cvMatchFeaturesNorm calls it replaces: wall clock.

One process, one MI355X. 64 images of --features (default 500, 2000, 8000) features each; every image is a
noisy copy of one base set with 40 % of its rows replaced by random ones, so any two images share about a
third of their features. B pairs (--b, default 1, 16, 256) are drawn from the 64 images with a fixed seed.
Descriptors: 32-byte ORB-like rows under Hamming, then 128-byte SIFT-like rows under L2; ratio 0.8, with and
without the cross-check. Both legs see the same DetectorResults and write into preallocated arrays:
  batch: ONE cvMatchFeaturesBatch
  loop:  B cvMatchFeaturesNorm calls (the code path of the commit before the batch: it is not touched)
Every leg ends synchronised (the exports return after their last stream synchronisation). --warmup rounds
(default 2), then --reps (default 11) rounds of the two legs alternating; median and p10 - p90 per leg, the
ratio loop / batch of the medians, the batch's launches / synchronisations / copies from
mcvTestMatchBatchStats, and a check that both legs return the same pairs and the same dist bits.
Writes profiles/match_batch_bench.json (--out)."""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from minicv_amd import native as N  # noqa: E402

N_IMAGES = 64
KP = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
               ("octave", "<i4"), ("class_id", "<i4")])


def images(n, kind, seed):
    """-> (DetectorResult array, the numpy arrays behind it)."""
    rng = np.random.default_rng(seed)
    dim = 32 if kind == "hamming" else 128
    base = rng.integers(0, 256, size=(n, dim), dtype=np.uint8)
    keep = []
    structs = (N.DetectorResult * N_IMAGES)()
    for k in range(N_IMAGES):
        if kind == "hamming":
            flips = (rng.random((n, dim, 8)) < 0.04)      # ~10 of 256 bits
            d = base ^ np.packbits(flips, axis=2)[:, :, 0]
        else:
            d = np.clip(base.astype(np.int16) + rng.normal(0, 6, size=(n, dim)).round().astype(np.int16), 0, 255)
            d = d.astype(np.uint8)
        other = rng.random(n) < 0.4
        d[other] = rng.integers(0, 256, size=(int(other.sum()), dim), dtype=np.uint8)
        d = np.ascontiguousarray(d[rng.permutation(n)])
        kp = np.zeros(n, dtype=KP)
        kp["x"], kp["y"] = rng.uniform(0, 1280, n), rng.uniform(0, 720, n)
        keep += [d, kp]
        structs[k] = N.DetectorResult(n, int(d.size), 0, kp.ctypes.data, d.ctypes.data)
    return structs, keep


def stats(v):
    v = np.sort(np.array(v)) * 1e3
    return {"median_ms": round(float(np.median(v)), 4), "p10_ms": round(float(v[int(0.1 * (len(v) - 1))]), 4),
            "p90_ms": round(float(v[int(np.ceil(0.9 * (len(v) - 1)))]), 4)}


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--features", type=int, nargs="+", default=[500, 2000, 8000])
    ap.add_argument("--b", type=int, nargs="+", default=[1, 16, 256])
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "match_batch_bench.json"))
    args = ap.parse_args()
    L = N.lib()
    if L.mcvDeviceCount() <= 0:
        raise SystemExit("bench_match_batch: no HIP device visible (there is no CPU path to time)")
    rows = []
    for kind, norm in (("hamming", N.NORM_HAMMING), ("sift_u8", N.NORM_L2)):
        for n in args.features:
            structs, keep = images(n, kind, seed=n)
            base = C.addressof(structs)
            step = C.sizeof(N.DetectorResult)
            for B in args.b:
                ip = np.random.default_rng(B).integers(0, N_IMAGES, size=(B, 2)).astype(np.int32)
                cap = B * n
                for cross in (0, 1):
                    cfg = N.MatchConfig(0.8, cross, 0.0, N.MODEL_HOMOGRAPHY)
                    bp, bd = np.zeros((cap, 2), np.int32), np.zeros(cap, np.float32)
                    lp, ld = np.zeros((cap, 2), np.int32), np.zeros(cap, np.float32)
                    boff, loff = np.zeros(B + 1, np.int32), np.zeros(B + 1, np.int32)

                    def batch():
                        return L.cvMatchFeaturesBatch(base, N_IMAGES, ip.ctypes.data, B, C.addressof(cfg), norm,
                                                      bp.ctypes.data, bd.ctypes.data, cap, boff.ctypes.data)

                    def loop():
                        o = 0
                        for p in range(B):
                            k = L.cvMatchFeaturesNorm(base + int(ip[p, 0]) * step, base + int(ip[p, 1]) * step,
                                                      C.addressof(cfg), norm, lp.ctypes.data + 8 * o,
                                                      ld.ctypes.data + 4 * o, cap - o)
                            if k < 0:
                                return -1
                            o += k
                            loff[p + 1] = o
                        return o

                    tb, tl = [], []
                    for r in range(args.warmup + args.reps):
                        (a, ka), (b, kb) = timed(batch), timed(loop)
                        if ka < 0 or kb < 0:
                            raise SystemExit(f"bench_match_batch: a leg failed: {N.last_error()}")
                        if r >= args.warmup:
                            tb.append(a)
                            tl.append(b)
                    st = np.zeros(8, dtype=np.int64)
                    batch()
                    L.mcvTestMatchBatchStats(st.ctypes.data)
                    same = bool(ka == kb and np.array_equal(boff, loff) and np.array_equal(bp[:ka], lp[:kb]) and
                                np.array_equal(bd[:ka].view(np.uint32), ld[:kb].view(np.uint32)))
                    sb, sl = stats(tb), stats(tl)
                    row = {"norm": "hamming" if kind == "hamming" else "l2_u8", "bytes": 32 if kind == "hamming" else 128,
                           "features": n, "B": B, "cross_check": bool(cross), "matches": int(ka), "same_output": same,
                           "batch": sb, "loop": sl, "loop_over_batch": round(sl["median_ms"] / sb["median_ms"], 3),
                           "launches": int(st[0]), "syncs": int(st[1]), "directed_problems": int(st[2]),
                           "workgroups": int(st[3]), "copies": int(st[4])}
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                    if not same:
                        raise SystemExit("bench_match_batch: the two legs disagree")
    out = {"device": "MI355X", "images": N_IMAGES, "reps": args.reps, "warmup": args.warmup, "ratio": 0.8,
           "rows": rows}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
