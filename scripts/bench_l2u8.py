#!/usr/bin/env python3
"""Call time of the uint8 L2 matcher (mcvMatchL2U8Device, match_l2u8.hip) against the way the job was
done before it: the same bytes widened to float32 and matched by mcvMatchL2Device (f16-split GEMM,
fp64 re-rank, exact scan). One process, device-resident inputs (the widening is done once, outside
the timed window: it is not counted against the float leg), HIP events around each call on one
stream, a warm-up of both legs at every size, then --reps calls per leg with the two legs
alternating. Reports each leg's median and spread and the ratio of the medians, checks that both
legs return the same answer at the sizes it times, and writes one JSON document (--out)."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from minicv_amd import device as D, native as N, synthetic as S  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="50000x50000x128,10000x10000x128", help="nq x nt x dim, comma separated")
    ap.add_argument("--reps", type=int, default=20, help="timed calls per leg (>= 20 for the recorded figures)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "l2u8_bench.json"))
    a = ap.parse_args()
    if N.lib().mcvDeviceCount() <= 0:
        raise SystemExit("bench_l2u8: no HIP device (this measurement has no CPU form)")
    import torch
    dev = torch.device("cuda:0")
    results = []
    for size in a.sizes.split(","):
        nq, nt, dim = map(int, size.split("x"))
        q, t, _ = S.sift_u8_problem(nq, nt, dim=dim, seed=5)
        q8, t8 = torch.from_numpy(q).to(dev), torch.from_numpy(t).to(dev)
        qf, tf = q8.to(torch.float32).contiguous(), t8.to(torch.float32).contiguous()
        outs = {leg: (torch.empty(nq, dtype=torch.int32, device=dev), torch.empty(nq, dtype=torch.float32, device=dev),
                      torch.empty(nq, dtype=torch.int32, device=dev), torch.empty(nq, dtype=torch.float32, device=dev))
                for leg in ("u8", "f32")}
        legs = {"u8": lambda: D.match_l2_u8(q8, t8, *outs["u8"]), "f32": lambda: D.match_l2(qf, tf, *outs["f32"])}
        for _ in range(a.warmup):
            for fn in legs.values():
                fn()
        torch.cuda.synchronize()
        same = all(torch.equal(x, y) for x, y in zip(outs["u8"], outs["f32"]))
        ms = {leg: [] for leg in legs}
        for _ in range(a.reps):
            for leg, fn in legs.items():          # alternating
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ms[leg].append(e0.elapsed_time(e1))
        r = {"nq": nq, "nt": nt, "dim": dim, "reps": a.reps, "outputs_equal": bool(same),
             "exact_scan_queries_f32": int(N.lib().mcvL2LastExactScans())}
        for leg, v in ms.items():
            v = np.sort(np.array(v))
            r[leg] = {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(v[0]), 4),
                      "p10_ms": round(float(v[int(0.1 * (len(v) - 1))]), 4),
                      "p90_ms": round(float(v[int(np.ceil(0.9 * (len(v) - 1)))]), 4), "max_ms": round(float(v[-1]), 4)}
        r["u8_over_f32"] = round(r["u8"]["median_ms"] / r["f32"]["median_ms"], 4)
        # the int8 GEMM's operations (2 nq nt K, K = the padded dim) over the u8 call's median time
        kp = 32 if dim <= 32 else 64 if dim <= 64 else 128 if dim <= 128 else 256 if dim <= 256 else 512
        r["u8_gemm_tops_over_call_time"] = round(2.0 * nq * nt * kp / (r["u8"]["median_ms"] * 1e-3) / 1e12, 2)
        print(json.dumps(r), flush=True)
        results.append(r)
    doc = {"bench": "l2u8", "device": torch.cuda.get_device_name(0), "legs": {
        "u8": "mcvMatchL2U8Device on uint8 rows", "f32": "mcvMatchL2Device on the same rows widened to float32"},
        "timing": "HIP events around each call, one stream, legs alternating", "results": results}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
