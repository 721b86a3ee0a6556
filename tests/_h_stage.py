"""Shared helpers of the staged homography sweep's newer GPU tests (test_gpu_h_cell_pre.py,
test_gpu_h_stage0_subset.py): problems, oracle keys, and one key-only evaluate under the test hooks."""
import ctypes as C
import functools

import numpy as np

import _h_cell as HC
import _oracle
from minicv_amd import native as N, opencv, synthetic as S

THR = 5e-3
THR2 = float(np.float32(THR * THR))
NO_FAIL = 2**63 - 1
PRUNED, NO_CANDIDATE, SAMPLER_FAILURE, LATE = 0, 1, 2, 3
ON, OFF = 1, 2


@functools.lru_cache(maxsize=None)
def problem(n, seed, share=0.5, sigma=1e-3):
    src, dst, _ = S.homography_problem(n, seed, outlier_frac=share, sigma=sigma)
    return src, dst


@functools.lru_cache(maxsize=None)
def models_of(n, seed, count):
    src, dst = problem(n, seed)
    return HC.oracle_models(_oracle, _oracle.pack4(src, dst), seed, count)


def oracle_key(src, dst, seed, begin, count, thr):
    """-> ([best key before the first sampler failure, that failure], the oracle's counts)."""
    ref = _oracle.h_counts(_oracle.pack4(src, dst), seed, begin, count, float(np.float32(thr * thr)))
    fail = np.nonzero(ref == -2)[0]
    lim = fail[0] if len(fail) else count
    k0 = 0
    if (ref[:lim] >= 4).any():
        c = ref[:lim].max()
        i = int(np.nonzero(ref[:lim] == c)[0][0])
        k0 = (int(c) << 32) | (0xFFFFFFFF - (begin + i))
    return [k0, begin + int(fail[0]) if len(fail) else NO_FAIL], ref


def pack(src, dst):
    import torch
    from minicv_amd import device as D
    return D.pack_points_tensor(src, dst, torch.device("cuda:0"))


def evaluate(pts, n, seed, begin, count, thr, staging, cell, plan=None, stage0=0, counts=False):
    """One mcvRansacEvaluate (key-only unless counts) under the hooks' settings, which are restored.
    -> (key words, staging stats (16), cell stats (6), the counts or None)."""
    import torch
    from minicv_amd import device as D
    L = N.lib()
    own = plan is None
    if own:
        plan = D.RansacPlan(N.MODEL_HOMOGRAPHY, n, count)
    cfg = opencv.RansacParams(threshold=thr, seed=seed, fixed_iters=True, max_iters=max(count, 1)).to_c()
    key = torch.zeros(2, dtype=torch.int64, device=pts.device)
    cnt = torch.zeros(count, dtype=torch.int32, device=pts.device) if counts else None
    ps, pc, p0 = L.mcvTestHStaging(staging, None), L.mcvTestHCellMode(cell, 0, 0, None), L.mcvTestHStage0Slots(stage0)
    try:
        plan.evaluate(pts, n, cfg, begin, count, key, cnt)
        torch.cuda.synchronize()
        st, cs = (C.c_longlong * 16)(), (C.c_longlong * 6)()
        L.mcvTestHStaging(-1, C.addressof(st))
        L.mcvTestHCellMode(-1, 0, 0, C.addressof(cs))
    finally:
        L.mcvTestHStaging(ps, None)
        L.mcvTestHCellMode(pc, 0, 0, None)
        L.mcvTestHStage0Slots(p0)
        if own:
            plan.close()
    return ([int(v) for v in key.cpu().numpy()], [int(v) for v in st], [int(v) for v in cs],
            cnt.cpu().numpy() if counts else None)
