"""Back-to-back step time of the three ways to get per-trait peaks + LOD > 5 triplets at the BXD shape (BASELINE.json configs[1]:
n = 79, p = 7321, m = 35554, null-exact), each after a warm-up, `steps` calls enqueued one after the other and ONE final
synchronisation:
  store       bulkscan_dev: the p x m matrix written to HBM (bench.py's step);
  sync        bulkscan_reduced_dev: reduce in the scan epilogues, every call synchronises (and re-runs through a resident matrix
              when a trait is flagged);
  async       bulkscan_reduced_async: the same reduction, stream-ordered, flagged traits re-scanned on the device.
Then once more with lr_tol = 0 (every trait flagged by the weight-basis guard).  Prints one JSON line (profiles/)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bulklmm_jl_amd as B  # noqa: E402


def synth(n, p, m, seed):
    from common import make_data          # bench.py's data: the BXD kinship at n = 79
    Y, G, K, _ = make_data(n=n, p=p, m=m, seed=seed, bxd=(n == 79))
    return Y, G, K


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=79)
    ap.add_argument("--p", type=int, default=7321)
    ap.add_argument("--m", type=int, default=35554)
    a = ap.parse_args()
    n, p, m = a.n, a.p, a.m
    Y, G, K = synth(n, p, m, 1)
    dev = torch.device("cuda", 0)
    ctx = B.Context(0, torch.cuda.current_stream().cuda_stream)
    dY = torch.from_numpy(np.ascontiguousarray(Y.T)).to(dev)
    dG = torch.from_numpy(np.ascontiguousarray(G.T)).to(dev)
    dK = torch.from_numpy(np.ascontiguousarray(K.T)).to(dev)
    dL = torch.empty((m, p), dtype=torch.float64, device=dev)
    dH = torch.empty(m, dtype=torch.float64, device=dev)
    mx = torch.empty(m, dtype=torch.float64, device=dev)
    ax = torch.empty(m, dtype=torch.int64, device=dev)
    cap = 1 << 21
    ti, tj = torch.empty(cap, dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.int32, device=dev)
    tl, tc = torch.empty(cap, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
    info = torch.zeros(B._lib.BLMM_RINFO_LEN, dtype=torch.int64, device=dev)
    trip = dict(threshold=5.0, trip_i=ti, trip_j=tj, trip_lod=tl, trip_count=tc)
    calls = {
        "store": lambda: B.bulkscan_dev(ctx, dY, dG, dK, dL, dH, method="null-exact"),
        "sync": lambda: B.bulkscan_reduced_dev(ctx, dY, dG, dK, mx, ax, dH, method="null-exact", **trip),
        "async": lambda: B.bulkscan_reduced_async(ctx, dY, dG, dK, mx, ax, dH, info, method="null-exact", **trip),
    }

    def timed(f):
        for _ in range(a.warmup):
            f()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.steps

    out = {"shape": {"n": n, "p": p, "m": m, "method": "null-exact"}, "steps": a.steps, "warmup": a.warmup,
           "threshold": 5.0, "unit": "ms per step, back to back, one final synchronisation"}
    for label, tol in (("default", None), ("lr_tol_0", 0.0)):
        ctx.set_tuning("defaults", 0)
        if tol is not None:
            ctx.set_tuning("lr_tol", tol)
        res = {k: timed(f) for k, f in calls.items()}
        res["async_info"] = B.reduced_info(info.cpu().numpy())
        res["sync_route"] = int(ctx.lib.blmm_last_reduced_route(ctx.h))
        out[label] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
