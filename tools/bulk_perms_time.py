"""Wall time of the permutation test for every trait at the BXD shape (BASELINE.json configs[1]: n = 79, p = 7321, m = 35554)
with `nperms` permutations:
  bulk        bulkscan_perms_dev on device inputs (torch), after a warm-up call, one synchronisation per call;
  scan_loop   scan(y_j, ...; permutation_test=True) for `loop_traits` traits one after the other (the single-trait route a user has
              without bulkscan_perms: L_perms of every trait comes back to the host), extrapolated to all m traits.
--kernel-stats: the kernel statistics of a `rocprofv3 --kernel-trace --stats -- python tools/bulk_perms_time.py --no-loop` run
(its kernel_stats.csv, or the results .db of the default output format); the kernel times are folded into the phases fit (design,
eigen, rotation, h2 search, generator), isx, panels, scan (table kernel + k_red_final) and summary, per bulk call.
Prints one JSON line (profiles/bulk_perms_time.json)."""
import argparse
import csv
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


def phase_of(kernel):
    k = kernel.split("(")[0]
    if "k_isx" in k:
        return "isx"
    if "k_bperm_summary" in k:
        return "summary"
    if "k_bperm" in k:
        return "panels"
    if "k_scan" in k or "k_red_final" in k:
        return "scan"
    return "fit"


def fold_stats(path, calls):
    """rocprofv3 kernel statistics -> ms per bulk call and phase.  CSV: Name, TotalDurationNs; .db: the top_kernels view
    (name, calls, total in microseconds)."""
    rows = []
    if path.endswith(".db"):
        import sqlite3
        rows = [(r[0], float(r[2]) / 1e3) for r in sqlite3.connect(path).execute("select * from top_kernels")]
    else:
        with open(path) as f:
            rows = [(r["Name"], float(r["TotalDurationNs"]) / 1e6) for r in csv.DictReader(f)]
    out = {}
    for name, ms in rows:
        ph = phase_of(name)
        out[ph] = out.get(ph, 0.0) + ms / calls
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nperms", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loop-traits", type=int, default=200)
    ap.add_argument("--n", type=int, default=79)
    ap.add_argument("--p", type=int, default=7321)
    ap.add_argument("--m", type=int, default=35554)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--no-loop", action="store_true")
    a = ap.parse_args()
    out = {"shape": {"n": a.n, "p": a.p, "m": a.m}, "nperms": a.nperms}
    if a.kernel_stats:
        # the stats of a profiled run of this tool: warm-up + reps bulk calls, no scan loop
        out["phase_ms_per_call"] = fold_stats(a.kernel_stats, a.reps + 1)
        print(json.dumps(out))
        return
    from common import make_data
    Y, G, K, _ = make_data(n=a.n, p=a.p, m=a.m, seed=20241, bxd=(a.n == 79))
    n, p, m = a.n, a.p, a.m
    dev = torch.device("cuda", 0)
    ctx = B.Context(0, torch.cuda.current_stream().cuda_stream)
    dY = torch.from_numpy(np.ascontiguousarray(Y.T)).to(dev)
    dG = torch.from_numpy(np.ascontiguousarray(G.T)).to(dev)
    dK = torch.from_numpy(np.ascontiguousarray(K.T)).to(dev)
    f64 = dict(dtype=torch.float64, device=dev)
    h2, s2, mx, pv = (torch.empty(m, **f64) for _ in range(4))
    arg = torch.empty(m, dtype=torch.int64, device=dev)
    mp = torch.empty((m, max(a.nperms, 1)), **f64)
    thr = torch.empty((m, 2), **f64)

    def bulk():
        B.bulkscan_perms_dev(ctx, dY, dG, dK, h2, s2, mx, arg, mp, thr, pv, nperms=a.nperms, seed=1)
        ctx.synchronize()

    bulk()
    times = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        bulk()
        times.append(time.perf_counter() - t0)
    out["bulk_s"] = {"min": min(times), "all": times}
    if not a.no_loop:
        k = min(a.loop_traits, m)
        B.scan(Y[:, 0], G, K, permutation_test=True, nperms=a.nperms, rndseed=1, ctx=ctx)    # warm-up
        t0 = time.perf_counter()
        for j in range(k):
            B.scan(Y[:, j], G, K, permutation_test=True, nperms=a.nperms, rndseed=1, ctx=ctx)
        loop = time.perf_counter() - t0
        out["scan_loop"] = {"traits": k, "s": loop, "s_per_trait": loop / k, "extrapolated_all_traits_s": loop / k * m}
        out["speedup_vs_scan_loop"] = loop / k * m / min(times)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
