"""bulkscan_multidf_perms_dev on device inputs at the BXD width (n = 79, P = 7321 loci, k = 2 and 8, m = 512 traits, 1000
permutations): wall time per call after a warm-up (one synchronisation per call) and the library's own phase timers
(blmm_set_timing).  The yardstick is k_mdf_grid's rate for the same (K, TJ): 2 n P k m (nperms + 1) flop per call.
--kernel-stats: the kernel statistics of a `rocprofv3 --kernel-trace --stats -- python tools/multidf_perms_time.py --k K` run (its
kernel_stats.csv, or the results .db), folded into the phases fit (design, eigen, rotations, h2 search, generator), tables
(k_mdf_table), panels, scan (k_mdf_grid_red + k_red_final) and summary, per call.
Prints one JSON line (--out: also written there, merged by k; profiles/multidf_perms_time.json)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def phase_of(kernel):
    k = kernel.split("(")[0]
    if "k_mdf_table" in k:
        return "tables"
    if "k_bperm_summary" in k:
        return "summary"
    if "k_bperm" in k:
        return "panels"
    if "k_mdf_grid_red" in k or "k_red_final" in k:
        return "scan"
    return "fit"


def fold_stats(path, calls):
    """rocprofv3 kernel statistics -> ms per call and phase.  CSV: Name, TotalDurationNs; .db: the top_kernels view (name, calls,
    total in microseconds)."""
    if path.endswith(".db"):
        import sqlite3
        rows = [(r[0], float(r[2]) / 1e3) for r in sqlite3.connect(path).execute("select * from top_kernels")]
    else:
        import csv
        with open(path) as f:
            rows = [(r["Name"], float(r["TotalDurationNs"]) / 1e6) for r in csv.DictReader(f)]
    out = {}
    for name, ms in rows:
        out[phase_of(name)] = out.get(phase_of(name), 0.0) + ms / calls
        if "k_mdf_grid_red" in name:
            out["k_mdf_grid_red"] = out.get("k_mdf_grid_red", 0.0) + ms / calls
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, nargs="+", default=[2, 8])
    ap.add_argument("--nperms", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--n", type=int, default=79)
    ap.add_argument("--loci", type=int, default=7321)
    ap.add_argument("--m", type=int, default=512)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = {"shape": {"n": a.n, "loci": a.loci, "m": a.m}, "nperms": a.nperms, "reps": a.reps, "k": {}}
    if a.out and os.path.exists(a.out):
        old = json.load(open(a.out))
        if old.get("shape") == out["shape"] and old.get("nperms") == a.nperms:
            out["k"] = old["k"]
    if a.kernel_stats:
        # the stats of a profiled run of this tool with one k: warm-up + reps calls
        out["k"].setdefault(str(a.k[0]), {})["phase_ms_per_call"] = fold_stats(a.kernel_stats, a.reps + 1)
    else:
        import torch
        import bulklmm_jl_amd as B
        from test_gpu_multidf import _founder_data
        dev = torch.device("cuda", 0)
        ctx = B.Context(0, torch.cuda.current_stream().cuda_stream)
        ctx.set_timing(True)
        f64 = dict(dtype=torch.float64, device=dev)
        n, m = a.n, a.m
        for k in a.k:
            Y, G, K, _ = _founder_data(n, a.loci, k, m, seed=79 + k)
            dY, dG, dK = (torch.from_numpy(np.ascontiguousarray(x.T)).to(dev) for x in (Y, G, K))
            h2, s2, mx, pv = (torch.empty(m, **f64) for _ in range(4))
            arg = torch.empty(m, dtype=torch.int64, device=dev)
            mp = torch.empty((m, max(a.nperms, 1)), **f64)
            thr = torch.empty((m, 2), **f64)

            def call():
                B.bulkscan_multidf_perms_dev(ctx, dY, dG, dK, k, h2, s2, mx, arg, mp, thr, pv, nperms=a.nperms, seed=1)
                ctx.synchronize()

            call()
            ctx.read_timings()
            times = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                call()
                times.append(time.perf_counter() - t0)
            flop = 2.0 * n * a.loci * k * m * (a.nperms + 1)
            r = out["k"].setdefault(str(k), {})
            r.update({"wall_s": {"min": min(times), "all": times}, "scan_flop": flop, "timers_ms_sum": ctx.read_timings()[0],
                      "finite": bool(torch.isfinite(mp).all().item())})
            del dY, dG, dK
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
