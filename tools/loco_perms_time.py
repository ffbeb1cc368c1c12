"""Wall time of the leave-one-chromosome-out permutation test at the BXD shape (n = 79, p = 7321, m = 35554, the chromosome runs of
tests/golden/bxd_chr_runs.json) with `nperms` permutations:
  loco_dev    bulkscan_loco_perms_dev on device inputs (torch), kinships computed inside the call, after a warm-up call, one
              synchronisation per call;
  loco_host   bulkscan_loco_perms (host arrays in, every table back; no chr_max_perms), one call after the warm-up;
  host_loop   what the call replaces: calcKinship_loco + one bulkscan_perms per chromosome (host form, its max_perms downloaded) + the
              NumPy combine (maximum over chromosomes, quantiles, p-values).
--kernel-stats: the kernel statistics of a `rocprofv3 --kernel-trace --stats -- python tools/loco_perms_time.py --no-loop` run
(its kernel_stats.csv, or the results .db); kernel times are folded into the phases fit (kinships, design, eigen, rotation, h2
search, generator), isx, panels, scan (table kernel + k_red_final), summary and merge, per call.
--merge PATH: update the JSON object in PATH with this run's keys (profiles/loco_perms_time.json).  Prints one JSON line."""
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

SIG = (0.10, 0.05)


def phase_of(kernel):
    k = kernel.split("(")[0]
    if "k_isx" in k:
        return "isx"
    if "k_bperm_summary" in k:
        return "summary"
    if "k_bperm_loco" in k:
        return "merge"
    if "k_bperm" in k:
        return "panels"
    if "k_scan" in k or "k_red_final" in k:
        return "scan"
    return "fit"


def fold_stats(path, calls):
    """rocprofv3 kernel statistics -> ms per call and phase.  CSV: Name, TotalDurationNs; .db: the top_kernels view (name, calls,
    total in microseconds)."""
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
    total = sum(out.values())
    return {k: round(v, 3) for k, v in out.items()}, {k: round(v / total, 4) for k, v in out.items()} if total > 0 else {}


def quantiles(mp, probs):
    nperms = mp.shape[0]
    s = np.sort(mp, axis=0)
    out = np.empty((len(probs), mp.shape[1]))
    for t, q in enumerate(probs):
        h = (nperms - 1) * min(max(q, 0.0), 1.0)
        lo = int(np.floor(h))
        hi = min(lo + 1, nperms - 1)
        out[t] = s[lo] + (h - lo) * (s[hi] - s[lo])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nperms", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--m", type=int, default=35554)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--no-loop", action="store_true")
    ap.add_argument("--merge", default=None)
    a = ap.parse_args()
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "bxd_chr_runs.json")))
    chrom = [lab for lab, k in zip(fx["chromosomes"], fx["counts"]) for _ in range(k)]
    n, p, m = 79, len(chrom), a.m
    out = {"shape": {"n": n, "p": p, "m": m, "nchr": len(fx["counts"])}, "nperms": a.nperms}
    if a.kernel_stats:
        # the stats of a profiled run of this tool: warm-up + reps device calls, no host loop
        out["phase_ms_per_call"], out["phase_share"] = fold_stats(a.kernel_stats, a.reps + 1)
    else:
        from common import make_data
        Y, G, _, _ = make_data(n=n, p=p, m=m, seed=20241)
        runs, cs = B.chromosome_runs(chrom, p)
        nchr = len(runs)
        dev = torch.device("cuda", 0)
        ctx = B.Context(0, torch.cuda.current_stream().cuda_stream)
        dY = torch.from_numpy(np.ascontiguousarray(Y.T)).to(dev)
        dG = torch.from_numpy(np.ascontiguousarray(G.T)).to(dev)
        f64 = dict(dtype=torch.float64, device=dev)
        h2, s2 = torch.empty((nchr, m), **f64), torch.empty((nchr, m), **f64)
        mx, pv = torch.empty(m, **f64), torch.empty(m, **f64)
        arg = torch.empty(m, dtype=torch.int64, device=dev)
        mp = torch.empty((m, max(a.nperms, 1)), **f64)
        thr = torch.empty((m, 2), **f64)
        cmx, cpv = torch.empty((nchr, m), **f64), torch.empty((nchr, m), **f64)
        carg = torch.empty((nchr, m), dtype=torch.int64, device=dev)
        cthr = torch.empty((nchr, m, 2), **f64)

        def loco():
            B.bulkscan_loco_perms_dev(ctx, dY, dG, cs, h2, s2, mx, arg, mp, thr, pv, cmx, carg, None, cthr, cpv, nperms=a.nperms, seed=1)
            ctx.synchronize()

        loco()
        times = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            loco()
            times.append(time.perf_counter() - t0)
        out["loco_dev_s"] = {"min": min(times), "all": times}
        if not a.no_loop:
            t0 = time.perf_counter()
            res = B.bulkscan_loco_perms(Y, G, chrom, nperms=a.nperms, rndseed=1, ctx=ctx)
            out["loco_host_s"] = time.perf_counter() - t0
            # the host loop it replaces (a warm-up of bulkscan_perms first: workspace and code objects are not the loop's cost)
            B.bulkscan_perms(Y[:, :64], G[:, cs[0]:cs[1]], np.eye(n), nperms=a.nperms, ctx=ctx)
            t0 = time.perf_counter()
            Kl = B.calcKinship_loco(G, chrom, ctx=ctx)
            t_kin = time.perf_counter() - t0
            cm, ca, gm = [], [], None
            for c in range(nchr):
                r = B.bulkscan_perms(Y, G[:, cs[c]:cs[c + 1]], np.ascontiguousarray(Kl[c]), nperms=a.nperms, rndseed=1,
                                     signif_level=SIG, ctx=ctx)
                cm.append(r["lod_max"])
                ca.append(np.where(r["lod_argmax"] >= 0, r["lod_argmax"] + cs[c], -1))
                gm = r["max_perms"] if gm is None else np.maximum(gm, r["max_perms"])
            t_perms = time.perf_counter() - t0 - t_kin
            t1 = time.perf_counter()
            cm = np.stack(cm)
            lod_max = cm.max(axis=0)
            lod_argmax = np.stack(ca)[np.argmax(cm, axis=0), np.arange(m)]
            thr_h = quantiles(gm, 1.0 - np.asarray(SIG))
            pv_h = (1.0 + ((gm >= lod_max[None, :]) & (gm != -np.inf)).sum(axis=0)) / (a.nperms + 1.0)
            t_comb = time.perf_counter() - t1
            loop = time.perf_counter() - t0
            out["host_loop_s"] = {"total": loop, "calcKinship_loco": t_kin, "bulkscan_perms_calls": t_perms, "numpy_combine": t_comb}
            out["speedup_vs_host_loop"] = {"host_form": loop / out["loco_host_s"], "dev_form": loop / min(times)}
            out["host_loop_agrees"] = bool(np.array_equal(res["max_perms"], gm) and np.array_equal(res["lod_max"], lod_max) and
                                           np.array_equal(res["lod_argmax"], lod_argmax) and np.array_equal(res["pvals_perm"], pv_h) and
                                           np.allclose(res["thresholds"], thr_h, rtol=1e-12, atol=1e-13))
    if a.merge:
        cur = json.load(open(a.merge)) if os.path.exists(a.merge) else {}
        cur.update(out)
        with open(a.merge, "w") as f:
            json.dump(cur, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
