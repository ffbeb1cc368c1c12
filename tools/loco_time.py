"""Wall time of the leave-one-chromosome-out bulkscan against the per-chromosome calls it replaces.

BXD shape (n = 79, p = 7321 in the 20 runs of tests/golden/bxd_chr_runs.json, m = 35554), null-exact and null-grid:
  dev_loco       bulkscan_loco_dev on resident torch inputs, kinships computed inside the call (K_loco = None)
  dev_loco_k     ... with the 20 kinships passed in (computed once outside)
  dev_separate   20 bulkscan_dev(Y, G_c, K_c) calls into the column blocks of one L (K_c resident), one synchronisation at the end
  host_loco      bulkscan_loco (host arrays in and out)
  host_separate  20 bulkscan(Y, G[:, rows_c], K_c) host calls
  phases         blmm_status phase times of one timed bulkscan_loco_dev call against one bulkscan_dev call on chromosome 1
and kinship_loco against kinship (device forms) at the BXD shape and at n = 1000, p = 1e5 (BASELINE configs[4]); then one
configs[2]-like shape (n = 500, p = 50000, m = 2500, 20 equal chromosomes: the per-chromosome divide-and-conquer eigen path).
Every figure is the median over --reps calls after one warm-up call.  Prints one JSON line; --out writes it to a file as well.
--reduced: bulkscan_loco_reduced at the BXD shape instead (null-exact, null-grid), against the full-matrix forms of the same run:
  host_reduced_ms  bulkscan_loco_reduced (host arrays in, peaks, chromosome tables and h2 out; no threshold)
  host_reduced_thr_ms  ... with threshold = 5 (the LOD > 5 triplets too)
  dev_reduced_ms   bulkscan_loco_reduced_dev on resident torch inputs and outputs (kinships inside the call)
  host_loco_ms / dev_loco_ms   bulkscan_loco / bulkscan_loco_dev as above
  phases_reduced_ms  blmm_status phase times of one timed dev call (summed over the chromosomes)
--eig-trace: the workload for a kernel trace of the eigen phase (single against batched launches); --fold-eig-trace CSV: its summary."""
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
from common import make_geno  # noqa: E402

GRID = [i / 10.0 for i in range(10)]


def bxd_chrom():
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "bxd_chr_runs.json")))
    return [lab for lab, k in zip(fx["chromosomes"], fx["counts"]) for _ in range(k)]


def med(f, reps):
    f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def shape_run(n, p, m, chrom, methods, reps, host):
    rng = np.random.default_rng(20241)
    G = make_geno(n, p, rng)
    Y = 10.0 + rng.standard_normal((n, m))
    _, cs = B.chromosome_runs(chrom, p)
    nchr = len(cs) - 1
    dev = torch.device("cuda", 0)
    ctx = B.Context(0, torch.cuda.current_stream().cuda_stream)
    sync = torch.cuda.synchronize
    dY = torch.from_numpy(np.ascontiguousarray(Y.T)).to(dev)
    dG = torch.from_numpy(np.ascontiguousarray(G.T)).to(dev)
    Kl = B.calcKinship_loco(G, chrom, ctx=ctx)
    dK = torch.from_numpy(np.ascontiguousarray(Kl)).to(dev)
    dL = torch.empty((m, p), dtype=torch.float64, device=dev)
    dh = torch.empty((nchr, m), dtype=torch.float64, device=dev)
    out = {"shape": {"n": n, "p": p, "m": m, "nchr": nchr}}
    for meth in methods:
        r = {}

        def loco(K=None):
            B.bulkscan_loco_dev(ctx, dY, dG, cs, dL, dh, method=meth, h2_grid=GRID, K_loco=K)
            sync()

        def separate():
            for c in range(nchr):
                s0, s1 = int(cs[c]), int(cs[c + 1])
                B.bulkscan_dev(ctx, dY, dG[s0:s1], dK[c], dL[:, s0:s1], dh[c], method=meth, h2_grid=GRID)
            sync()

        r["dev_loco_ms"] = med(loco, reps)
        r["dev_loco_k_ms"] = med(lambda: loco(dK), reps)
        r["dev_separate_ms"] = med(separate, reps)
        r["dev_speedup"] = r["dev_separate_ms"] / r["dev_loco_ms"]
        if host:
            Ks = [np.asfortranarray(Kl[c]) for c in range(nchr)]
            r["host_loco_ms"] = med(lambda: B.bulkscan_loco(Y, G, chrom, method=meth, h2_grid=GRID, ctx=ctx), reps)

            def host_sep():
                for c in range(nchr):
                    B.bulkscan(Y, G[:, cs[c]:cs[c + 1]], Ks[c], method=meth, h2_grid=GRID, ctx=ctx)
            r["host_separate_ms"] = med(host_sep, reps)
        # phase split: the summed phases of one LOCO call against one single call on the first chromosome
        ctx.set_timing(True)
        st = B.bulkscan_loco_dev(ctx, dY, dG, cs, dL, dh, method=meth, h2_grid=GRID, K_loco=dK, status=True)
        s0, s1 = int(cs[0]), int(cs[1])
        st1 = B.bulkscan_dev(ctx, dY, dG[s0:s1], dK[0], dL[:, s0:s1], dh[0], method=meth, h2_grid=GRID, status=True)
        ctx.read_timings()
        ctx.set_timing(False)
        names = ("t_eigen_ms", "t_rotate_ms", "t_h2_ms", "t_prep_ms", "t_scan_ms", "t_total_ms")
        r["phases_loco_ms"] = {k: round(getattr(st, k), 4) for k in names}
        r["phases_single_chr1_ms"] = {k: round(getattr(st1, k), 4) for k in names}
        r["eigen_loco_over_single"] = st.t_eigen_ms / max(st1.t_eigen_ms, 1e-9)
        out[meth] = r
        print(meth, json.dumps(r), flush=True)
    return out


def reduced_run(reps):
    n, m = 79, 35554
    chrom = bxd_chrom()
    p = len(chrom)
    rng = np.random.default_rng(20241)
    G = make_geno(n, p, rng)
    Y = 10.0 + rng.standard_normal((n, m))
    _, cs = B.chromosome_runs(chrom, p)
    nchr = len(cs) - 1
    dev = torch.device("cuda", 0)
    ctx = B.Context(0, torch.cuda.current_stream().cuda_stream)
    sync = torch.cuda.synchronize
    dY = torch.from_numpy(np.ascontiguousarray(Y.T)).to(dev)
    dG = torch.from_numpy(np.ascontiguousarray(G.T)).to(dev)
    dL = torch.empty((m, p), dtype=torch.float64, device=dev)
    dh = torch.empty((nchr, m), dtype=torch.float64, device=dev)
    mx = torch.empty(m, dtype=torch.float64, device=dev)
    ax = torch.empty(m, dtype=torch.int64, device=dev)
    cmx = torch.empty((nchr, m), dtype=torch.float64, device=dev)
    cax = torch.empty((nchr, m), dtype=torch.int64, device=dev)
    out = {"shape": {"n": n, "p": p, "m": m, "nchr": nchr}}
    for meth in ("null-exact", "null-grid"):
        r = {}

        def dev_loco():
            B.bulkscan_loco_dev(ctx, dY, dG, cs, dL, dh, method=meth, h2_grid=GRID)
            sync()

        def dev_red():
            B.bulkscan_loco_reduced_dev(ctx, dY, dG, cs, mx, ax, cmx, cax, dh, method=meth, h2_grid=GRID)
            sync()

        r["host_loco_ms"] = med(lambda: B.bulkscan_loco(Y, G, chrom, method=meth, h2_grid=GRID, ctx=ctx), reps)
        r["dev_loco_ms"] = med(dev_loco, reps)
        r["host_reduced_ms"] = med(lambda: B.bulkscan_loco_reduced(Y, G, chrom, method=meth, h2_grid=GRID, ctx=ctx), reps)
        r["host_reduced_thr_ms"] = med(lambda: B.bulkscan_loco_reduced(Y, G, chrom, method=meth, h2_grid=GRID, threshold=5.0, ctx=ctx), reps)
        r["dev_reduced_ms"] = med(dev_red, reps)
        r["host_loco_over_host_reduced"] = r["host_loco_ms"] / r["host_reduced_ms"]
        r["host_reduced_over_dev_loco"] = r["host_reduced_ms"] / r["dev_loco_ms"]
        r["route"] = B.bulkscan_loco_reduced(Y[:, :64], G, chrom, method=meth, h2_grid=GRID, ctx=ctx)["route"]
        ctx.set_timing(True)
        st = B.bulkscan_loco_reduced_dev(ctx, dY, dG, cs, mx, ax, cmx, cax, dh, method=meth, h2_grid=GRID, status=True)
        ctx.read_timings()
        ctx.set_timing(False)
        names = ("t_eigen_ms", "t_rotate_ms", "t_h2_ms", "t_prep_ms", "t_scan_ms", "t_total_ms")
        r["phases_reduced_ms"] = {k: round(getattr(st, k), 4) for k in names}
        out[meth] = r
        print(meth, json.dumps(r), flush=True)
    return out


def kinship_run(n, p, nchr, reps):
    rng = np.random.default_rng(7)
    G = (rng.random((n, p)) < 0.5).astype(np.float64)
    b = np.linspace(0, p, nchr + 1).round().astype(np.int64)
    dev = torch.device("cuda", 0)
    ctx = B.Context(0, torch.cuda.current_stream().cuda_stream)
    dG = torch.from_numpy(np.ascontiguousarray(G.T)).to(dev)
    dK = torch.empty((n, n), dtype=torch.float64, device=dev)
    dKl = torch.empty((nchr, n, n), dtype=torch.float64, device=dev)

    def one():
        ctx.check(ctx.lib.blmm_kinship_dev(ctx.h, dG.data_ptr(), n, p, dK.data_ptr()))
        torch.cuda.synchronize()

    def loco():
        ctx.check(ctx.lib.blmm_kinship_loco_dev(ctx.h, dG.data_ptr(), n, p, b.ctypes.data, nchr, -1, dKl.data_ptr()))
        torch.cuda.synchronize()
    r = {"n": n, "p": p, "nchr": nchr, "kinship_ms": med(one, reps), "kinship_loco_ms": med(loco, reps)}
    r["loco_over_kinship"] = r["kinship_loco_ms"] / r["kinship_ms"]
    print("kinship", json.dumps(r), flush=True)
    return r


def eig_trace(reps):
    """The workload of a kernel trace (rocprofv3 --kernel-trace -- python tools/loco_time.py --eig-trace): at the BXD shape (m = 1024:
    the eigen phase does not depend on m), `reps` single bulkscan_dev calls on chromosome 1, then `reps` bulkscan_loco_dev calls."""
    chrom = bxd_chrom()
    rng = np.random.default_rng(20241)
    G = make_geno(79, len(chrom), rng)
    Y = 10.0 + rng.standard_normal((79, 1024))
    _, cs = B.chromosome_runs(chrom, G.shape[1])
    dev = torch.device("cuda", 0)
    ctx = B.Context(0, torch.cuda.current_stream().cuda_stream)
    dY = torch.from_numpy(np.ascontiguousarray(Y.T)).to(dev)
    dG = torch.from_numpy(np.ascontiguousarray(G.T)).to(dev)
    dK = torch.from_numpy(np.ascontiguousarray(B.calcKinship_loco(G, chrom, ctx=ctx))).to(dev)
    dL = torch.empty((1024, G.shape[1]), dtype=torch.float64, device=dev)
    dh = torch.empty((len(cs) - 1, 1024), dtype=torch.float64, device=dev)
    for _ in range(reps):
        B.bulkscan_dev(ctx, dY, dG[0:int(cs[1])], dK[0], dL[:, 0:int(cs[1])], dh[0])
    torch.cuda.synchronize()
    for _ in range(reps):
        B.bulkscan_loco_dev(ctx, dY, dG, cs, dL, dh, K_loco=dK)
    torch.cuda.synchronize()


def fold_eig_trace(path):
    """Kernel-trace CSV of an --eig-trace run -> the fast eigen path per call: single launches (Grid_Size_Y = 1) against the
    batched ones (Grid_Size_Y = nchr): summed kernel time and the span from k_eigf_reduce's start to k_backtransform's end."""
    import csv
    rows = list(csv.DictReader(open(path)))
    names = ("k_eigf_reduce", "k_eigf_pairs", "k_backtransform")
    out = {}
    for kind, sel in (("single", lambda y: y == 1), ("batched", lambda y: y > 1)):
        ev = [r for r in rows if any(k in r["Kernel_Name"] for k in names) and sel(int(r.get("Grid_Size_Y", r.get("Grid_Size_y", 1))))]
        ev.sort(key=lambda r: int(r["Start_Timestamp"]))
        calls = [ev[i:i + 3] for i in range(0, len(ev) - 2, 3)]
        if not calls:
            continue
        busy = [sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in c) / 1e6 for c in calls]
        span = [(int(c[-1]["End_Timestamp"]) - int(c[0]["Start_Timestamp"])) / 1e6 for c in calls]
        out[kind] = {"calls": len(calls), "kernel_ms_median": float(np.median(busy)), "span_ms_median": float(np.median(span)),
                     "grid_y": int(calls[0][0].get("Grid_Size_Y", 1))}
    if "single" in out and "batched" in out:
        out["batched_over_single_span"] = out["batched"]["span_ms_median"] / out["single"]["span_ms_median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--eig-trace", action="store_true")
    ap.add_argument("--fold-eig-trace", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-large", action="store_true")
    ap.add_argument("--reduced", action="store_true")
    a = ap.parse_args()
    if a.fold_eig_trace:
        line = json.dumps(fold_eig_trace(a.fold_eig_trace))
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return
    if a.eig_trace:
        eig_trace(a.reps)
        return
    res = {"device": torch.cuda.get_device_name(0)}
    if a.reduced:
        res["reduced_bxd"] = reduced_run(a.reps)
        line = json.dumps(res)
        print(line)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return
    res["bxd"] = shape_run(79, 7321, 35554, bxd_chrom(), ("null-exact", "null-grid"), a.reps, not a.no_host)
    res["kinship_bxd"] = kinship_run(79, 7321, 20, a.reps)
    res["kinship_n1000_p1e5"] = kinship_run(1000, 100000, 20, a.reps)
    if not a.no_large:
        p = 50000
        b = np.linspace(0, p, 21).round().astype(int)
        chrom = [str(c + 1) for c in range(20) for _ in range(b[c + 1] - b[c])]
        res["n500"] = shape_run(500, p, 2500, chrom, ("null-exact",), max(2, a.reps // 2), False)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
