"""bulkscan_multidf_reduced against the routes it replaces, at the BXD shape (n = 79, P = 7321 loci, m = 35554 traits): null-grid k = 2
and k = 8 and null-exact k = 2, wall time of the last of three calls of
  reduced_host    bulkscan_multidf_reduced (host arrays in, peaks out)
  reduced_dev     bulkscan_multidf_reduced_dev on device tensors
  stored_host     blmm_bulkscan_multidf with L into pinned host memory + NumPy max / argmax over it (what a caller had to do before)
  stored_dev      bulkscan_multidf_dev with L left on the device + blmm_lod_colmax_dev
--kernel-stats: the kernel statistics (kernel_stats.csv) of a `rocprofv3 --kernel-trace --stats -- python
tools/multidf_reduced_time.py --case METHOD K --routes reduced_dev stored_dev` run: the reducing kernel beside the storing kernel of the
same run (average / min / max per launch) and the expectation `reducing average <= storing average + the storing kernel's spread`.
Prints one JSON line (--out: also written there, merged by case; profiles/multidf_reduced_time.json)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = [("null-grid", 2), ("null-grid", 8), ("null-exact", 2)]
ROUTES = ["reduced_host", "reduced_dev", "stored_host", "stored_dev"]
PAIRS = {"null-grid": ("k_mdf_grid_red<", "k_mdf_grid<"), "null-exact": ("k_mdf_exact_red<", "k_mdf_exact<")}


def fold_stats(path, method):
    import csv
    red, sto = PAIRS[method]
    out = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            for key, tag in (("reducing", red), ("storing", sto)):
                if tag in r["Name"]:
                    out[key] = {"kernel": r["Name"].split("(")[0], "calls": int(r["Calls"]), "avg_ms": float(r["AverageNs"]) / 1e6,
                                "min_ms": float(r["MinNs"]) / 1e6, "max_ms": float(r["MaxNs"]) / 1e6}
            if "k_red_final" in r["Name"]:
                out["k_red_final_avg_ms"] = float(r["AverageNs"]) / 1e6
    if "reducing" in out and "storing" in out:
        s = out["storing"]
        out["bound_ms"] = s["avg_ms"] + (s["max_ms"] - s["min_ms"])
        out["within_expectation"] = out["reducing"]["avg_ms"] <= out["bound_ms"]
    return out


def last_of(fn, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return {"last_ms": 1e3 * t[-1], "all_ms": [1e3 * x for x in t]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", nargs=2, action="append", metavar=("METHOD", "K"), default=None)
    ap.add_argument("--routes", nargs="+", default=ROUTES, choices=ROUTES)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--n", type=int, default=79)
    ap.add_argument("--loci", type=int, default=7321)
    ap.add_argument("--m", type=int, default=35554)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cases = [(mth, int(k)) for mth, k in a.case] if a.case else CASES
    out = {"shape": {"n": a.n, "loci": a.loci, "m": a.m}, "reps": a.reps, "cases": {}}
    if a.out and os.path.exists(a.out):
        old = json.load(open(a.out))
        if old.get("shape") == out["shape"]:
            out["cases"] = old["cases"]
    if a.kernel_stats:
        method, k = cases[0]
        out["cases"].setdefault(f"{method} k={k}", {})["kernels"] = fold_stats(a.kernel_stats, method)
    else:
        import torch
        import bulklmm_jl_amd as B
        from test_gpu_multidf import _founder_data
        dev = torch.device("cuda", 0)
        ctx = B.Context(0, torch.cuda.current_stream().cuda_stream)
        f64 = dict(dtype=torch.float64, device=dev)
        n, m, P = a.n, a.m, a.loci
        grid = np.array([i / 10.0 for i in range(10)])
        for method, k in cases:
            Y, G, K, _ = _founder_data(n, P, k, m, seed=79 + k)
            res = out["cases"].setdefault(f"{method} k={k}", {})
            res["L_bytes"] = 8 * P * m
            peaks = {}
            if "reduced_host" in a.routes:
                def f():
                    peaks["reduced_host"] = B.bulkscan_multidf_reduced(Y, G, K, k, method=method, ctx=ctx)
                res["reduced_host"] = last_of(f, a.reps)
            if "stored_host" in a.routes:
                Yf, Gf, Kf = (np.asfortranarray(x) for x in (Y, G, K))
                Lh = np.empty((P, m), order="F"); h2 = np.empty(m)
                B.host_register(Lh)
                o = B.api._opts(B.api._METHODS[method])
                vp = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731

                def f():
                    ctx.check(ctx.lib.blmm_bulkscan_multidf(ctx.h, C.byref(o), vp(Yf), n, m, vp(Gf), P * k, k, None, 0, vp(Kf), None,
                                                            None if method == "null-exact" else vp(grid),
                                                            0 if method == "null-exact" else len(grid), vp(Lh), vp(h2), None))
                    arg = np.argmax(Lh, axis=0)
                    peaks["stored_host"] = {"argmax": arg, "max_lod": Lh[arg, np.arange(m)]}
                res["stored_host"] = last_of(f, a.reps)
                B.host_unregister(Lh)
                del Lh
            if "reduced_dev" in a.routes or "stored_dev" in a.routes:
                dY, dG, dK = (torch.from_numpy(np.ascontiguousarray(x.T)).to(dev) for x in (Y, G, K))
                mx, h2d = torch.empty(m, **f64), torch.empty(m, **f64)
                arg = torch.empty(m, dtype=torch.int64, device=dev)
                if "reduced_dev" in a.routes:
                    def f():
                        B.bulkscan_multidf_reduced_dev(ctx, dY, dG, dK, k, mx, arg, h2d, method=method)
                    res["reduced_dev"] = last_of(f, a.reps)
                    peaks["reduced_dev"] = {"argmax": arg.cpu().numpy(), "max_lod": mx.cpu().numpy()}
                if "stored_dev" in a.routes:
                    Ld = torch.empty((m, P), **f64)

                    def f():
                        B.bulkscan_multidf_dev(ctx, dY, dG, dK, k, Ld, h2d, method=method)
                        ctx.check(ctx.lib.blmm_lod_colmax_dev(ctx.h, Ld.data_ptr(), P, m, P, mx.data_ptr(), arg.data_ptr()))
                        ctx.synchronize()
                    res["stored_dev"] = last_of(f, a.reps)
                    peaks["stored_dev"] = {"argmax": arg.cpu().numpy(), "max_lod": mx.cpu().numpy()}
                    del Ld
                del dY, dG, dK
            names = list(peaks)
            res["peaks_equal"] = all(np.array_equal(peaks[names[0]][f], peaks[x][f]) for x in names[1:] for f in ("argmax", "max_lod"))
            if "reduced_host" in res and "stored_host" in res:
                res["host_ratio_stored_over_reduced"] = res["stored_host"]["last_ms"] / res["reduced_host"]["last_ms"]
            if "reduced_dev" in res and "stored_dev" in res:
                res["dev_ratio_stored_over_reduced"] = res["stored_dev"]["last_ms"] / res["reduced_dev"]["last_ms"]
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
