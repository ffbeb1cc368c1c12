"""Times bulkscan_stepwise at the BXD shape (n = 79, p = 7321, m = 35554, BXD kinship) on synthetic data: make_data's traits (30 % of
them carry one marker effect drawn from N(0, 1.5^2)) with a second planted locus of size 1.5 on every tenth trait; max_loci = 4,
threshold 4.0, both methods.  Three calls each, all three times kept (the last is the figure, the three give the spread), of
  the host form, the _dev form (device inputs and outputs, with a status), and
  the loop the call replaces, in the same process: per round bulkscan_cond(cond = the table so far, keep_on_device = True), .colmax()
  on the resident matrix and the table update on the host -- every trait in every round, as a user has to run it today.
Writes profiles/stepwise_time.json (or --out DIR) when --write is given.
Kernel times per round: `rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/stepwise_time.py --no-loop`, then
`python tools/stepwise_time.py --rounds DIR/.../*_kernel_trace.csv [--write]` cuts the trace into calls (each ends with k_step_finish) and
rounds (k_cond_null .. k_step_update), sums the device time of every kernel per round for the last _dev call of each method and adds
it to the JSON as "kernel_trace"."""
import csv
import ctypes as C
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

S, THR = 4, 4.0


def out_path():
    where = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles")
    return os.path.join(where, "stepwise_time.json")


def rounds_from_trace(path):
    """Per method (the order main() runs them in: three host calls, then three _dev calls each) the last _dev call's kernels: device
    ms per kernel in the front (before the first k_cond_null) and in every round, the launches per round, and the time from a round's
    first kernel start to its k_step_update's end."""
    with open(path, newline="") as f:
        rows = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(f)))
    calls, cur = [], []
    for t0, t1, name in rows:
        k = re.search(r"\bk_\w+", name)
        k = k.group(0) if k else re.split(r"[<(]", name)[0].split("::")[-1].strip()
        cur.append((t0, t1, k))
        if k == "k_step_finish":
            calls.append(cur); cur = []
    res = {}
    for method, idx in (("null-grid", 5), ("null-exact", 11)):
        if idx >= len(calls):
            continue
        parts, part = [], []
        for e in calls[idx]:
            if e[2] == "k_cond_null":                  # one per round
                parts.append(part); part = []
            part.append(e)
        parts.append(part)
        rec = {"call_span_ms": (calls[idx][-1][1] - calls[idx][0][0]) / 1e6, "parts": []}
        for i, part in enumerate(parts):
            ms, cnt = {}, {}
            for t0, t1, k in part:
                ms[k] = ms.get(k, 0.0) + (t1 - t0) / 1e6; cnt[k] = cnt.get(k, 0) + 1
            rec["parts"].append({"part": "front" if i == 0 else "round %d" % (i - 1), "span_ms": round((part[-1][1] - part[0][0]) / 1e6, 4),
                                 "device_ms": round(sum(ms.values()), 4), "kernels_ms": {k: round(v, 4) for k, v in ms.items()},
                                 "launches": cnt})
        res[method] = rec
    return res



def host_loop(b, Y, G, K, method):
    m = Y.shape[1]
    T = np.full((m, S), -1, dtype=np.int64)
    A = np.arange(m)
    active = []
    for t in range(S + 1):
        if A.size == 0:
            break
        active.append(int(A.size))
        r = b.bulkscan_cond(Y, G, K, T, method=method, keep_on_device=True)
        mx, arg = r["L"].colmax()
        if t == S:
            break
        sel = A[mx[A] > THR]
        T[sel, t] = arg[sel]
        A = sel
    return T, active


def main():
    if "--rounds" in sys.argv:
        res = rounds_from_trace(sys.argv[sys.argv.index("--rounds") + 1])
        print(json.dumps(res, indent=1))
        if "--write" in sys.argv:
            with open(out_path()) as f:
                out = json.load(f)
            out["kernel_trace"] = res
            with open(out_path(), "w") as f:
                json.dump(out, f, indent=1)
                f.write("\n")
        return
    import bulklmm_jl_amd as b
    from common import DevBuf, make_data
    n, p, m = 79, 7321, 35554
    Y, G, K = make_data(n=n, p=p, m=m, seed=20241)[:3]
    rng = np.random.default_rng(20242)
    second = np.arange(0, m, 10)
    Y[:, second] += 1.5 * G[:, rng.integers(0, p, size=second.size)]
    ctx = b.default_context()
    Lc = b._lib
    out = {"shape": [n, p, m], "max_loci": S, "threshold": THR, "planted": "make_data: 30 % of the traits one locus, N(0, 1.5^2); "
           "every tenth trait a second one of size 1.5", "methods": {}}
    dY, dG, dK = DevBuf(Y.T), DevBuf(G.T), DevBuf(K)
    douts = [DevBuf(nbytes=8 * m * S)] + [DevBuf(nbytes=8 * m * (S + 1)) for _ in range(3)] + [DevBuf(nbytes=8 * m), DevBuf(nbytes=64)]
    grid = np.arange(10) / 10.0
    for method in ("null-grid", "null-exact"):
        rec = {"host_ms": [], "dev_ms": [], "loop_ms": []}
        for _ in range(3):
            t0 = time.perf_counter()
            r = b.bulkscan_stepwise(Y, G, K, max_loci=S, threshold=THR, method=method, return_status=True)
            rec["host_ms"].append(1e3 * (time.perf_counter() - t0))
        rec["active"] = r["active"].tolist(); rec["rounds"] = r["rounds"]
        rec["nloci_counts"] = np.bincount(r["nloci"], minlength=S + 1).tolist()
        rec["n_rule_zero"] = r["n_rule_zero"]; rec["n_illcond_rescan"] = int(r["status"].n_illcond_rescan)
        o = b.api._opts(Lc.BLMM_NULL_EXACT if method == "null-exact" else Lc.BLMM_NULL_GRID)
        st = Lc.blmm_status()
        for _ in range(3):
            ctx.synchronize()
            t0 = time.perf_counter()
            rc = ctx.lib.blmm_bulkscan_stepwise_dev(ctx.h, C.byref(o), C.c_void_p(dY.ptr), n, m, C.c_void_p(dG.ptr), p, None, 0,
                                                    C.c_void_p(dK.ptr), None, grid.ctypes.data_as(C.c_void_p), 10, S, THR,
                                                    *[C.c_void_p(d.ptr) for d in douts], C.byref(st))
            rec["dev_ms"].append(1e3 * (time.perf_counter() - t0))
            assert rc == 0
        assert np.array_equal(douts[0].get((m, S), dtype=np.int64), r["loci"])
        if "--no-loop" not in sys.argv:
            for _ in range(3):
                t0 = time.perf_counter()
                T, active = host_loop(b, Y, G, K, method)
                rec["loop_ms"].append(1e3 * (time.perf_counter() - t0))
            assert np.array_equal(T, r["loci"]) and active == [a for a in rec["active"] if a > 0]
            rec["loop_over_host"] = rec["loop_ms"][-1] / rec["host_ms"][-1]
        out["methods"][method] = rec
        print(method, json.dumps(rec), flush=True)
    if "--write" in sys.argv:
        with open(out_path(), "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
