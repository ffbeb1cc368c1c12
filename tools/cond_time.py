"""Times bulkscan_cond at the BXD shape (n = 79, p = 7321, m = 35554, BXD kinship), every trait conditioned on its own peak, both
methods: wall time of the last of three calls with L kept on the device, the phases of blmm_set_timing, and the achieved rate of
the scan kernel against the fp64 matrix peak (2 n (2 + c + s) p m flop).  In the same run, the loop the call replaces: traits
grouped by conditioning marker, one bulkscan(Y[:, group], G, K, Covar=g_q) per distinct marker (D of them).  Writes
profiles/cond_time.json when --write is given.  Kernel times: `rocprofv3 --kernel-trace --stats -- python tools/cond_time.py --no-loop`
(k_cond_null, k_cond_panels, k_scan<.., COND>)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bulklmm_jl_amd as b  # noqa: E402
from common import make_data  # noqa: E402

PEAK_TF = 78.6


def main():
    n, p, m = 79, 7321, 35554
    Y, G, K = make_data(n=n, p=p, m=m, seed=20241)[:3]
    ctx = b.default_context()
    ctx.set_timing(True)
    out = {"shape": [n, p, m], "peak_tflops": PEAK_TF, "methods": {}}
    for method in ("null-grid", "null-exact"):
        peaks = b.bulkscan_reduced(Y, G, K, method=method)["argmax"]
        for _ in range(3):
            ctx.read_timings()
            t0 = time.perf_counter()
            r = b.bulkscan_cond(Y, G, K, peaks, method=method, keep_on_device=True, return_status=True)
            ctx.synchronize()
            t1 = time.perf_counter()
        ph, _ = ctx.read_timings()
        flop = 2.0 * n * (2 + 1 + 1) * p * m
        rec = {"call_ms": 1e3 * (t1 - t0), "phases_ms": ph, "scan_phase_tflops": flop / (ph["scan"] * 1e-3) / 1e12,
               "scan_phase_share_of_peak": flop / (ph["scan"] * 1e-3) / 1e12 / PEAK_TF, "n_rule_zero": r["n_rule_zero"],
               "n_illcond_rescan": int(r["status"].n_illcond_rescan)}
        if "--no-loop" not in sys.argv:
            order = np.argsort(peaks, kind="stable")
            marks, starts = np.unique(peaks[order], return_index=True)
            t0 = time.perf_counter()
            for q, lo, hi in zip(marks, starts, list(starts[1:]) + [m]):
                b.bulkscan(np.asfortranarray(Y[:, order[lo:hi]]), G, K, G[:, [q]], method=method)
            ctx.synchronize()
            rec["loop_ms"] = 1e3 * (time.perf_counter() - t0)
            rec["loop_distinct_markers"] = int(marks.size)
            rec["loop_over_call"] = rec["loop_ms"] / rec["call_ms"]
        out["methods"][method] = rec
        print(method, json.dumps(rec), flush=True)
    if "--write" in sys.argv:
        with open(os.path.join(ROOT, "profiles", "cond_time.json"), "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
