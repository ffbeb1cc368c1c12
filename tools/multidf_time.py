"""Times bulkscan_multidf at the BXD shape (n = 79, P = 7321 loci, m = 35554 traits): null-grid k = 2 and 8, null-exact k = 2, L kept
on the device.  Prints the wall time of the last of three calls and its scan phase (blmm_set_timing).  Kernel times: run it under
`rocprofv3 --kernel-trace --stats -- python tools/multidf_time.py` (k_mdf_table, k_mdf_grid, k_mdf_exact)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bulklmm_jl_amd as b  # noqa: E402
from common import bxd_kinship  # noqa: E402


def main():
    rng = np.random.default_rng(1)
    n, P, m = 79, 7321, 35554
    K = bxd_kinship()
    Y = rng.standard_normal((n, m)) + 3.0
    ctx = b.default_context()
    ctx.set_timing(True)
    for method, k in (("null-grid", 2), ("null-grid", 8), ("null-exact", 2)):
        G = rng.dirichlet(np.full(k + 1, 0.7), size=(n, P))[:, :, :k].reshape(n, P * k)
        for _ in range(3):
            t0 = time.perf_counter()
            r = b.bulkscan_multidf(Y, G, K, k, method=method, keep_on_device=True, return_status=True)
            ctx.synchronize()
            t1 = time.perf_counter()
        print(f"{method} k={k}: call {1e3 * (t1 - t0):.1f} ms; scan phase {r['status'].t_scan_ms:.3f} ms", flush=True)


if __name__ == "__main__":
    main()
