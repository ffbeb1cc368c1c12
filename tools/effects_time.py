"""Times bulkscan_effects at the BXD shape (n = 79, P = 7321 loci, m = 35554 traits), null-exact, k = 1 and k = 8, for (a) T = m
tests, one per trait (every trait's peak) and (b) T = 10^6 random tests.  Prints, for the last of three calls: the wall time, the
phases of blmm_set_timing (eigen, rotate, h2 = the null-model phases bulkscan_reduced spends before its scan; prep = marker rotation,
transposition and the sort of the tests; scan = k_effects) and the time the bytes the kernel must read, T k n 8, would take at the
measured HBM rate of 6.29 TB/s.  Kernel times: `rocprofv3 --kernel-trace --stats -- python tools/effects_time.py` (k_effects,
k_eff_hist, k_eff_scan, k_eff_scatter, k_untranspose)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bulklmm_jl_amd as b  # noqa: E402
from common import bxd_kinship  # noqa: E402

HBM = 6.29e12


def main():
    rng = np.random.default_rng(1)
    n, P, m = 79, 7321, 35554
    K = bxd_kinship()
    Y = rng.standard_normal((n, m)) + 3.0
    ctx = b.default_context()
    ctx.set_timing(True)
    for k in (1, 8):
        G = rng.dirichlet(np.full(k + 1, 0.7), size=(n, P))[:, :, :k].reshape(n, P * k)
        for what, T in (("one test per trait", m), ("random tests", 1000000)):
            trait = np.arange(m) if T == m else rng.integers(0, m, T)
            locus = rng.integers(0, P, T)
            for _ in range(3):
                t0 = time.perf_counter()
                r = b.bulkscan_effects(Y, G, K, k=k, locus=locus, trait=trait, method="null-exact", return_status=True)
                t1 = time.perf_counter()
            st = r["status"]
            print(f"k={k} T={T} ({what}): call {1e3 * (t1 - t0):.1f} ms; eigen {st.t_eigen_ms:.3f} rotate {st.t_rotate_ms:.3f} "
                  f"h2 {st.t_h2_ms:.3f} prep {st.t_prep_ms:.3f} effects {st.t_scan_ms:.3f} ms; byte bound "
                  f"{1e3 * T * k * n * 8 / HBM:.3f} ms", flush=True)


if __name__ == "__main__":
    main()
