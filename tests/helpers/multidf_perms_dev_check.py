"""Child program of tests/test_gpu_multidf_perms.py::test_dev_form_in_its_own_process: bulkscan_multidf_perms_dev on torch tensors
(covariates, weights, explicit permutations and the library's generator, status) on the context's stream, bit-equal to the host
form bulkscan_multidf_perms."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bulklmm_jl_amd as blmm  # noqa: E402
from oracle import bulklmm_oracle as O  # noqa: E402
from test_gpu_multidf import _founder_data  # noqa: E402

dev = torch.device("cuda", 0)
s = torch.cuda.Stream(device=dev)
ctx = blmm.Context(0, s.cuda_stream)
n, P, k, m, nperms = 79, 70, 3, 11, 19
SIG = (0.2, 0.1, 0.05)
Y, G, K, Cov = _founder_data(n, P, k, m, seed=7700, ncov=2)
w = np.random.default_rng(7701).uniform(0.5, 2.0, n)
pidx = O.make_perm_idx(n, nperms, 7702)


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


dY, dG, dK, dC, dW, dP = t(Y.T), t(G.T), t(K.T), t(Cov.T), t(w), t(pidx.T)
for explicit in (True, False):
    host = blmm.bulkscan_multidf_perms(Y, G, K, k, Cov, nperms=nperms, rndseed=5, perm_idx=pidx if explicit else None,
                                       signif_level=SIG, weights=w, reml=True, ctx=ctx, return_status=True)
    f64 = dict(dtype=torch.float64, device=dev)
    h2, s2, mx, pv = (torch.full((m,), float("nan"), **f64) for _ in range(4))
    arg = torch.full((m,), -7, dtype=torch.int64, device=dev)
    mp = torch.full((m, nperms), float("nan"), **f64)
    thr = torch.full((m, len(SIG)), float("nan"), **f64)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        st = blmm.bulkscan_multidf_perms_dev(ctx, dY, dG, dK, k, h2, s2, mx, arg, mp, thr, pv, nperms=nperms, seed=5,
                                             perm_idx=dP if explicit else None, signif_level=SIG, Covar=dC, weights=dW, reml=True,
                                             status=True)
        got = {"h2_null": h2.cpu().numpy(), "sigma2_e": s2.cpu().numpy(), "lod_max": mx.cpu().numpy(), "lod_argmax": arg.cpu().numpy(),
               "max_perms": mp.cpu().numpy().T, "thresholds": thr.cpu().numpy().T, "pvals_perm": pv.cpu().numpy()}
    assert st.n_nan_lod == host["status"].n_nan_lod == 0, explicit
    for key, val in got.items():
        assert np.array_equal(val, host[key]), (explicit, key)
    assert np.isfinite(got["max_perms"]).all() and (got["lod_argmax"] >= 0).all()
print("multidf_perms_dev ok")
