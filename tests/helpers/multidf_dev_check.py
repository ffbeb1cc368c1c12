"""Child program of tests/test_gpu_multidf_edges.py::test_torch_wrapper_in_its_own_process: bulkscan_multidf_dev on torch tensors
(covariates, weights, a padded L_out and log10p_out, status) for both methods, equal to the host form bulkscan_multidf."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bulklmm_jl_amd as blmm  # noqa: E402
from test_gpu_multidf import _founder_data  # noqa: E402

dev = torch.device("cuda", 0)
s = torch.cuda.Stream(device=dev)
ctx = blmm.Context(0, s.cuda_stream)
n, P, k, m, pad = 79, 70, 3, 37, 4
Y, G, K, Cov = _founder_data(n, P, k, m, seed=5500, ncov=2)
w = np.random.default_rng(5501).uniform(0.5, 2.0, n)


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


dY, dG, dK, dC, dW = t(Y.T), t(G.T), t(K.T), t(Cov.T), t(w)
for method in ("null-grid", "null-exact"):
    host = blmm.bulkscan_multidf(Y, G, K, k, Cov, method=method, weights=w, output_pvals=True, return_status=True, ctx=ctx)
    Lbuf = torch.full((m, P + pad), float("nan"), dtype=torch.float64, device=dev)
    Pbuf = torch.full((m, P + pad), float("nan"), dtype=torch.float64, device=dev)
    h2 = torch.empty(m, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        st = blmm.bulkscan_multidf_dev(ctx, dY, dG, dK, k, Lbuf[:, :P], h2, method=method, Covar=dC, weights=dW, status=True,
                                       log10p_out=Pbuf[:, :P])
        Lh, Ph, hh = Lbuf.cpu().numpy(), Pbuf.cpu().numpy(), h2.cpu().numpy()
    assert st.n_nan_lod == host["status"].n_nan_lod == 0, method
    assert np.array_equal(hh, host["h2_null_list"]), method
    assert np.array_equal(Lh[:, :P].T, host["L"]), (method, float(np.max(np.abs(Lh[:, :P].T - host["L"]))))
    assert np.array_equal(Ph[:, :P].T, host["log10Pvals_mat"]), method
    assert np.isnan(Lh[:, P:]).all() and np.isnan(Ph[:, P:]).all(), method     # the padding is not written
print("multidf_dev ok")
