"""Child program of tests/test_gpu_effects.py::test_torch_wrapper_in_its_own_process: bulkscan_effects_dev on torch tensors
(covariates, weights, status) for both methods equals the host form bulkscan_effects bit for bit, and a test out of range gets
NaN / accepted = -1 and an error with the status."""
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
n, P, k, m, T = 79, 70, 3, 37, 500
Y, G, K, Cov = _founder_data(n, P, k, m, seed=5600, ncov=2)
rng = np.random.default_rng(5601)
w = rng.uniform(0.5, 2.0, n)
locus, trait = rng.integers(0, P, T), rng.integers(0, m, T)


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def run(method, loc, status):
    out = dict(beta=torch.empty((T, k), dtype=torch.float64, device=dev), se=torch.empty((T, k), dtype=torch.float64, device=dev),
               sigma2=torch.empty(T, dtype=torch.float64, device=dev), lod=torch.empty(T, dtype=torch.float64, device=dev),
               accepted=torch.empty(T, dtype=torch.int32, device=dev), h2_null_list=torch.empty(m, dtype=torch.float64, device=dev))
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        try:
            st = blmm.bulkscan_effects_dev(ctx, dY, dG, dK, k, t(loc), dT, out["beta"], out["se"], out["sigma2"], out["lod"],
                                           out["accepted"], out["h2_null_list"], method=method, Covar=dC, weights=dW, status=status)
        except blmm.BulkLMMError as e:
            st = e
        s.synchronize()
        return st, {f: v.cpu().numpy() for f, v in out.items()}


dY, dG, dK, dC, dW, dT = t(Y.T), t(G.T), t(K.T), t(Cov.T), t(w), t(trait)
for method in ("null-grid", "null-exact"):
    host = blmm.bulkscan_effects(Y, G, K, Cov, k=k, locus=locus, trait=trait, method=method, weights=w, ctx=ctx)
    st, got = run(method, locus, True)
    assert not isinstance(st, Exception) and st.n_nan_lod == 0, (method, st)
    for f in got:
        assert np.array_equal(got[f], host[f]), (method, f)
    bad = locus.copy()
    bad[11], bad[400] = P, -1
    st, got = run(method, bad, True)
    assert isinstance(st, blmm.BulkLMMError) and st.code == -1 and "2 test(s)" in st.msg, (method, st)
    ok = np.ones(T, bool)
    ok[[11, 400]] = False
    for f in ("beta", "se", "sigma2", "lod"):
        assert np.isnan(got[f][~ok]).all() and np.array_equal(got[f][ok], host[f][ok]), (method, f)
    assert np.all(got["accepted"][~ok] == -1) and np.array_equal(got["accepted"][ok], host["accepted"][ok]), method
print("effects_dev ok")
