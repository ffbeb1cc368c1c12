"""Child program of tests/test_gpu_stepwise.py::test_torch_wrapper_in_its_own_process: bulkscan_stepwise_dev on torch tensors with a
caller stream (covariates, weights), for both methods equal to the host form; without a status the results are complete after
ctx.synchronize(); a pending -log10 p request is refused and consumed; no matrix is left resident.  Every output sits between guard
words that must stay intact."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bulklmm_jl_amd as blmm  # noqa: E402
from common import make_data  # noqa: E402

C = blmm.api.C
dev = torch.device("cuda", 0)
s = torch.cuda.Stream(device=dev)
ctx = blmm.Context(0, s.cuda_stream)
n, p, m, S, thr = 79, 150, 37, 3, 2.0
Y, G, K, Cov = make_data(n=n, p=p, m=m, seed=8800, ncov=2)
rng = np.random.default_rng(8801)
for j in range(12):                                     # two planted loci on the first twelve traits
    q = rng.choice(p, size=2, replace=False)
    Y[:, j] += 2.6 * G[:, q[0]] + 1.9 * G[:, q[1]]
w = np.random.default_rng(8802).uniform(0.5, 2.0, n)
GUARD_F, GUARD_I = -12345.5, -424242


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def guarded(shape, dtype):
    count = int(np.prod(shape))
    buf = torch.full((count + 2,), GUARD_F if dtype == torch.float64 else GUARD_I, dtype=dtype, device=dev)
    return buf, buf[1:count + 1].view(*shape)


def intact(*bufs):
    for b in bufs:
        h = b.cpu().numpy()
        g = GUARD_F if h.dtype == np.float64 else GUARD_I
        assert h[0] == g and h[-1] == g, "a guard word was overwritten"


dY, dG, dK, dC, dW = t(Y.T), t(G.T), t(K.T), t(Cov.T), t(w)
for method in ("null-grid", "null-exact"):
    host = blmm.bulkscan_stepwise(Y, G, K, Cov, max_loci=S, threshold=thr, method=method, weights=w, return_status=True, ctx=ctx)
    assert host["active"][1] > 0, method
    for status in (True, False):
        bl, loci = guarded((m, S), torch.int64); bo, lod = guarded((m, S + 1), torch.float64)
        ba, arg = guarded((m, S + 1), torch.int64); bh, h2 = guarded((m, S + 1), torch.float64)
        bn, nloci = guarded((m,), torch.int64); bi, info = guarded((8,), torch.int64)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            st = blmm.bulkscan_stepwise_dev(ctx, dY, dG, dK, loci, lod, arg, h2, nloci, threshold=thr, sinfo_out=info, method=method,
                                            Covar=dC, weights=dW, status=status)
            ctx.synchronize()
            got = {"loci": loci.cpu().numpy(), "lod": lod.cpu().numpy(), "argmax": arg.cpu().numpy(), "h2": h2.cpu().numpy(),
                   "nloci": nloci.cpu().numpy()}
            hi = info.cpu().numpy()
        for k in got:
            assert np.array_equal(got[k], host[k], equal_nan=True), (method, status, k)
        assert hi[0] == host["rounds"] and hi[1] == host["n_cond_traits"] and hi[2] == host["n_rule_zero"], (method, hi)
        assert hi[3:4 + S].tolist() == host["active"].tolist(), (method, hi)
        if status:
            assert st.n_nan_lod == host["status"].n_nan_lod and st.n_illcond_rescan == host["status"].n_illcond_rescan, method
        intact(bl, bo, ba, bh, bn, bi)
        pp, mm = C.c_int64(-1), C.c_int64(-1)
        assert ctx.lib.blmm_last_dims(ctx.h, C.byref(pp), C.byref(mm)) != 0, method     # no resident matrix
    # a pending -log10 p request: refused, consumed, nothing written
    bl, loci = guarded((m, S), torch.int64); bo, lod = guarded((m, S + 1), torch.float64)
    ba, arg = guarded((m, S + 1), torch.int64); bh, h2 = guarded((m, S + 1), torch.float64); bn, nloci = guarded((m,), torch.int64)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        assert ctx.lib.blmm_set_log10p_output(ctx.h, None, 0, 1) == 0
        try:
            blmm.bulkscan_stepwise_dev(ctx, dY, dG, dK, loci, lod, arg, h2, nloci, threshold=thr, method=method)
            raise SystemExit("the pending request was not refused")
        except blmm.BulkLMMError as e:
            assert e.code == -1 and "blmm_set_log10p_output request is pending" in e.msg, e.msg
        ctx.synchronize()
        assert (lod.cpu().numpy() == GUARD_F).all() and (loci.cpu().numpy() == GUARD_I).all(), method
        blmm.bulkscan_stepwise_dev(ctx, dY, dG, dK, loci, lod, arg, h2, nloci, threshold=thr, method=method, Covar=dC, weights=dW)
        ctx.synchronize()
        assert np.array_equal(loci.cpu().numpy(), host["loci"]), method                 # consumed: the next call runs
print("stepwise_dev ok")
