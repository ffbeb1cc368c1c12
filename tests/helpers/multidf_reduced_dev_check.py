"""Child program of tests/test_gpu_multidf_reduced.py::test_torch_wrapper_in_its_own_process: bulkscan_multidf_reduced_dev on torch
tensors (covariates, weights, status) for both methods, equal to the consumers on the matrix the host form bulkscan_multidf writes.
Every output sits between guard words that must stay intact; colmax = NULL with triplets only, and triplets off with maxima only."""
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
n, P, k, m = 79, 70, 2, 37
Y, G, K, Cov = _founder_data(n, P, k, m, seed=5600, ncov=2)
w = np.random.default_rng(5601).uniform(0.5, 2.0, n)
GUARD_F, GUARD_I = -12345.5, -424242


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def guarded(count, dtype):
    """count elements between two guard words: (whole buffer, the view handed to the library)"""
    buf = torch.full((count + 2,), GUARD_F if dtype == torch.float64 else GUARD_I, dtype=dtype, device=dev)
    return buf, buf[1:count + 1]


def intact(*bufs):
    for b in bufs:
        h = b.cpu().numpy()
        g = GUARD_F if h.dtype == np.float64 else GUARD_I
        assert h[0] == g and h[-1] == g, "a guard word was overwritten"


dY, dG, dK, dC, dW = t(Y.T), t(G.T), t(K.T), t(Cov.T), t(w)
for method in ("null-grid", "null-exact"):
    host = blmm.bulkscan_multidf(Y, G, K, k, Cov, method=method, weights=w, return_status=True, ctx=ctx)
    L = host["L"]
    emx, earg = blmm.lod_colmax(L, ctx=ctx)
    thr = float(np.quantile(L, 0.9))
    ei, ej, el = blmm.lod_threshold(L, thr, ctx=ctx)
    cap = len(ei) + 5
    kw = dict(method=method, Covar=dC, weights=dW, status=True)
    # maxima and triplets
    bmx, mx = guarded(m, torch.float64); barg, arg = guarded(m, torch.int64); bh2, h2 = guarded(m, torch.float64)
    bti, ti = guarded(cap, torch.int32); btj, tj = guarded(cap, torch.int32); btl, tl = guarded(cap, torch.float64)
    bcnt, cnt = guarded(1, torch.int64)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        st = blmm.bulkscan_multidf_reduced_dev(ctx, dY, dG, dK, k, mx, arg, h2, threshold=thr, trip_i=ti, trip_j=tj, trip_lod=tl,
                                               trip_count=cnt, **kw)
        c = int(cnt.cpu().numpy()[0])
        hti, htj, htl = ti.cpu().numpy()[:c], tj.cpu().numpy()[:c], tl.cpu().numpy()[:c]
        hmx, harg, hh2 = mx.cpu().numpy(), arg.cpu().numpy(), h2.cpu().numpy()
    assert st.n_nan_lod == host["status"].n_nan_lod == 0 and st.n_illcond_rescan == host["status"].n_illcond_rescan, method
    assert np.array_equal(hmx, emx) and np.array_equal(harg, earg) and np.array_equal(hh2, host["h2_null_list"]), method
    order = np.lexsort((hti, htj))
    assert c == len(ei) and np.array_equal(hti[order], ei) and np.array_equal(htj[order], ej) and np.array_equal(htl[order], el), method
    assert (ti.cpu().numpy()[c:] == GUARD_I).all() and (tl.cpu().numpy()[c:] == GUARD_F).all(), method     # nothing beyond count
    intact(bmx, barg, bh2, bti, btj, btl, bcnt)
    # colmax = NULL: triplets only
    bh2, h2 = guarded(m, torch.float64)
    bti, ti = guarded(cap, torch.int32); btj, tj = guarded(cap, torch.int32); btl, tl = guarded(cap, torch.float64)
    bcnt, cnt = guarded(1, torch.int64)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        blmm.bulkscan_multidf_reduced_dev(ctx, dY, dG, dK, k, None, None, h2, threshold=thr, trip_i=ti, trip_j=tj, trip_lod=tl,
                                          trip_count=cnt, **kw)
        c = int(cnt.cpu().numpy()[0])
        hti, htj, htl = ti.cpu().numpy()[:c], tj.cpu().numpy()[:c], tl.cpu().numpy()[:c]
    order = np.lexsort((hti, htj))
    assert c == len(ei) and np.array_equal(hti[order], ei) and np.array_equal(htj[order], ej) and np.array_equal(htl[order], el), method
    assert np.array_equal(h2.cpu().numpy(), host["h2_null_list"]), method
    intact(bh2, bti, btj, btl, bcnt)
    # triplets off: maxima only
    bmx, mx = guarded(m, torch.float64); barg, arg = guarded(m, torch.int64); bh2, h2 = guarded(m, torch.float64)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        blmm.bulkscan_multidf_reduced_dev(ctx, dY, dG, dK, k, mx, arg, h2, **kw)
        hmx, harg = mx.cpu().numpy(), arg.cpu().numpy()
    assert np.array_equal(hmx, emx) and np.array_equal(harg, earg), method
    intact(bmx, barg, bh2)
    pp, mm = blmm.api.C.c_int64(-1), blmm.api.C.c_int64(-1)
    assert ctx.lib.blmm_last_dims(ctx.h, blmm.api.C.byref(pp), blmm.api.C.byref(mm)) != 0, method     # no resident matrix
print("multidf_reduced_dev ok")
