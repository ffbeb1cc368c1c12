"""Child program of tests/test_gpu_reduced_async.py::test_torch_binding_in_its_own_process: bulkscan_reduced_async on torch
tensors, enqueued on a torch stream with no synchronisation in between, against bulkscan_reduced_dev; reduced_info decodes the
info block."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bulklmm_jl_amd as blmm  # noqa: E402
from common import make_data  # noqa: E402

dev = torch.device("cuda", 0)
s = torch.cuda.Stream(device=dev)
ctx = blmm.Context(0, s.cuda_stream)
_, G, K, Cov = make_data(p=700, m=500, seed=5700, ncov=2)
dG = torch.from_numpy(np.ascontiguousarray(G.T)).to(dev)
dK = torch.from_numpy(np.ascontiguousarray(K.T)).to(dev)
dC = torch.from_numpy(np.ascontiguousarray(Cov.T)).to(dev)
m, cap = 500, 1 << 15


def outs():
    return dict(max_out=torch.empty(m, dtype=torch.float64, device=dev), argmax_out=torch.empty(m, dtype=torch.int64, device=dev),
                h2_out=torch.empty(m, dtype=torch.float64, device=dev), trip_i=torch.empty(cap, dtype=torch.int32, device=dev),
                trip_j=torch.empty(cap, dtype=torch.int32, device=dev), trip_lod=torch.empty(cap, dtype=torch.float64, device=dev),
                trip_count=torch.zeros(1, dtype=torch.int64, device=dev))


Ys = [torch.from_numpy(np.ascontiguousarray(make_data(p=700, m=500, seed=5701 + k, ncov=2)[0].T)).to(dev) for k in range(3)]
got = []
torch.cuda.synchronize()
with torch.cuda.stream(s):
    for dY in Ys:                                     # enqueued back to back on torch's stream
        o = outs()
        info = torch.full((9,), -1, dtype=torch.int64, device=dev)
        blmm.bulkscan_reduced_async(ctx, dY, dG, dK, o["max_out"], o["argmax_out"], o["h2_out"], info, Covar=dC, threshold=3.0,
                                    trip_i=o["trip_i"], trip_j=o["trip_j"], trip_lod=o["trip_lod"], trip_count=o["trip_count"])
        got.append((o, info))
    host = [(o["max_out"].cpu(), o["argmax_out"].cpu(), o["trip_count"].cpu(), info.cpu()) for o, info in got]   # torch's stream, after
for (o, _), dY, (mx, ax, cnt, info) in zip(got, Ys, host):
    r = outs()
    blmm.bulkscan_reduced_dev(ctx, dY, dG, dK, r["max_out"], r["argmax_out"], r["h2_out"], Covar=dC, threshold=3.0,
                              trip_i=r["trip_i"], trip_j=r["trip_j"], trip_lod=r["trip_lod"], trip_count=r["trip_count"])
    assert torch.equal(mx, r["max_out"].cpu()) and torch.equal(ax, r["argmax_out"].cpu()) and torch.equal(o["h2_out"], r["h2_out"])
    k = int(r["trip_count"].item())
    assert int(cnt.item()) == k > 0
    a = sorted(zip(o["trip_j"][:k].tolist(), o["trip_i"][:k].tolist(), o["trip_lod"][:k].tolist()))
    b = sorted(zip(r["trip_j"][:k].tolist(), r["trip_i"][:k].tolist(), r["trip_lod"][:k].tolist()))
    assert a == b
    d = blmm.reduced_info(info.numpy())
    assert d["route"] in (1, 3) and d["triplets"] == k and d["device_error"] == 0, d
print("reduced_async ok")
