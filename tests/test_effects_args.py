"""bulkscan_effects without a GPU: every refusal of the host mirror (code and message, before a context exists), the agreement of
the header, the Julia binding and the Python mirror on the entry points' signatures, and the condition that keeps the GPU tests'
tolerance honest: on every input set they use, the oracle's two solves (wls by QR and by Cholesky) agree on beta to 1e-9."""
import ctypes as C
import os
import re
import warnings

import numpy as np
import pytest

from effects_cases import GRID, all_cases
from effects_ref import effects_ref
from oracle import bulklmm_oracle as O
from test_binding_abi import ALLOWED, c_prototypes, julia_ccalls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _no_context(blmm):
    return blmm.api._default_ctx is None


def _refused(blmm, code, msg, *args, **kw):
    before = _no_context(blmm)
    with pytest.raises(blmm.BulkLMMError) as e:
        blmm.bulkscan_effects(*args, **kw)
    assert e.value.code == code, (e.value.code, e.value.msg)
    assert msg in e.value.msg, e.value.msg
    assert _no_context(blmm) == before


def _zeros(n=6, m=2, p=4):
    return np.zeros((n, m)), np.zeros((n, p)), np.eye(n)


@pytest.mark.parametrize("k,p", [(0, 6), (-1, 6), (4, 6), (5, 12)])
def test_p_not_a_multiple_of_k_is_refused(blmm, k, p):
    Y, G, K = _zeros(p=p)
    _refused(blmm, -2, "multiple of k", Y, G, K, k=k, locus=[0], trait=[0])


@pytest.mark.parametrize("method", ["null-grid", "null-exact"])
def test_k_above_eight_is_refused(blmm, method):
    Y, G, K = _zeros(n=12, p=18)
    _refused(blmm, -10, "takes 1 <= k <= 8", Y, G, K, k=9, locus=[0], trait=[0], method=method)


def test_alt_grid_and_unknown_methods_are_refused(blmm):
    Y, G, K = _zeros()
    _refused(blmm, -10, "alt-grid is not supported", Y, G, K, k=2, locus=[0], trait=[0], method="alt-grid")
    _refused(blmm, -5, "Unknown method", Y, G, K, k=2, locus=[0], trait=[0], method="grid")


def test_more_than_eight_covariates_are_refused(blmm):
    Y, G, K = _zeros(n=20)
    _refused(blmm, -10, "more than 8 null covariates", Y, G, K, np.zeros((20, 8)), k=1, locus=[0], trait=[0])
    _refused(blmm, -10, "more than 8 null covariates", Y, G, K, np.zeros((20, 9)), k=1, locus=[0], trait=[0], addIntercept=False)


def test_more_than_2048_individuals_is_refused(blmm):
    Y, G, K = _zeros(n=2049, m=1, p=2)
    _refused(blmm, -10, "2048", Y, G, K, k=2, locus=[0], trait=[0])


@pytest.mark.parametrize("locus,trait", [([2], [0]), ([-1], [0]), ([0], [2]), ([0], [-1]), ([0, 1, 0], [0, 1, 5])])
def test_an_index_out_of_range_is_refused(blmm, locus, trait):
    Y, G, K = _zeros()                                                   # k = 2: two loci, two traits
    _refused(blmm, -1, "out of range", Y, G, K, k=2, locus=locus, trait=trait)


def test_mismatched_lists_are_refused(blmm):
    Y, G, K = _zeros()
    _refused(blmm, -1, "same length", Y, G, K, k=2, locus=[0, 1], trait=[0])
    _refused(blmm, -1, "both locus and trait", Y, G, K, k=2, locus=[0])
    _refused(blmm, -1, "required for k > 1", Y, G, K, k=2)


def test_shape_mismatches_are_refused(blmm):
    Y, G, K = _zeros()
    _refused(blmm, -2, "Dimension mismatch", Y, np.zeros((7, 4)), K, k=1, locus=[0], trait=[0])
    _refused(blmm, -2, "Dimension mismatch", Y, G, K, np.zeros((5, 1)), k=1, locus=[0], trait=[0])
    _refused(blmm, -2, "Dimension mismatch", Y, G, K, k=1, locus=[0], trait=[0], weights=np.ones(7))


# ---- one signature in the header, the Julia binding and the Python mirror -------------------------------------------------------
CT = {"const double*": C.c_void_p, "double*": C.c_void_p, "const int64_t*": C.c_void_p, "int32_t*": C.c_void_p, "int64_t": C.c_int64,
      "blmm_ctx*": C.c_void_p}


def test_header_julia_and_python_agree(blmm):
    protos = c_prototypes()
    host, dev = protos["blmm_bulkscan_effects"], protos["blmm_bulkscan_effects_dev"]
    assert host == dev and host[0] == "int" and len(host[1]) == 24
    assert host[1][14:17] == ["const int64_t*", "const int64_t*", "int64_t"] and host[1][21] == "int32_t*"
    lib = blmm.load()
    for sym in ("blmm_bulkscan_effects", "blmm_bulkscan_effects_dev"):
        assert sym in blmm.EXPORTS
        at = getattr(lib, sym).argtypes
        assert len(at) == 24
        for i, (a, ct) in enumerate(zip(at, host[1])):
            if ct in CT:
                assert a is CT[ct], (sym, i, ct, a)
    calls = [c for c in julia_ccalls() if c[0] == "blmm_bulkscan_effects"]
    assert len(calls) == 1
    _, ret, types, nvals = calls[0]
    assert ret == "Cint" and nvals == len(types) == 24
    for jt, ct in zip(types, host[1]):
        assert jt in ALLOWED[ct], (jt, ct)
    jl = open(os.path.join(ROOT, "bulklmm.jl_amd", "julia", "BulkLMMHIP.jl")).read()
    assert re.search(r"^export .*\bbulkscan_effects\b", jl, flags=re.M)
    hdr = open(os.path.join(ROOT, "include", "bulklmm_hip.h")).read()
    assert re.search(r"#define BLMM_EFFECTS_MAX_K 8\b", hdr) and blmm._lib.BLMM_EFFECTS_MAX_K == 8
    assert "bulkscan_effects" in blmm.__all__ and "bulkscan_effects_dev" in blmm.__all__


# ---- the oracle's own condition ---------------------------------------------------------------------------------------------------
CASES = dict(all_cases())


@pytest.mark.parametrize("name", list(CASES))
def test_the_two_cpu_solves_agree_on_every_gpu_input(name):
    c = CASES[name]()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        G1 = c["G"][:, :1]                                               # the null model does not involve G
        if c["method"] == "null-exact":
            h2 = O.bulkscan_null(c["Y"], G1, c["K"], c["Cov"], **c["kw"]).h2_null_list
        else:
            h2 = O.bulkscan_null_grid(c["Y"], G1, c["K"], GRID, c["Cov"], **c["kw"]).h2_null_list
        args = (c["Y"], c["G"], c["K"], c["k"], c["locus"], c["trait"], h2)
        qr = effects_ref(*args, Covar=c["Cov"], **c["kw"])
        ch = effects_ref(*args, Covar=c["Cov"], method="cholesky", **c["kw"])
    scale = np.abs(qr.beta).max()
    assert scale > 0 and np.isfinite(qr.beta).all() and np.isfinite(qr.se).all()
    rel = np.abs(qr.beta - ch.beta).max() / scale
    print(f"{name}: QR against Cholesky, max |d beta| / max |beta| = {rel:.3e}")
    assert rel <= 1e-9
    np.testing.assert_array_equal(qr.accepted, ch.accepted)
