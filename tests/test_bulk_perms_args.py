"""CPU checks of bulkscan_perms (the permutation test for every trait): the argument errors are raised by the host mirror before
a context exists (no GPU needed), and the entry point is exported at every layer."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _no_context(blmm):
    return blmm.api._default_ctx is None


def test_bulkscan_perms_is_exported(blmm):
    assert "bulkscan_perms" in blmm.__all__ and "bulkscan_perms_dev" in blmm.__all__
    assert callable(blmm.bulkscan_perms) and callable(blmm.bulkscan_perms_dev)
    lib = blmm.load()
    for sym in ("blmm_bulkscan_perms", "blmm_bulkscan_perms_dev"):
        assert sym in blmm.EXPORTS and hasattr(lib, sym)
    jl = open(os.path.join(ROOT, "bulklmm.jl_amd", "julia", "BulkLMMHIP.jl")).read()
    assert re.search(r"ccall\(\(:blmm_bulkscan_perms, libblmm\)", jl)
    assert re.search(r"^export .*\bbulkscan_perms\b", jl, flags=re.M)


def test_negative_nperms_is_refused(blmm):
    Y = np.zeros((6, 2)); G = np.zeros((6, 3)); K = np.eye(6)
    before = _no_context(blmm)
    with pytest.raises(blmm.BulkLMMError) as e:
        blmm.bulkscan_perms(Y, G, K, nperms=-1)
    assert e.value.code == -9 and e.value.msg == "The required number of permutations must be a positive integer."
    assert _no_context(blmm) == before


@pytest.mark.parametrize("case", ["G_rows", "K_rows", "K_cols", "Covar_rows", "weights_len", "perm_idx_shape", "perm_idx_rows"])
def test_shape_mismatches_are_refused(blmm, case):
    n = 6
    Y = np.zeros((n, 2)); G = np.zeros((n, 3)); K = np.eye(n)
    kw = {"nperms": 4}
    if case == "G_rows":
        G = np.zeros((n + 1, 3))
    elif case == "K_rows":
        K = np.eye(n + 1)[:, :n]
    elif case == "K_cols":
        K = np.eye(n + 1)[:n, :]
    elif case == "Covar_rows":
        kw["Covar"] = np.zeros((n - 1, 1))
    elif case == "weights_len":
        kw["weights"] = np.ones(n + 2)
    elif case == "perm_idx_shape":
        kw["perm_idx"] = np.zeros((n, 3), dtype=np.int32)      # nperms = 4 columns expected
    elif case == "perm_idx_rows":
        kw["perm_idx"] = np.zeros((n - 1, 4), dtype=np.int32)
    before = _no_context(blmm)
    with pytest.raises(blmm.BulkLMMError) as e:
        blmm.bulkscan_perms(Y, G, K, **kw)
    assert e.value.code == -2 and e.value.msg == "Dimension mismatch."
    assert _no_context(blmm) == before


def test_more_than_2048_individuals_is_refused_before_a_context(blmm):
    n = 2049
    Y = np.zeros((n, 1)); G = np.zeros((n, 2)); K = np.eye(n)
    before = _no_context(blmm)
    with pytest.raises(blmm.BulkLMMError) as e:
        blmm.bulkscan_perms(Y, G, K, nperms=2)
    assert e.value.code == -10 and "2048" in e.value.msg
    assert _no_context(blmm) == before
