"""bulkscan_multidf_reduced without a GPU: the entry points are exported at every layer, and every refusal of bulkscan_multidf
(tests/test_multidf_args.py) comes back through the new call with the same code and message, before a context exists."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _no_context(blmm):
    return blmm.api._default_ctx is None


def test_bulkscan_multidf_reduced_is_exported(blmm):
    assert "bulkscan_multidf_reduced" in blmm.__all__ and "bulkscan_multidf_reduced_dev" in blmm.__all__
    assert callable(blmm.bulkscan_multidf_reduced) and callable(blmm.bulkscan_multidf_reduced_dev)
    lib = blmm.load()
    for sym in ("blmm_bulkscan_multidf_reduced", "blmm_bulkscan_multidf_reduced_dev"):
        assert sym in blmm.EXPORTS and hasattr(lib, sym)
    hdr = open(os.path.join(ROOT, "include", "bulklmm_hip.h")).read()
    assert re.search(r"^int blmm_bulkscan_multidf_reduced\(", hdr, flags=re.M)
    assert re.search(r"^int blmm_bulkscan_multidf_reduced_dev\(", hdr, flags=re.M)
    assert re.search(r"#define BLMM_VERSION 210\b", hdr)                      # appended to the comment only
    jl = open(os.path.join(ROOT, "bulklmm.jl_amd", "julia", "BulkLMMHIP.jl")).read()
    assert re.search(r"ccall\(\(:blmm_bulkscan_multidf_reduced, libblmm\)", jl)
    assert re.search(r"ccall\(\(:blmm_bulkscan_multidf_reduced_dev, libblmm\)", jl)
    assert re.search(r"^export .*\bbulkscan_multidf_reduced\b", jl, flags=re.M)


def test_the_new_tuning_key_is_documented():
    hdr = open(os.path.join(ROOT, "include", "bulklmm_hip.h")).read()
    assert '"mdf_red_chunk"' in hdr


def _refused(blmm, code, msg, *args, **kw):
    before = _no_context(blmm)
    with pytest.raises(blmm.BulkLMMError) as e:
        blmm.bulkscan_multidf_reduced(*args, **kw)
    assert e.value.code == code, (e.value.code, e.value.msg)
    assert msg in e.value.msg, e.value.msg
    assert _no_context(blmm) == before


@pytest.mark.parametrize("k,p", [(0, 6), (-1, 6), (4, 6), (5, 12)])
def test_p_not_a_multiple_of_k_is_refused(blmm, k, p):
    _refused(blmm, -2, "multiple of k", np.zeros((6, 2)), np.zeros((6, p)), np.eye(6), k)


@pytest.mark.parametrize("method,k", [("null-grid", 9), ("null-exact", 5), ("null-exact", 8)])
def test_k_above_the_method_limit_is_refused(blmm, method, k):
    _refused(blmm, -10, "takes 1 <= k <= %d" % (8 if method == "null-grid" else 4), np.zeros((12, 2)), np.zeros((12, 2 * k)),
             np.eye(12), k, method=method)


def test_alt_grid_and_unknown_methods_are_refused(blmm):
    _refused(blmm, -10, "alt-grid is not supported", np.zeros((6, 2)), np.zeros((6, 4)), np.eye(6), 2, method="alt-grid")
    _refused(blmm, -5, "Unknown method", np.zeros((6, 2)), np.zeros((6, 4)), np.eye(6), 2, method="grid")


def test_more_than_eight_covariates_are_refused(blmm):
    n = 20
    _refused(blmm, -10, "more than 8 null covariates", np.zeros((n, 2)), np.zeros((n, 4)), np.eye(n), 2, np.zeros((n, 8)))
    _refused(blmm, -10, "more than 8 null covariates", np.zeros((n, 2)), np.zeros((n, 4)), np.eye(n), 2, np.zeros((n, 9)),
             addIntercept=False)


def test_more_than_2048_individuals_is_refused(blmm):
    n = 2049
    _refused(blmm, -10, "2048", np.zeros((n, 1)), np.zeros((n, 2)), np.eye(n), 2)


@pytest.mark.parametrize("case", ["G_rows", "K_rows", "Covar_rows", "weights_len"])
def test_shape_mismatches_are_refused(blmm, case):
    n = 6
    Y = np.zeros((n, 2)); G = np.zeros((n, 4)); K = np.eye(n); kw = {}
    if case == "G_rows":
        G = np.zeros((n + 1, 4))
    elif case == "K_rows":
        K = np.eye(n + 1)[:, :n]
    elif case == "Covar_rows":
        kw["Covar"] = np.zeros((n - 1, 1))
    else:
        kw["weights"] = np.ones(n + 1)
    _refused(blmm, -2, "Dimension mismatch.", Y, G, K, 2, **kw)


@pytest.mark.parametrize("cap", [0, -3])
def test_threshold_without_a_positive_cap_is_refused(blmm, cap):
    _refused(blmm, -1, "positive `cap`", np.zeros((6, 2)), np.zeros((6, 4)), np.eye(6), 2, threshold=1.0, cap=cap)


def test_the_effects_refusal_names_the_new_call(blmm):
    with pytest.raises(blmm.BulkLMMError) as e:
        blmm.bulkscan_effects(np.zeros((6, 2)), np.zeros((6, 4)), np.eye(6), k=2)
    assert "required for k > 1" in e.value.msg and "bulkscan_multidf_reduced" in e.value.msg
