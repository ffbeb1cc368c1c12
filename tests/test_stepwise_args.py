"""bulkscan_stepwise (blmm_bulkscan_stepwise) without a GPU: the entry points are exported and declared at every layer, and every
refusal of the contract is raised by the host mirror before a context exists, with the library's code, message and order.  The same
refusals through the C ABI, host and _dev prototypes in the same order, need a context: tests/test_gpu_stepwise.py."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_context(blmm, monkeypatch):
    """Any attempt to create a context fails the test: the refusals must come first."""
    def boom(*a, **k):
        raise AssertionError("a context was created before the arguments were checked")
    monkeypatch.setattr(blmm.api, "default_context", boom)
    monkeypatch.setattr(blmm.api.Context, "__init__", boom)
    return blmm


def test_bulkscan_stepwise_is_exported_and_declared(blmm):
    assert "bulkscan_stepwise" in blmm.__all__ and "bulkscan_stepwise_dev" in blmm.__all__
    assert callable(blmm.bulkscan_stepwise) and callable(blmm.bulkscan_stepwise_dev)
    lib = blmm.load()
    hdr = open(os.path.join(ROOT, "include", "bulklmm_hip.h")).read()
    for sym in ("blmm_bulkscan_stepwise", "blmm_bulkscan_stepwise_dev"):
        assert sym in blmm.EXPORTS and hasattr(lib, sym)
        assert re.search(r"^int %s\(blmm_ctx\* ctx," % sym, hdr, flags=re.M), sym
    assert re.search(r"#define BLMM_VERSION 210\b", hdr)                      # appended to the comment only
    assert re.search(r"added since without a new number:[^/]*blmm_bulkscan_stepwise\[_dev\]", hdr)
    jl = open(os.path.join(ROOT, "bulklmm.jl_amd", "julia", "BulkLMMHIP.jl")).read()
    assert re.search(r"ccall\(\(:blmm_bulkscan_stepwise, libblmm\)", jl)
    assert re.search(r"ccall\(\(:blmm_bulkscan_stepwise_dev, libblmm\)", jl)
    assert re.search(r"^export .*\bbulkscan_stepwise\b", jl, flags=re.M)


def test_the_info_length_equals_the_headers(blmm):
    hdr = open(os.path.join(ROOT, "include", "bulklmm_hip.h")).read()
    m = re.search(r"#define BLMM_STEP_INFO_LEN (\d+)\b", hdr)
    assert m and int(m.group(1)) == blmm._lib.BLMM_STEP_INFO_LEN == 8


def test_the_new_tuning_key_is_documented():
    hdr = open(os.path.join(ROOT, "include", "bulklmm_hip.h")).read()
    assert '"cond_red_chunk"' in hdr


def test_a_null_context_is_refused_by_both_prototypes(blmm):
    lib = blmm.load()
    args = [None] * 13 + [1, 3.0] + [None] * 7
    for i in (3, 4, 6, 8, 12):
        args[i] = 0
    assert lib.blmm_bulkscan_stepwise(*args) == -1 and lib.blmm_bulkscan_stepwise_dev(*args) == -1


def _refused(b, code, msg, *args, **kw):
    kw.setdefault("threshold", 3.0)
    with pytest.raises(b.BulkLMMError) as e:
        b.bulkscan_stepwise(*args, **kw)
    assert e.value.code == code, (e.value.code, e.value.msg)
    assert msg in e.value.msg, e.value.msg


def _zeros(n=12, p=6, m=3):
    return np.zeros((n, m)), np.zeros((n, p)), np.eye(n)


def test_the_threshold_is_required(blmm):
    with pytest.raises(TypeError):
        blmm.bulkscan_stepwise(*_zeros())


@pytest.mark.parametrize("S", [0, -1])
def test_no_locus_is_refused(no_context, S):
    _refused(no_context, -1, "max_loci must be at least 1", *_zeros(), max_loci=S)


def test_five_loci_are_refused(no_context):
    _refused(no_context, -10, "at most 4 loci per trait", *_zeros(), max_loci=5)


@pytest.mark.parametrize("ncov,S,addI", [(7, 1, True), (4, 4, True), (8, 1, False), (5, 4, False)])
def test_nine_design_columns_are_refused(no_context, ncov, S, addI):
    n = 30
    _refused(no_context, -10, "more than 8 null-design columns", *_zeros(n), np.zeros((n, ncov)), max_loci=S, addIntercept=addI)


@pytest.mark.parametrize("thr", [float("nan"), -1e-300, -3.0, float("-inf")])
def test_a_negative_or_nan_threshold_is_refused(no_context, thr):
    _refused(no_context, -1, "the threshold must be a number >= 0", *_zeros(), threshold=thr)


def test_alt_grid_and_unknown_methods_are_refused(no_context):
    _refused(no_context, -10, "alt-grid is not supported", *_zeros(), method="alt-grid")
    _refused(no_context, -5, "Unknown method", *_zeros(), method="grid")


def test_more_than_2048_individuals_are_refused(no_context):
    _refused(no_context, -10, "more than 2048 individuals", np.zeros((2049, 1)), np.zeros((2049, 2)), np.eye(2049))


def test_a_design_as_long_as_the_sample_is_refused(no_context):
    _refused(no_context, -2, "Dimension mismatch.", *_zeros(n=5), max_loci=4)          # c + S = 5 >= n


def test_shape_mismatches_are_refused(no_context):
    _refused(no_context, -2, "Dimension mismatch.", np.zeros((6, 2)), np.zeros((7, 4)), np.eye(6))
    _refused(no_context, -2, "Dimension mismatch.", np.zeros((6, 2)), np.zeros((6, 4)), np.eye(6), weights=np.ones(7))


def test_the_order_of_the_refusals(no_context):
    """max_loci < 1, then the two limits, then the threshold, then bulkscan_cond's own (method, alt-grid, n, c + S >= n)."""
    big = (np.zeros((2049, 1)), np.zeros((2049, 2)), np.eye(2049))
    _refused(no_context, -1, "max_loci must be at least 1", *big, max_loci=0, threshold=-1.0, method="alt-grid")
    _refused(no_context, -10, "at most 4 loci per trait", *big, max_loci=5, threshold=-1.0, method="alt-grid")
    _refused(no_context, -10, "more than 8 null-design columns", *big, np.zeros((2049, 7)), max_loci=1, threshold=-1.0, method="grid")
    _refused(no_context, -1, "the threshold must be", *big, threshold=float("nan"), method="grid")
    _refused(no_context, -5, "Unknown method", *big, method="grid")
    _refused(no_context, -10, "alt-grid is not supported", *big, method="alt-grid")
    _refused(no_context, -10, "more than 2048 individuals", *big)


def test_a_fractional_max_loci_is_refused(no_context):
    _refused(no_context, -1, "max_loci must be an integer", *_zeros(), max_loci=1.9)
    _refused(no_context, -1, "max_loci must be an integer", *_zeros(), max_loci="2")


def test_the_device_mirror_refuses_in_the_same_order(no_context):
    """bulkscan_stepwise_dev on tensors that never reach a device: the library's refusals (max_loci is loci_out's width) come before
    the mirror's own complaints about the output tensors."""
    import torch
    n, p, m = 12, 6, 3
    Y, G, K = torch.zeros(m, n, dtype=torch.float64), torch.zeros(p, n, dtype=torch.float64), torch.eye(n, dtype=torch.float64)

    def outs(S, rows=m):
        return [torch.zeros(rows, S, dtype=torch.int64), torch.zeros(m, S + 1, dtype=torch.float64),
                torch.zeros(m, S + 1, dtype=torch.int64), torch.zeros(m, S + 1, dtype=torch.float64), torch.zeros(m, dtype=torch.int64)]

    def refused(code, msg, o, **kw):
        kw.setdefault("threshold", 3.0)
        with pytest.raises(no_context.BulkLMMError) as e:
            no_context.bulkscan_stepwise_dev(None, Y, G, K, *o, **kw)
        assert e.value.code == code and msg in e.value.msg, (e.value.code, e.value.msg)

    refused(-1, "max_loci must be at least 1", outs(0, rows=m + 1), threshold=-1.0, method="alt-grid")
    refused(-10, "at most 4 loci per trait", outs(5, rows=m + 1), threshold=-1.0, method="alt-grid")
    refused(-10, "more than 8 null-design columns", outs(2, rows=m + 1), Covar=torch.zeros(6, n, dtype=torch.float64), threshold=-1.0)
    refused(-1, "the threshold must be", outs(2, rows=m + 1), threshold=float("nan"), method="grid")
    refused(-5, "Unknown method", outs(2, rows=m + 1), method="grid")
    refused(-10, "alt-grid is not supported", outs(2, rows=m + 1), method="alt-grid")
    refused(-2, "loci_out must be", outs(2, rows=m + 1))
    o = outs(2)
    o[1] = torch.zeros(m, 2, dtype=torch.float64)
    refused(-2, "lod_out, argmax_out and h2_out must be", o)
