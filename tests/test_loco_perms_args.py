"""CPU checks of bulkscan_loco_perms (the leave-one-chromosome-out permutation test): every argument error is raised by the host
mirror before a context exists (no GPU needed), and the entry points are exported and declared at every layer."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHROM = ["1"] * 4 + ["2"] * 4


@pytest.fixture
def no_context(blmm, monkeypatch):
    """Any attempt to create a context fails the test: the refusals must come first."""
    def boom(*a, **k):
        raise AssertionError("a context was created before the arguments were checked")
    monkeypatch.setattr(blmm.api, "default_context", boom)
    monkeypatch.setattr(blmm.api.Context, "__init__", boom)
    return blmm


def _data(n=6, p=8, m=2):
    return np.zeros((n, m)), np.zeros((n, p))


def _raises(blmm, code, *a, **kw):
    with pytest.raises(blmm.BulkLMMError) as e:
        blmm.bulkscan_loco_perms(*a, **kw)
    assert e.value.code == code, (e.value.code, e.value.msg)
    return e.value.msg


def test_loco_perms_symbols_are_exported_and_declared(blmm):
    for name in ("bulkscan_loco_perms", "bulkscan_loco_perms_dev"):
        assert name in blmm.__all__ and callable(getattr(blmm, name))
    lib = blmm.load()
    hdr = open(os.path.join(ROOT, "include", "bulklmm_hip.h")).read()
    for sym in ("blmm_bulkscan_loco_perms", "blmm_bulkscan_loco_perms_dev"):
        assert sym in blmm.EXPORTS and hasattr(lib, sym)
        assert getattr(lib, sym).argtypes is not None and len(getattr(lib, sym).argtypes) == (32 if sym.endswith("_dev") else 31)
        assert re.search(r"\bint %s\(blmm_ctx\* ctx," % sym, hdr), sym
    jl = open(os.path.join(ROOT, "bulklmm.jl_amd", "julia", "BulkLMMHIP.jl")).read()
    assert re.search(r"ccall\(\(:blmm_bulkscan_loco_perms, libblmm\)", jl)
    assert re.search(r"^export .*\bbulkscan_loco_perms\b", jl, flags=re.M)


def test_non_contiguous_labels_are_refused_by_name(no_context):
    Y, G = _data()
    msg = _raises(no_context, -1, Y, G, ["1", "1", "2", "2", "7", "7", "2", "3"], nperms=4)
    assert "'2'" in msg and "appears again" in msg


def test_one_chromosome_is_refused(no_context):
    Y, G = _data()
    assert "at least 2 chromosomes" in _raises(no_context, -1, Y, G, ["1"] * 8, nperms=4)


@pytest.mark.parametrize("chr_start,msg", [
    ([0, 8], "at least 2 chromosomes"),
    ([0, 3, 3, 8], "chromosome 1 is empty"),
    ([1, 3, 8], "from 0 to p"),
    ([0, 3, 7], "from 0 to p"),
    ([0, 5, 3, 8], "not increasing"),
])
def test_bad_offsets_are_refused_by_the_dev_form(no_context, chr_start, msg):
    torch = pytest.importorskip("torch")
    n, p, m = 6, 8, 2
    f64 = dict(dtype=torch.float64)
    Y = torch.zeros((m, n), **f64); G = torch.zeros((p, n), **f64)
    nchr = len(chr_start) - 1
    h2, s2 = torch.zeros((nchr, m), **f64), torch.zeros((nchr, m), **f64)
    mx, arg = torch.zeros(m, **f64), torch.zeros(m, dtype=torch.int64)
    with pytest.raises(no_context.BulkLMMError) as e:
        no_context.bulkscan_loco_perms_dev(None, Y, G, chr_start, h2, s2, mx, arg, nperms=4)
    assert msg in e.value.msg and e.value.code == -1


@pytest.mark.parametrize("case", ["G_rows", "chrom_len", "Covar_rows", "weights_len", "perm_idx_shape", "perm_idx_rows"])
def test_shape_mismatches_are_refused(no_context, case):
    n, p = 6, 8
    Y, G = _data(n, p)
    chrom = list(CHROM)
    kw = {"nperms": 4}
    if case == "G_rows":
        G = np.zeros((n + 1, p))
    elif case == "chrom_len":
        chrom = chrom[:-1]
    elif case == "Covar_rows":
        kw["Covar"] = np.zeros((n - 1, 1))
    elif case == "weights_len":
        kw["weights"] = np.ones(n + 1)
    elif case == "perm_idx_shape":
        kw["perm_idx"] = np.zeros((n, 3), dtype=np.int32)      # nperms = 4 columns expected
    elif case == "perm_idx_rows":
        kw["perm_idx"] = np.zeros((n - 1, 4), dtype=np.int32)
    assert _raises(no_context, -2, Y, G, chrom, **kw) == "Dimension mismatch."


def test_more_than_2048_individuals_is_refused(no_context):
    n = 2049
    assert "2048" in _raises(no_context, -10, np.zeros((n, 1)), np.zeros((n, 4)), ["a", "a", "b", "b"], nperms=2)


def test_negative_nperms_is_refused(no_context):
    Y, G = _data()
    assert _raises(no_context, -9, Y, G, CHROM, nperms=-1) == "The required number of permutations must be a positive integer."


def test_more_than_16384_permutations_is_refused(no_context):
    Y, G = _data()
    assert "16384" in _raises(no_context, -10, Y, G, CHROM, nperms=16385)


def test_more_than_8_null_covariates_is_refused(no_context):
    Y, G = _data(n=12)
    msg = _raises(no_context, -10, Y, G, CHROM, np.zeros((12, 8)), nperms=4)          # 8 + the intercept
    assert "more than 8 null covariates" in msg
    with pytest.raises(AssertionError, match="a context was created"):                # 8 without the intercept: accepted
        no_context.bulkscan_loco_perms(Y, G, CHROM, np.zeros((12, 8)), nperms=4, addIntercept=False)


def test_more_than_64_levels_is_refused(no_context):
    Y, G = _data()
    assert "64" in _raises(no_context, -1, Y, G, CHROM, nperms=4, signif_level=np.linspace(0.01, 0.5, 65))


@pytest.mark.parametrize("bad", [-1, 6])
def test_out_of_range_perm_idx_is_refused(no_context, bad):
    Y, G = _data()
    pidx = np.tile(np.arange(6, dtype=np.int32)[:, None], (1, 4))
    pidx[3, 2] = bad
    assert "perm_idx entries must lie in 0 .. n - 1" in _raises(no_context, -1, Y, G, CHROM, nperms=4, perm_idx=pidx)
