"""CPU checks of the reduced leave-one-chromosome-out bulkscan (blmm_bulkscan_loco_reduced): it is exported and declared at every
layer, and every argument error is raised by the host mirror before a context exists (no GPU needed)."""
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


def test_loco_reduced_symbols_are_exported_and_declared(blmm):
    for name in ("bulkscan_loco_reduced", "bulkscan_loco_reduced_dev"):
        assert name in blmm.__all__ and callable(getattr(blmm, name))
    lib = blmm.load()
    hdr = open(os.path.join(ROOT, "include", "bulklmm_hip.h")).read()
    for sym in ("blmm_bulkscan_loco_reduced", "blmm_bulkscan_loco_reduced_dev"):
        assert sym in blmm.EXPORTS and hasattr(lib, sym)
        assert re.search(r"\bint %s\(blmm_ctx\* ctx," % sym, hdr), sym
        assert len(getattr(lib, sym).argtypes) == (20 if sym.endswith("reduced") else 21), sym
    jl = open(os.path.join(ROOT, "bulklmm.jl_amd", "julia", "BulkLMMHIP.jl")).read()
    assert re.search(r"ccall\(\(:blmm_bulkscan_loco_reduced, libblmm\)", jl)
    assert re.search(r"^export .*\bbulkscan_loco_reduced\b", jl, flags=re.M)


def test_non_contiguous_labels_are_refused_by_name(no_context):
    Y, G = _data()
    with pytest.raises(no_context.BulkLMMError) as e:
        no_context.bulkscan_loco_reduced(Y, G, ["1", "1", "2", "2", "7", "7", "2", "3"])
    assert "'2'" in e.value.msg and "appears again" in e.value.msg


def test_one_chromosome_is_refused(no_context):
    Y, G = _data()
    with pytest.raises(no_context.BulkLMMError) as e:
        no_context.bulkscan_loco_reduced(Y, G, ["1"] * 8)
    assert "at least 2 chromosomes" in e.value.msg and e.value.code == -1


@pytest.mark.parametrize("chr_start,msg", [
    ([0, 8], "at least 2 chromosomes"),
    ([0, 3, 3, 8], "chromosome 1 is empty"),
    ([0, 8, 8], "chromosome 1 is empty"),
    ([1, 3, 8], "from 0 to p"),
    ([0, 3, 7], "from 0 to p"),
    ([0, 5, 3, 8], "not increasing"),
])
def test_bad_offsets_are_refused_by_the_dev_form(no_context, chr_start, msg):
    torch = pytest.importorskip("torch")
    n, p, m = 6, 8, 2
    Y = torch.zeros((m, n), dtype=torch.float64); G = torch.zeros((p, n), dtype=torch.float64)
    with pytest.raises(no_context.BulkLMMError) as e:
        no_context.bulkscan_loco_reduced_dev(None, Y, G, chr_start, None, None, None, None, None)
    assert msg in e.value.msg and e.value.code == -1


@pytest.mark.parametrize("case", ["G_rows", "chrom_len", "Covar_rows", "weights_len"])
def test_shape_mismatches_are_refused(no_context, case):
    n, p = 6, 8
    Y, G = _data(n, p)
    chrom = list(CHROM)
    kw = {}
    if case == "G_rows":
        G = np.zeros((n + 1, p))
    elif case == "chrom_len":
        chrom = chrom[:-1]
    elif case == "Covar_rows":
        kw["Covar"] = np.zeros((n - 1, 1))
    elif case == "weights_len":
        kw["weights"] = np.ones(n + 1)
    with pytest.raises(no_context.BulkLMMError) as e:
        no_context.bulkscan_loco_reduced(Y, G, chrom, **kw)
    assert e.value.code == -2 and e.value.msg == "Dimension mismatch."


def test_more_than_2048_individuals_is_refused(no_context):
    n = 2049
    with pytest.raises(no_context.BulkLMMError) as e:
        no_context.bulkscan_loco_reduced(np.zeros((n, 1)), np.zeros((n, 4)), ["a", "a", "b", "b"])
    assert e.value.code == -10 and "2048" in e.value.msg


@pytest.mark.parametrize("dev", [False, True])
def test_unknown_method_is_refused(no_context, dev):
    Y, G = _data()
    with pytest.raises(no_context.BulkLMMError) as e:
        if dev:
            torch = pytest.importorskip("torch")
            no_context.bulkscan_loco_reduced_dev(None, torch.zeros((2, 6), dtype=torch.float64), torch.zeros((8, 6), dtype=torch.float64),
                                                 [0, 4, 8], None, None, None, None, None, method="nope")
        else:
            no_context.bulkscan_loco_reduced(Y, G, CHROM, method="nope")
    assert e.value.code == -5


def test_negative_cap_is_refused(no_context):
    Y, G = _data()
    with pytest.raises(no_context.BulkLMMError) as e:
        no_context.bulkscan_loco_reduced(Y, G, CHROM, threshold=3.0, cap=-1)
    assert e.value.code == -1 and "cap" in e.value.msg
