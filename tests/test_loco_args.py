"""CPU checks of the leave-one-chromosome-out (LOCO) entry points: every argument error is raised by the host mirror before a context
exists (no GPU needed), and calcKinship_loco / bulkscan_loco are exported and declared at every layer."""
import json
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


def _data(n=6, p=8, m=2):
    return np.zeros((n, m)), np.zeros((n, p))


def test_loco_symbols_are_exported_and_declared(blmm):
    for name in ("calcKinship_loco", "bulkscan_loco", "bulkscan_loco_dev"):
        assert name in blmm.__all__ and callable(getattr(blmm, name))
    lib = blmm.load()
    hdr = open(os.path.join(ROOT, "include", "bulklmm_hip.h")).read()
    for sym in ("blmm_kinship_loco", "blmm_kinship_loco_dev", "blmm_bulkscan_loco", "blmm_bulkscan_loco_dev"):
        assert sym in blmm.EXPORTS and hasattr(lib, sym)
        assert re.search(r"\bint %s\(blmm_ctx\* ctx," % sym, hdr), sym
    jl = open(os.path.join(ROOT, "bulklmm.jl_amd", "julia", "BulkLMMHIP.jl")).read()
    for sym in ("blmm_kinship_loco", "blmm_bulkscan_loco"):
        assert re.search(r"ccall\(\(:%s, libblmm\)" % sym, jl), sym
    for name in ("calcKinship_loco", "bulkscan_loco"):
        assert re.search(r"^export .*\b%s\b" % name, jl, flags=re.M), name


def test_bxd_fixture_runs():
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "bxd_chr_runs.json")))
    assert fx["chromosomes"] == [str(i) for i in range(1, 20)] + ["X"]
    assert sum(fx["counts"]) == 7321 and min(fx["counts"]) > 0


def test_chromosome_runs(blmm):
    runs, cs = blmm.chromosome_runs(["1", "1", "2", "X", "X"], 5)
    assert runs == ["1", "2", "X"] and cs.tolist() == [0, 2, 3, 5]
    runs, cs = blmm.chromosome_runs(np.array([3, 3, 1, 1, 1]), 5)   # run order, not sorted order
    assert runs == [3, 1] and cs.tolist() == [0, 2, 5]


@pytest.mark.parametrize("fn", ["bulkscan_loco", "calcKinship_loco"])
def test_non_contiguous_labels_are_refused_by_name(no_context, fn):
    Y, G = _data()
    chrom = ["1", "1", "2", "2", "7", "7", "2", "3"]
    with pytest.raises(no_context.BulkLMMError) as e:
        no_context.bulkscan_loco(Y, G, chrom) if fn == "bulkscan_loco" else no_context.calcKinship_loco(G, chrom)
    assert "'2'" in e.value.msg and "appears again" in e.value.msg


@pytest.mark.parametrize("fn", ["bulkscan_loco", "calcKinship_loco"])
def test_one_chromosome_is_refused(no_context, fn):
    Y, G = _data()
    with pytest.raises(no_context.BulkLMMError) as e:
        no_context.bulkscan_loco(Y, G, ["1"] * 8) if fn == "bulkscan_loco" else no_context.calcKinship_loco(G, ["1"] * 8)
    assert "at least 2 chromosomes" in e.value.msg and e.value.code == -1


@pytest.mark.parametrize("chr_start,msg", [
    ([0, 8], "at least 2 chromosomes"),
    ([0, 3, 3, 8], "chromosome 1 is empty"),
    ([0, 8, 8], "chromosome 1 is empty"),                # the other run holds every marker
    ([1, 3, 8], "from 0 to p"),
    ([0, 3, 7], "from 0 to p"),
    ([0, 5, 3, 8], "not increasing"),
])
def test_bad_offsets_are_refused(no_context, chr_start, msg):
    torch = pytest.importorskip("torch")
    n, p, m = 6, 8, 2
    Y = torch.zeros((m, n), dtype=torch.float64); G = torch.zeros((p, n), dtype=torch.float64)
    Lo = torch.zeros((m, p), dtype=torch.float64); h2 = torch.zeros((len(chr_start) - 1, m), dtype=torch.float64)
    with pytest.raises(no_context.BulkLMMError) as e:
        no_context.bulkscan_loco_dev(None, Y, G, chr_start, Lo, h2)
    assert msg in e.value.msg and e.value.code == -1


@pytest.mark.parametrize("case", ["G_rows", "chrom_len", "Covar_rows", "weights_len"])
def test_shape_mismatches_are_refused(no_context, case):
    n, p = 6, 8
    Y, G = _data(n, p)
    chrom = ["1"] * 4 + ["2"] * 4
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
        no_context.bulkscan_loco(Y, G, chrom, **kw)
    assert e.value.code == -2 and e.value.msg == "Dimension mismatch."


def test_more_than_2048_individuals_is_refused(no_context):
    n, p = 2049, 4
    with pytest.raises(no_context.BulkLMMError) as e:
        no_context.bulkscan_loco(np.zeros((n, 1)), np.zeros((n, p)), ["a", "a", "b", "b"])
    assert e.value.code == -10 and "2048" in e.value.msg


def test_unknown_method_is_refused(no_context):
    Y, G = _data()
    with pytest.raises(no_context.BulkLMMError) as e:
        no_context.bulkscan_loco(Y, G, ["1"] * 4 + ["2"] * 4, method="nope")
    assert e.value.code == -5


def test_too_many_chromosomes_is_refused(no_context):
    torch = pytest.importorskip("torch")
    n, m, p = 4, 1, 65536
    Y = torch.zeros((m, n), dtype=torch.float64); G = torch.zeros((p, n), dtype=torch.float64)
    with pytest.raises(no_context.BulkLMMError) as e:
        no_context.bulkscan_loco_dev(None, Y, G, np.arange(p + 1), torch.zeros((m, p), dtype=torch.float64), None)
    assert "65535" in e.value.msg and e.value.code == -1
