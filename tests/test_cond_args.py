"""CPU checks of bulkscan_cond (blmm_bulkscan_cond): every refusal is raised by the host mirror before a context exists, with the
library's code and message; the entry points are exported and declared at every layer; the oracle (tests/cond_ref.py) agrees with
the reference's own scan of (y_j, G, [Covar g_q], K) away from the rank rule's rows."""
import os
import re

import numpy as np
import pytest

from common import RTOL, ATOL, make_data
from cond_ref import TAU, bulkscan_cond_ref, step1
from oracle import bulklmm_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_context(blmm, monkeypatch):
    """Any attempt to create a context fails the test: the refusals must come first."""
    def boom(*a, **k):
        raise AssertionError("a context was created before the arguments were checked")
    monkeypatch.setattr(blmm.api, "default_context", boom)
    monkeypatch.setattr(blmm.api.Context, "__init__", boom)
    return blmm


def test_bulkscan_cond_is_exported_and_declared(blmm):
    assert "bulkscan_cond" in blmm.__all__ and "bulkscan_cond_dev" in blmm.__all__
    lib = blmm.load()
    hdr = open(os.path.join(ROOT, "include", "bulklmm_hip.h")).read()
    for sym in ("blmm_bulkscan_cond", "blmm_bulkscan_cond_dev"):
        assert sym in blmm.EXPORTS and hasattr(lib, sym)
        assert re.search(r"\bint %s\(blmm_ctx\* ctx," % sym, hdr), sym
    assert re.search(r"#define BLMM_COND_TAU BLMM_MULTIDF_TAU\b", hdr) and re.search(r"#define BLMM_COND_MAX_LOCI 4\b", hdr)
    assert re.search(r"#define BLMM_COND_INFO_LEN 4\b", hdr) and re.search(r"#define BLMM_VERSION 210\b", hdr)
    L = blmm._lib
    assert (L.BLMM_COND_TAU, L.BLMM_COND_MAX_LOCI, L.BLMM_COND_INFO_LEN) == (1e-8, 4, 4)
    jl = open(os.path.join(ROOT, "bulklmm.jl_amd", "julia", "BulkLMMHIP.jl")).read()
    assert re.search(r"ccall\(\(:blmm_bulkscan_cond, libblmm\)", jl)
    assert re.search(r"^export .*\bbulkscan_cond\b", jl, flags=re.M)


def _refused(b, code, msg, *args, **kw):
    with pytest.raises(b.BulkLMMError) as e:
        b.bulkscan_cond(*args, **kw)
    assert e.value.code == code, (e.value.code, e.value.msg)
    assert msg in e.value.msg, e.value.msg


def _zeros(n=12, p=6, m=3):
    return np.zeros((n, m)), np.zeros((n, p)), np.eye(n)


def test_alt_grid_and_unknown_methods_are_refused(no_context):
    Y, G, K = _zeros()
    _refused(no_context, -10, "bulkscan_cond: alt-grid is not supported", Y, G, K, [0, 1, 2], method="alt-grid")
    _refused(no_context, -5, "Unknown method", Y, G, K, [0, 1, 2], method="grid")


def test_more_than_2048_individuals_are_refused(no_context):
    _refused(no_context, -10, "more than 2048 individuals", np.zeros((2049, 1)), np.zeros((2049, 2)), np.eye(2049), [0])


def test_five_loci_are_refused(no_context):
    Y, G, K = _zeros()
    _refused(no_context, -10, "at most 4 conditioning loci", Y, G, K, np.zeros((3, 5), dtype=int))


@pytest.mark.parametrize("ncov,s,addI", [(7, 1, True), (4, 4, True), (8, 1, False), (5, 4, False)])
def test_nine_design_columns_are_refused(no_context, ncov, s, addI):
    n = 30
    Y, G, K = _zeros(n)
    _refused(no_context, -10, "more than 8 null-design columns", Y, G, K, np.zeros((3, s), dtype=int), np.zeros((n, ncov)),
             addIntercept=addI)


@pytest.mark.parametrize("bad", [6, -2, 100])
def test_an_index_outside_the_markers_is_refused(no_context, bad):
    Y, G, K = _zeros()
    _refused(no_context, -1, "trait 1 has a conditioning index outside [-1, p)", Y, G, K, [0, bad, -1])
    _refused(no_context, -1, "trait 2 has a conditioning index outside", Y, G, K, np.array([[0, 1], [2, -1], [3, bad]]))


def test_cond_shapes(no_context):
    Y, G, K = _zeros()
    _refused(no_context, -2, "cond must have shape (m,) or (m, s)", Y, G, K, [0, 1])
    _refused(no_context, -2, "cond must have shape (m,) or (m, s)", Y, G, K, np.zeros((2, 3), dtype=int))
    _refused(no_context, -2, "cond must have shape (m,) or (m, s)", Y, G, K, np.zeros((3, 1, 1), dtype=int))
    _refused(no_context, -1, "integer column indices", Y, G, K, [0.0, 1.0, 2.0])
    _refused(no_context, -1, 'the string "peak"', Y, G, K, "peek")
    _refused(no_context, -2, "Dimension mismatch.", np.zeros((4, 3)), np.zeros((4, 6)), np.eye(4), np.zeros((3, 3), dtype=int))


def test_peak_checks_its_arguments_before_a_context(no_context):
    Y, G, K = _zeros()
    _refused(no_context, -10, "alt-grid is not supported", Y, G, K, "peak", method="alt-grid")
    _refused(no_context, -10, "more than 8 null-design columns", np.zeros((30, 3)), np.zeros((30, 6)), np.eye(30), "peak",
             np.zeros((30, 7)))


def test_step1_drops_repeats_covariates_and_constants():
    rng = np.random.default_rng(5)
    n = 40
    Z0 = np.hstack([np.ones((n, 1)), rng.standard_normal((n, 1))])
    X = rng.standard_normal((n, 6))
    X[:, 2] = Z0[:, 1]          # equal to a covariate
    X[:, 3] = 3.0               # constant beside the intercept
    X[:, 4] = X[:, 0] + X[:, 1]  # in the span of two kept ones
    kept, nd = step1(Z0, X, np.array([0, 0, 2, -1, 3, 1, 4, 5]))
    assert kept.tolist() == [0, 1, 5] and nd == 4
    kept, nd = step1(Z0, X, np.array([-1, -1]))
    assert kept.size == 0 and nd == 0


@pytest.mark.parametrize("n,p,m,ncov,seed", [(79, 120, 6, 0, 1), (60, 90, 5, 2, 2)])
def test_oracle_agrees_with_the_reference_scan_of_the_augmented_covariates(n, p, m, ncov, seed):
    """Column j of the oracle against O.bulkscan_null(y_j, G without the rule's rows, K, [Cov g_q]): h2 to the search's tolerance,
    LOD (the reference pinned at the oracle's h2) within the parity bound."""
    Y, G, K, Cov = make_data(n=n, p=p, m=m, seed=seed, ncov=ncov)
    cond = np.argmax(O.bulkscan_null(Y, G, K, Cov).L, axis=0)
    L, H, RHO, kept, nd = bulkscan_cond_ref(Y, G, K, cond, Cov)
    assert nd == 0 and all(k.tolist() == [int(q)] for k, q in zip(kept, cond))
    for j in range(m):
        assert L[cond[j], j] == 0.0 and RHO[cond[j], j] <= TAU
        dec = RHO[:, j] > 100 * TAU
        Cj = G[:, [cond[j]]] if Cov is None else np.hstack([Cov, G[:, [cond[j]]]])
        own = O.bulkscan_null(Y[:, [j]], G[:, dec], K, Cj)
        assert abs(own.h2_null_list[0] - H[j]) <= 1e-6
        ref = O.bulkscan_null(Y[:, [j]], G[:, dec], K, Cj, h2_override=np.array([H[j]]))
        assert np.all(np.abs(ref.L[:, 0] - L[dec, j]) <= RTOL * np.abs(ref.L[:, 0]) + ATOL)
