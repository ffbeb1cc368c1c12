"""Edges of the grid methods on small shapes, against the NumPy oracle, for both h2_panel rules (first arg-max and the reference's
improvement counter): grid lengths around the packed / unpacked arg-max boundary of k_scan_alt (<= 255 grid points
pack the arg-max into bytes, longer grids use k_scan_alt<..., false>), an unsorted grid with duplicates, ragged 128-marker and
32-trait tiles, and c = 3 with REML, a prior and weights.  L within 1e-6 |ref| + 1e-10; h2_panel equal to the oracle's or tied in
its logL1 to 1e-12 relative, and exactly equal on the duplicated grid, whose equal values give equal logL1 on both sides."""
import numpy as np
import pytest

from common import assert_h2_panel_ties_only, assert_lod_close, make_data
from oracle import bulklmm_oracle as O

pytestmark = pytest.mark.gpu

DUP = [0.5, 0.25, 0.5, 0.0, 0.25, 0.75, 0.0, 0.5, 0.125, 0.75]


def grid_of(ng):
    return list(np.linspace(0.0, 0.95, ng)) if ng > 1 else [0.3]


def check_alt(blmm, Y, G, K, grid, Cov=None, exact_panel=False, **kw):
    for quirk in (False, True):
        got = blmm.bulkscan_alt_grid(Y, G, K, grid, Cov, compat_counter_quirk=quirk, **kw)
        ref, tab = O.bulkscan_alt_grid(Y, G, K, grid, Covar=Cov, compat_counter_quirk=quirk, return_tables=True, **kw)
        assert_lod_close(got.L, ref.L, what=f"alt-grid L ({len(grid)} grid points, counter rule {quirk})")
        if exact_panel:
            assert np.array_equal(got.h2_panel, ref.h2_panel)
        else:
            nt = assert_h2_panel_ties_only(got.h2_panel, ref.h2_panel, tab, grid, quirk=quirk)
            assert nt <= 1e-3 * ref.h2_panel.size


def check_null_grid(blmm, Y, G, K, grid, Cov=None, **kw):
    got = blmm.bulkscan_null_grid(Y, G, K, grid, Cov, **kw)
    ref = O.bulkscan_null_grid(Y, G, K, grid, Covar=Cov, **kw)
    assert np.array_equal(got.h2_null_list, ref.h2_null_list)
    assert_lod_close(got.L, ref.L, what=f"null-grid L ({len(grid)} grid points)")


@pytest.mark.parametrize("ng", [1, 2, 255, 256, 300])
def test_alt_grid_lengths_around_the_packed_argmax(blmm, ng):
    Y, G, K, _ = make_data(p=150, m=37, seed=8100 + ng)
    grid = grid_of(ng)
    check_alt(blmm, Y, G, K, grid)
    if ng >= 256:
        check_null_grid(blmm, Y, G, K, grid)
        assert len(np.unique(blmm.bulkscan_alt_grid(Y, G, K, grid).h2_panel)) > 10   # the unpacked arg-max really spans the grid


def test_unsorted_grid_with_duplicates(blmm):
    """Equal grid values give equal logL1: the first maximum wins on both sides, so the panel and the null-grid choice are exact."""
    Y, G, K, _ = make_data(p=150, m=37, seed=8200)
    check_alt(blmm, Y, G, K, DUP, exact_panel=True)
    check_null_grid(blmm, Y, G, K, DUP)


@pytest.mark.parametrize("p", [1, 127, 128, 129])
@pytest.mark.parametrize("m", [1, 31, 33, 65])
def test_ragged_tiles(blmm, p, m):
    Y, G, K, _ = make_data(p=max(p, 2), m=m, seed=8300 + p + 7 * m)
    G = G[:, :p]
    grid = [i / 10.0 for i in range(10)]
    check_alt(blmm, Y, G, K, grid)
    check_null_grid(blmm, Y, G, K, grid)


def test_c3_reml_prior_weights(blmm):
    Y, G, K, Cov = make_data(p=150, m=37, seed=8400, ncov=2)
    w = np.random.default_rng(8400).uniform(0.5, 2.0, Y.shape[0])
    kw = dict(reml=True, prior_variance=1.0, prior_sample_size=0.1, weights=w)
    grid = [i / 16.0 for i in range(16)]
    check_alt(blmm, Y, G, K, grid, Cov, **kw)
    check_null_grid(blmm, Y, G, K, grid, Cov, **kw)
    check_alt(blmm, Y, G, K, grid_of(300), Cov, **kw)
