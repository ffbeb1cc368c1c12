"""The derived error bound of the fp32 permutation scan (tests/f32_ref.py) on the host: the emulation of the kernels' arithmetic is
exact, sits inside the bound, and the bound is sharp enough to reject the mistakes a tiled kernel typically makes.

No GPU: the rotation here is the host's own eigen-decomposition, which is all the bound needs (the device tests use the device's)."""
from fractions import Fraction

import numpy as np
import pytest

import f32_ref as F
from common import kinship_of, make_geno
from oracle import bulklmm_oracle as O

H2 = 0.4


def problem(n, p, nperms, seed, ncov=0, weights=False):
    """(Operands, oracle pieces): independent genotypes (neighbouring markers differ), a trait with one QTL, host rotation."""
    rng = np.random.default_rng(seed)
    G = rng.integers(0, 3, size=(n, p)) / 2.0
    K = kinship_of(make_geno(n, 200, rng))
    y = 1.0 + 0.4 * G[:, 0] + rng.standard_normal(n)
    Cov = rng.standard_normal((n, ncov)) if ncov else None
    w = rng.uniform(0.5, 1.5, n) if weights else None
    lam, U = np.linalg.eigh(F.weighted_kinship(K, w))
    pidx = O.make_perm_idx(n, nperms, seed + 1)
    return F.Operands(y, G, U.T, lam, H2, pidx, Covar=Cov, weights=w), (y, G, K, Cov, w, U.T, lam, pidx)


# ---- the emulation is the kernels' arithmetic -------------------------------------------------------------------------------
def rn32(q: Fraction) -> Fraction:
    """Round-to-nearest-even to fp32 (subnormals included), exactly."""
    if q == 0:
        return Fraction(0)
    a = abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    quantum = Fraction(2) ** (max(e, -126) - 23)
    m = a / quantum
    fl = m.numerator // m.denominator
    rem = m - fl
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and fl % 2 == 1):
        fl += 1
    return (1 if q > 0 else -1) * fl * quantum


def exact_chain(x, a, order):
    acc = Fraction(0)
    for k in order:
        acc = rn32(acc + Fraction(float(x[k])) * Fraction(float(a[k])))
    return float(acc)


@pytest.mark.parametrize("n", [9, 17, 40])
def test_emulated_fma_chain_is_exact(n):
    """emulate_chain (fp64 round-to-odd, then fp32) against exact rational arithmetic with round-to-nearest-even per step, bit
    for bit, in the scan's order and in k_rotate_f32's; operands spread over 60 binades so that sums lose bits at every step."""
    rng = np.random.default_rng(n)
    X = F.f32(rng.standard_normal((n, 3)) * 2.0 ** rng.integers(-30, 30, (n, 3)))
    A = F.f32(rng.standard_normal((n, 4)) * 2.0 ** rng.integers(-30, 30, (n, 4)))
    for order in (list(range(n)), F.rotate_order(n)):
        assert sorted(order) == list(range(n))
        got = F.emulate_chain(X, A, order)
        want = np.array([[exact_chain(X[:, i], A[:, b], order) for b in range(4)] for i in range(3)])
        assert np.array_equal(got.view(np.int64), want.view(np.int64))


def test_splitmix_perms_are_permutations():
    P = F.splitmix_perms(300, 5, 7)
    assert all(np.array_equal(np.sort(P[:, b]), np.arange(300)) for b in range(5))
    assert not np.array_equal(P[:, 0], P[:, 1])


# ---- the host model is the oracle's statistic -------------------------------------------------------------------------------
@pytest.mark.parametrize("ncov,weights", [(0, False), (2, False), (1, True), (3, True)])
def test_host_model_matches_oracle(ncov, weights):
    """Operands.L / lod (centred rotation R = Q U' W, panel sqrt(w) P pi(r0) / |r0|) equal scan_perms_lite on the same rotation."""
    op, (y, G, K, Cov, w, Ut, lam, pidx) = problem(79, 30, 12, 500 + ncov, ncov=ncov, weights=weights)
    n = y.shape[0]
    Z = np.ones((n, 1)) if Cov is None else np.hstack([np.ones((n, 1)), Cov])
    W = np.ones(n) if w is None else w
    rot = (Ut @ (W * y), Ut @ (W[:, None] * np.hstack([Z, G])), lam)
    ref = O.scan(y, G, K, covar=Z, addIntercept=False, weights=w, permutation_test=True, nperms=12, perm_idx=pidx,
                 prior_variance=1.0, prior_sample_size=0.1, h2_override=H2, rotation_override=rot)
    assert np.allclose(op.L(), ref["L_perms"], rtol=1e-9, atol=1e-12)
    assert np.allclose(op.lod(), ref["lod"], rtol=1e-9, atol=1e-12)


# ---- the emulation sits inside the bound, and how tight the bound is ---------------------------------------------------------
SIZES = {9: (40, 36), 79: (64, 48), 1000: (64, 48), 2048: (48, 40)}


@pytest.mark.parametrize("route", ["fp64-rotation", "own-rotation"])
@pytest.mark.parametrize("n", [9, 79, 1000, 2048])
def test_emulation_inside_bound(n, route):
    own = route == "own-rotation"
    p, m = SIZES[n]
    if own:
        p = 16
    op, _ = problem(n, p, m, 900 + n)
    L = op.L()
    if own:
        XF = F.emulate_rotation(op)
        assert np.all(np.abs(XF - op.X) <= op.rotation_error())
        got = F.emulate_scan(op, XF=XF, isx=F.isx_of(op, XF))
    else:
        got = F.emulate_scan(op)
    b = op.bound(own)
    ratio = np.abs(got - L) / b
    assert np.isfinite(b).all()
    q = np.quantile(ratio, [0.5, 0.99])
    print(f"n = {n} {route}: error / bound median {q[0]:.3g}, 99th percentile {q[1]:.3g}, worst {ratio.max():.3g} at "
          f"{F.locate(ratio, op)}; bound / L median {np.median(b / np.maximum(L, 1e-300)):.3g}")
    assert ratio.max() <= 1.0


# ---- the bound rejects planted mistakes ---------------------------------------------------------------------------------------
# share of entries whose emulated error exceeds the bound, per mistake (at least; observed shares are printed).  The rotated rows
# come in ascending eigenvalue order, and the last ones carry the largest eigenvalues, which the weights 1 / (1 + delta lambda) damp:
# at n >= 1000 a dropped LAST term moves no entry beyond the bound (observed 0 %), while the first term, at full weight, does.
MIN_SHARE = {
    "dropped term k = 0": {9: 0.9, 79: 0.9, 1000: 0.6, 2048: 0.5},
    "dropped term k = n - 1": {9: 0.9, 79: 0.8, 1000: 0.0, 2048: 0.0},
    "dropped K block 0": {9: 0.9, 79: 0.9, 1000: 0.9, 2048: 0.8},
    "K index shifted by one in block 0": {9: 0.9, 79: 0.9, 1000: 0.9, 2048: 0.8},
    "isx of the neighbouring marker": {9: 0.9, 79: 0.9, 1000: 0.6, 2048: 0.4},
}


@pytest.mark.parametrize("n", [9, 79, 1000, 2048])
def test_bound_rejects_planted_mistakes(n):
    p, m = SIZES[n]
    op, _ = problem(n, p, m, 900 + n)
    L = op.L()
    b = op.bound(False)
    shifted = np.arange(n)
    shifted[:8] = (np.arange(8) + 1) % 8
    swap = np.arange(p) ^ 1
    mutants = {
        "dropped term k = 0": F.emulate_scan(op, order=range(1, n)),
        "dropped term k = n - 1": F.emulate_scan(op, order=range(n - 1)),
        "dropped K block 0": F.emulate_scan(op, order=range(8, n)),
        "K index shifted by one in block 0": F.emulate_scan(op, a_index=shifted),
        "isx of the neighbouring marker": F.emulate_scan(op, isx=op.isx[swap]),
    }
    shares = {}
    for what, got in mutants.items():
        shares[what] = float(np.mean(np.abs(got - L) > b))
        print(f"n = {n}: {what}: rejected in {100 * shares[what]:.1f} % of {L.size} entries")
    for what, s in shares.items():
        assert s >= MIN_SHARE[what][n], (what, s)
