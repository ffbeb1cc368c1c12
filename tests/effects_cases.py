"""The input sets of tests/test_gpu_effects.py, in one place so that tests/test_effects_args.py can hold the CPU oracle to its own
condition on every one of them (wls by QR and by Cholesky agree on beta to 1e-9) without a GPU.  A case is a dict: Y, G, K, Cov, k,
method, kw (the options both bulkscan_effects and the oracle take), locus, trait."""
import numpy as np

from common import make_data
from test_gpu_multidf import _founder_data

GRID = [i / 10.0 for i in range(10)]


def _tests(rng, P, m, T):
    return rng.integers(0, P, size=T), rng.integers(0, m, size=T)


def _case(name, method, k, n, P, m, ncov, T=160, weights=False, reml=False, prior=None, seed=0):
    def build():
        Y, G, K, Cov = _founder_data(n, P, k, m, seed=9000 + seed, founders=2 if k == 1 else None, ncov=ncov)
        rng = np.random.default_rng(9100 + seed)
        kw = {}
        if weights:
            kw["weights"] = rng.uniform(0.5, 2.0, n)
        if reml:
            kw["reml"] = True
        if prior:
            kw["prior_variance"], kw["prior_sample_size"] = prior
        locus, trait = _tests(rng, P, m, T)
        return dict(Y=Y, G=G, K=K, Cov=Cov, k=k, method=method, kw=kw, locus=locus, trait=trait)
    return name, build


# k = 1, 2, 3, 8; both methods; c = 1, 2, 5; weights; REML with a prior; n = 79, 200, 1000 and once 2048 (k = 8, c = 2: the
# wave buffers leave LDS for the global slab from (c + 2 + k) n > 5120 doubles on)
PARITY = dict([
    _case("grid_k1_n79_c1", "null-grid", 1, 79, 120, 30, 0, seed=1),
    _case("exact_k1_n79_c2_weights", "null-exact", 1, 79, 90, 25, 1, weights=True, seed=2),
    _case("exact_k1_n1000_c1", "null-exact", 1, 1000, 40, 12, 0, T=80, seed=3),
    _case("grid_k2_n200_c5", "null-grid", 2, 200, 60, 20, 4, seed=4),
    _case("exact_k2_n79_c1_reml_prior", "null-exact", 2, 79, 80, 24, 0, reml=True, prior=(0.8, 2.0), seed=5),
    _case("grid_k3_n1000_c2", "null-grid", 3, 1000, 30, 10, 1, T=80, seed=6),
    _case("exact_k3_n200_c5_weights_reml_prior", "null-exact", 3, 200, 50, 16, 4, weights=True, reml=True, prior=(1.3, 3.0), seed=7),
    _case("grid_k8_n79_c2", "null-grid", 8, 79, 40, 18, 1, seed=8),
    _case("exact_k8_n79_c1", "null-exact", 8, 79, 40, 18, 0, seed=9),
    _case("exact_k8_n2048_c2", "null-exact", 8, 2048, 6, 5, 1, T=24, seed=10),
])


def rank_rule_case(extra):
    """k = 8 loci: `full` = all eight founder probabilities (they sum to one beside the intercept: the last column drops);
    `duplicate` = column 5 a copy of column 2; `constant` = column 3 constant."""
    n, P, m, k = 79, 30, 14, 8
    Y, G, K, _ = _founder_data(n, P, k, m, seed=9300, founders=8 if extra == "full" else 12)
    X = G.reshape(n, P, k).copy()
    if extra == "duplicate":
        X[:, :, 5] = X[:, :, 2]
    elif extra == "constant":
        X[:, :, 3] = 0.37
    rng = np.random.default_rng(9301)
    locus, trait = _tests(rng, P, m, 150)
    return dict(Y=Y, G=X.reshape(n, P * k), K=K, Cov=None, k=k, method="null-grid", kw={}, locus=locus, trait=trait)


def collinear_case():
    """test_gpu_multidf.py's conditioning-guard construction (tools/fuzz_parity.py seed 201, case 237: n = 13, a kinship with a
    zero eigenvalue) at c = 3: every other trait is made polygenic so that its likelihood peaks at the h2 -> 1 boundary, where the
    weights sit on the null eigenvector and the weighted covariates are nearly collinear (condition 9e3)."""
    Y, G, K, Cov = make_data(n=13, p=63, m=15, seed=1000 + 237 + 7919 * 201, ncov=7, bxd=False)
    const = np.ptp(G, axis=0) == 0
    if const.any():
        G = G.copy(); G[:, const] = np.random.default_rng(237).random((13, int(const.sum())))
    Cov = Cov[:, :2]
    lam, U = np.linalg.eigh(K)
    rng = np.random.default_rng(9401)
    Y = Y.copy()
    for j in range(0, 15, 2):
        Y[:, j] = 10 + (U * np.sqrt(np.maximum(lam, 0))) @ rng.standard_normal(13) * 3 + 1e-4 * rng.standard_normal(13) + Cov @ rng.standard_normal(2)
    locus, trait = _tests(rng, 21, 15, 200)
    return dict(Y=Y, G=G, K=K, Cov=Cov, k=3, method="null-exact", kw={}, locus=locus, trait=trait)


def all_cases():
    for name, build in PARITY.items():
        yield name, build
    for extra in ("full", "duplicate", "constant"):
        yield "rank_" + extra, (lambda e=extra: rank_rule_case(e))
    yield "collinear", collinear_case
