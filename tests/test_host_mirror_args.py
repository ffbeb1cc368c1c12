"""The Python mirror's argument refusals, entry point by entry point, without a GPU: for every bad input the exact exception (type,
code, message) comes back before a context exists, and where two inputs are bad at once the same check fires first as it always
has.  Then the two places where the device forms once differed from the host forms: an unknown method, and a 2-D h2 grid."""
import numpy as np
import pytest

N_MSG = "more than 2048 individuals: the device eigensolver (tridiagonalisation + divide and conquer) stops at n = 2048"
REFUSALS = {
    "method": (-5, "Unknown method `nope`; choose null-exact, null-grid or alt-grid."),
    "shape": (-2, "Dimension mismatch."),
    "K_rows": (-2, "Dimension mismatch."),
    "K_cols": (-2, "Dimension mismatch."),
    "n": (-10, N_MSG),
    "covar": (-2, "Dimension mismatch."),
    "weights": (-2, "Dimension mismatch."),
    "perm_idx": (-2, "Dimension mismatch."),
}
MULTIDF_METHOD = (-5, "Unknown method; choose null-exact, null-grid or alt-grid.")
P = 4
CHROM = ["1", "1", "2", "2"]


@pytest.fixture
def no_context(blmm, monkeypatch):
    """Any attempt to create a context fails the test: the refusals must come first."""
    def boom(*a, **k):
        raise AssertionError("a context was created before the arguments were checked")
    monkeypatch.setattr(blmm.api, "default_context", boom)
    monkeypatch.setattr(blmm.api.Context, "__init__", boom)
    monkeypatch.setattr(blmm.api.MultiContext, "__init__", boom)
    return blmm


def _inputs(faults):
    """Host inputs with the given faults: n = 6 individuals (2049 with "n"), P markers, 2 traits."""
    n = 2049 if "n" in faults else 6
    d = {"Y": np.zeros((n, 2)), "G": np.zeros((n + ("shape" in faults), P)), "K": np.zeros((n, n), order="F"), "kw": {}}
    if "K_rows" in faults:
        d["K"] = np.zeros((n + 1, n), order="F")
    if "K_cols" in faults:
        d["K"] = np.zeros((n, n + 1), order="F")
    if "covar" in faults:
        d["kw"]["Covar"] = np.zeros((n - 1, 1))
    if "weights" in faults:
        d["kw"]["weights"] = np.ones(n + 1)
    if "method" in faults:
        d["kw"]["method"] = "nope"
    d["pidx"] = np.zeros((n, 3 if "perm_idx" in faults else 4), dtype=np.int32)
    return d


def _scan(B, d):
    kw = dict(d["kw"])
    if "Covar" in kw:
        kw["covar"] = kw.pop("Covar")
    return B.scan(d["Y"][:, :1], d["G"], d["K"], permutation_test=True, nperms=4, perm_idx=d["pidx"], **kw)


# name: (call, the order in which its checks fire)
HOST = {
    "bulkscan": (lambda B, d: B.bulkscan(d["Y"], d["G"], d["K"], **d["kw"]), ["method", "shape", "n", "covar"]),
    "bulkscan_null": (lambda B, d: B.bulkscan_null(d["Y"], d["G"], d["K"], **d["kw"]), ["shape", "n", "covar"]),
    "bulkscan_null_grid": (lambda B, d: B.bulkscan_null_grid(d["Y"], d["G"], d["K"], [0.1, 0.5], **d["kw"]), ["shape", "n", "covar"]),
    "bulkscan_alt_grid": (lambda B, d: B.bulkscan_alt_grid(d["Y"], d["G"], d["K"], [0.1, 0.5], **d["kw"]), ["shape", "n", "covar"]),
    "bulkscan_alt_exact": (lambda B, d: B.bulkscan_alt_exact(d["Y"], d["G"], d["K"], **d["kw"]), ["shape", "n", "covar"]),
    "bulkscan_multi": (lambda B, d: B.bulkscan_multi(None, d["Y"], d["G"], d["K"], **d["kw"]), ["method", "shape", "n", "covar"]),
    "bulkscan_reduced": (lambda B, d: B.bulkscan_reduced(d["Y"], d["G"], d["K"], threshold=1.0, **d["kw"]),
                         ["method", "shape", "n", "covar"]),
    "scan": (_scan, ["shape", "n", "covar", "perm_idx"]),
    "bulkscan_perms": (lambda B, d: B.bulkscan_perms(d["Y"], d["G"], d["K"], nperms=4, perm_idx=d["pidx"], **d["kw"]),
                       ["shape", "n", "covar", "perm_idx"]),
    "bulkscan_loco": (lambda B, d: B.bulkscan_loco(d["Y"], d["G"], CHROM, **d["kw"]), ["method", "shape", "n", "covar"]),
    "bulkscan_loco_reduced": (lambda B, d: B.bulkscan_loco_reduced(d["Y"], d["G"], CHROM, threshold=1.0, **d["kw"]),
                              ["method", "shape", "n", "covar"]),
    "bulkscan_loco_perms": (lambda B, d: B.bulkscan_loco_perms(d["Y"], d["G"], CHROM, nperms=4, perm_idx=d["pidx"], **d["kw"]),
                            ["shape", "covar", "n", "perm_idx"]),
    "bulkscan_multidf": (lambda B, d: B.bulkscan_multidf(d["Y"], d["G"], d["K"], 2, **d["kw"]), ["shape", "covar", "method", "n"]),
    "transform_rotation": (lambda B, d: B.transform_rotation(d["Y"], d["G"], d["K"]), ["shape", "n"]),
}
_LOCO = ("bulkscan_loco", "bulkscan_loco_reduced", "bulkscan_loco_perms")
# weights and the K checks sit with the shapes and covariates they are named after; all three raise the same refusal
_CLASS = {"weights": "covar", "K_rows": "shape", "K_cols": "shape"}


def _applies(name, fault):
    order = HOST[name][1]
    if fault in ("K_rows", "K_cols"):
        return name not in _LOCO and not (name == "transform_rotation" and fault == "K_cols")
    if name == "transform_rotation":
        return fault in order
    return _CLASS.get(fault, fault) in order


def _expected(name, faults):
    order = HOST[name][1]
    first = min(faults, key=lambda f: order.index(_CLASS.get(f, f)))
    if first == "method" and name == "bulkscan_multidf":
        return MULTIDF_METHOD
    return REFUSALS[first]


SINGLE = ["method", "shape", "K_rows", "K_cols", "n", "covar", "weights", "perm_idx"]
PAIRS = [("n", "covar"), ("shape", "n"), ("method", "shape"), ("method", "n"), ("method", "covar"), ("n", "perm_idx"),
         ("K_rows", "n"), ("covar", "perm_idx")]
CASES = [(name, (f,)) for name in HOST for f in SINGLE if _applies(name, f)]
CASES += [(name, pair) for name in HOST for pair in PAIRS if all(_applies(name, f) for f in pair)]


@pytest.mark.parametrize("name,faults", CASES, ids=["%s-%s" % (nm, "+".join(f)) for nm, f in CASES])
def test_host_refusals(no_context, name, faults):
    call = HOST[name][0]
    with pytest.raises(no_context.BulkLMMError) as e:
        call(no_context, _inputs(faults))
    assert (type(e.value), e.value.code, e.value.msg) == (no_context.BulkLMMError, *_expected(name, faults))


# ---- device forms: the checks that fire before any tensor is read ----------------------------------------------------------------
def _dev(torch, name, n=6, method="null-exact"):
    f64 = dict(dtype=torch.float64)
    Y, G, K = torch.zeros((2, n), **f64), torch.zeros((P, n), **f64), torch.zeros((n, n), **f64)
    L_out, h2 = torch.zeros((2, P), **f64), torch.zeros(2, **f64)
    import bulklmm_jl_amd as B
    if name == "bulkscan_loco_dev":
        return lambda: B.bulkscan_loco_dev(None, Y, G, [0, 2, 4], L_out, None, method=method)
    if name == "bulkscan_loco_reduced_dev":
        return lambda: B.bulkscan_loco_reduced_dev(None, Y, G, [0, 2, 4], None, None, None, None, None, method=method)
    if name == "bulkscan_loco_perms_dev":
        return lambda: B.bulkscan_loco_perms_dev(None, Y, G, [0, 2, 4], None, None, None, None, nperms=4)
    if name == "bulkscan_multidf_dev":
        return lambda: B.bulkscan_multidf_dev(None, Y, G, K, 2, torch.zeros((2, P // 2), **f64), h2, method=method)
    raise KeyError(name)


DEV = [("bulkscan_loco_dev", ("method",)), ("bulkscan_loco_dev", ("n",)), ("bulkscan_loco_dev", ("n", "method")),
       ("bulkscan_loco_reduced_dev", ("method",)), ("bulkscan_loco_reduced_dev", ("n",)), ("bulkscan_loco_reduced_dev", ("n", "method")),
       ("bulkscan_loco_perms_dev", ("n",)),
       ("bulkscan_multidf_dev", ("method",)), ("bulkscan_multidf_dev", ("n",)), ("bulkscan_multidf_dev", ("method", "n"))]


@pytest.mark.parametrize("name,faults", DEV, ids=["%s-%s" % (nm, "+".join(f)) for nm, f in DEV])
def test_device_refusals(no_context, name, faults):
    torch = pytest.importorskip("torch")
    call = _dev(torch, name, n=2049 if "n" in faults else 6, method="nope" if "method" in faults else "null-grid")
    with pytest.raises(no_context.BulkLMMError) as e:
        call()
    want = REFUSALS[faults[0]] if not (faults[0] == "method" and name == "bulkscan_multidf_dev") else MULTIDF_METHOD
    assert (type(e.value), e.value.code, e.value.msg) == (no_context.BulkLMMError, *want)


# ---- the two divergences the device forms had --------------------------------------------------------------------------------------
class _Lib:
    """Stands in for the library: records every call, returns success (blmm_rotated_rows: 0 rows)."""

    def __init__(self):
        self.calls = {}

    def __getattr__(self, name):
        def f(*args):
            self.calls[name] = args
            return 0
        return f


class _Ctx:
    h, ndev = None, 1

    def __init__(self):
        self.lib = _Lib()

    def check(self, rc):
        assert rc == 0


def _dev_unknown_method(B, torch, name, ctx, method="nope", h2_grid=None):
    f64 = dict(dtype=torch.float64)
    n = 6
    Y, G, K = torch.zeros((2, n), **f64), torch.zeros((P, n), **f64), torch.zeros((n, n), **f64)
    L_out, h2 = torch.zeros((2, P), **f64), torch.zeros(2, **f64)
    mx, arg = torch.zeros(2, **f64), torch.zeros(2, dtype=torch.int64)
    kw = dict(method=method, h2_grid=h2_grid)
    if name == "bulkscan_dev":
        return B.bulkscan_dev(ctx, Y, G, K, L_out, h2, **kw)
    if name == "bulkscan_reduced_dev":
        return B.bulkscan_reduced_dev(ctx, Y, G, K, mx, arg, h2, **kw)
    if name == "bulkscan_reduced_async":
        return B.bulkscan_reduced_async(ctx, Y, G, K, mx, arg, h2, None, **kw)
    if name == "bulkscan_prerotated_dev":
        return B.bulkscan_prerotated_dev(ctx, Y, torch.zeros((1, 0, P), **f64), P, P, L_out, h2, **kw)
    if name == "bulkscan_loco_dev":
        return B.bulkscan_loco_dev(ctx, Y, G, [0, 2, 4], L_out, None, **kw)
    if name == "bulkscan_loco_reduced_dev":
        return B.bulkscan_loco_reduced_dev(ctx, Y, G, [0, 2, 4], mx, arg, None, None, None, **kw)
    if name == "bulkscan_multidf_dev":
        return B.bulkscan_multidf_dev(ctx, Y, G, K, 2, torch.zeros((2, P // 2), **f64), h2, **kw)
    raise KeyError(name)


@pytest.mark.parametrize("name", ["bulkscan_dev", "bulkscan_reduced_dev", "bulkscan_reduced_async", "bulkscan_prerotated_dev"])
def test_device_forms_refuse_an_unknown_method_as_the_host_forms_do(no_context, name):
    """These four once raised a bare KeyError from the method table."""
    torch = pytest.importorskip("torch")
    ctx = _Ctx()
    with pytest.raises(no_context.BulkLMMError) as e:
        _dev_unknown_method(no_context, torch, name, ctx)
    assert (e.value.code, e.value.msg) == REFUSALS["method"]
    assert not ctx.lib.calls


# the library function each form hands its grid to, and the argument position of ngrid there
_NGRID_AT = {"bulkscan_dev": ("blmm_bulkscan_dev", 12), "bulkscan_reduced_dev": ("blmm_bulkscan_reduced_dev", 12),
             "bulkscan_reduced_async": ("blmm_bulkscan_reduced_async", 12),
             "bulkscan_prerotated_dev": ("blmm_bulkscan_prerotated_dev", 10),
             "bulkscan_loco_dev": ("blmm_bulkscan_loco_dev", 14), "bulkscan_loco_reduced_dev": ("blmm_bulkscan_loco_reduced_dev", 14),
             "bulkscan_multidf_dev": ("blmm_bulkscan_multidf_dev", 13)}


@pytest.mark.parametrize("name", sorted(_NGRID_AT))
@pytest.mark.parametrize("grid", [[0.1, 0.2, 0.3], [[0.1, 0.2, 0.3]], [[0.1], [0.2], [0.3]]])
def test_device_forms_ravel_the_grid(no_context, name, grid):
    """A 2-D h2 grid counts its entries, as in the host forms (it once passed ngrid = its row count)."""
    torch = pytest.importorskip("torch")
    ctx = _Ctx()
    _dev_unknown_method(no_context, torch, name, ctx, method="null-grid", h2_grid=grid)
    fn, at = _NGRID_AT[name]
    assert ctx.lib.calls[fn][at] == 3


def test_bulkscan_multi_and_bulkscan_into_ravel_the_grid(no_context):
    grid = [[0.1, 0.2, 0.3]]
    Y, G, K = np.zeros((6, 2)), np.zeros((6, P)), np.eye(6)
    ctx = _Ctx()
    no_context.bulkscan_multi(ctx, Y, G, K, h2_grid=grid)
    assert ctx.lib.calls["blmm_bulkscan_multi"][13] == 3
    no_context.bulkscan_into(ctx, no_context._lib.BLMM_NULL_GRID, Y, G, K, np.empty((P, 2), order="F"), h2_grid=grid)
    assert ctx.lib.calls["blmm_bulkscan"][12] == 3
