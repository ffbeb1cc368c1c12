"""Drop-in check of the host bindings against the reference's own signatures, read as TEXT: every keyword argument of
bulkscan / bulkscan_null / bulkscan_null_grid / bulkscan_alt_grid (src/bulkscan.jl:81-124,188-219,321-346,428-451) and of
the four scan methods (src/scan.jl:94-199) must be accepted by the Julia binding (bulklmm.jl_amd/julia/BulkLMMHIP.jl, the
method with the same positional arity) and by the Python mirror (bulklmm.jl_amd/api.py).  The reference's signatures are
stored as data, tests/golden/reference_signatures.json ({file: {function: [[n_positional, [keywords]], ...]}}), which this
module's parser wrote from the reference's sources:  python tests/test_binding_kwargs.py <reference checkout>"""
import inspect
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGS = os.path.join(ROOT, "tests", "golden", "reference_signatures.json")


def julia_methods(path):
    """{name: [(n_positional, {kwargs}), ...]} for every `function name(...)` of a Julia file."""
    txt = open(path).read()
    txt = re.sub(r"#=.*?=#", "", txt, flags=re.S)
    txt = "\n".join(line.split("#", 1)[0] if '"' not in line.split("#", 1)[0] or line.count('"') % 2 == 0 else line
                    for line in txt.splitlines())
    out = {}
    for mt in re.finditer(r"^function\s+([A-Za-z_][\w!]*)\s*\(", txt, flags=re.M):
        i = mt.end()
        depth, j = 1, i
        while depth and j < len(txt):
            depth += txt[j] in "([{"
            depth -= txt[j] in ")]}"
            j += 1
        sig = txt[i:j - 1]
        # split at top-level ';' and ','
        parts, cur, d, semi = [[]], "", 0, False
        for ch in sig:
            if ch in "([{":
                d += 1
            elif ch in ")]}":
                d -= 1
            if d == 0 and ch in ",;":
                parts[-1].append(cur.strip())
                cur = ""
                if ch == ";":
                    parts.append([])
                continue
            cur += ch
        parts[-1].append(cur.strip())
        pos = [a for a in parts[0] if a]
        kws = set()
        for a in (parts[1] if len(parts) > 1 else []):
            if a:
                kws.add(re.split(r"::|=", a, maxsplit=1)[0].strip())
        out.setdefault(mt.group(1), []).append((len(pos), kws))
    return out


REF_FUNCS = {"bulkscan.jl": ["bulkscan", "bulkscan_null", "bulkscan_null_grid", "bulkscan_alt_grid"], "scan.jl": ["scan"]}


def reference_methods(fname):
    """The stored form of julia_methods(<reference>/src/<fname>), restricted to REF_FUNCS[fname]."""
    sigs = json.load(open(SIGS))[fname]
    return {f: [(npos, set(kws)) for npos, kws in methods] for f, methods in sigs.items()}


def test_reference_signatures_parse():
    ref = reference_methods("bulkscan.jl")
    assert {"method", "h2_grid", "nb", "nt_blas", "weights", "prior_variance", "prior_sample_size", "reml", "optim_interval",
            "decomp_scheme", "output_pvals", "chisq_df"} <= ref["bulkscan"][0][1]
    assert set(ref) == set(REF_FUNCS["bulkscan.jl"])
    sc = reference_methods("scan.jl")
    assert len(sc["scan"]) == 4 and all({"profileLL", "markerID", "h2_grid", "method"} <= kw for _, kw in sc["scan"])


def test_julia_binding_accepts_every_reference_keyword():
    mine = julia_methods(os.path.join(ROOT, "bulklmm.jl_amd", "julia", "BulkLMMHIP.jl"))
    for fname, funcs in REF_FUNCS.items():
        ref = reference_methods(fname)
        for f in funcs:
            assert f in mine, f
            for npos, kws in ref[f]:
                cands = [k for n, k in mine[f] if n == npos]
                assert cands, f"{f}: no method with {npos} positional arguments in BulkLMMHIP.jl"
                missing = kws - set().union(*cands)
                assert not missing, f"{f}/{npos}: BulkLMMHIP.jl lacks keyword(s) {sorted(missing)}"


def test_python_mirror_accepts_every_reference_keyword(blmm):
    for fname, funcs in REF_FUNCS.items():
        ref = reference_methods(fname)
        for f in funcs:
            params = set(inspect.signature(getattr(blmm, f)).parameters)
            for _, kws in ref[f]:
                missing = kws - params
                assert not missing, f"api.{f} lacks keyword(s) {sorted(missing)}"


if __name__ == "__main__":
    # regenerate the fixture from a checkout of the reference
    src = os.path.join(sys.argv[1], "src")
    out = {fname: {f: [[npos, sorted(kws)] for npos, kws in julia_methods(os.path.join(src, fname))[f]] for f in funcs}
           for fname, funcs in REF_FUNCS.items()}
    with open(SIGS, "w") as fh:
        fh.write("{\n" + ",\n".join(
            f"  {json.dumps(fname)}: {{\n" + ",\n".join(f"    {json.dumps(f)}: {json.dumps(ms)}" for f, ms in fs.items()) + "\n  }"
            for fname, fs in out.items()) + "\n}\n")
