"""The device interpreter of expression tapes (`mnk_tape_*`, csrc/tape_eval.hip) against the independent 60-digit reference of
tests/tape_reference.py: random patterns entry by entry within a running-error bound, the kernel at its full LDS footprint
(32 slots + 8 variables + 8 parameters, 36 Hessian pairs) on exact integers, and the library functions at edge arguments.
tests/test_tape_reference_cpu.py holds the numpy interpreter to the same references."""
import functools

import numpy as np
import pytest
from mpmath import mpf

from madnlp_jl_amd import tape_model as T
from tests import tape_reference as R
from tests.test_hip_tape import device_eval, make_callbacks

OBJ, GRAD, CONS, JAC, HESS = 1, 2, 4, 8, 16      # the bits of mnk_tape_extended


@pytest.fixture()
def gpu_ctx():
    torch = pytest.importorskip("torch")
    import madnlp_jl_amd as mj
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    st = torch.cuda.Stream()       # NOT torch's current stream: the callbacks must not depend on torch's stream order
    ctx = mj.HipContext(0, stream=st.cuda_stream)
    yield ctx
    ctx.close()


def device_structure(cb, M):
    """(jac_I, jac_J, hess_I, hess_J) as the library reports them"""
    import madnlp_jl_amd as mj
    st = [np.zeros(max(len(a), 1), dtype=np.int32) for a in (M.jac_I, M.jac_J, M.hess_I, M.hess_J)]
    assert mj.lib().mnk_tape_get_structure(cb._h, *[a.ctypes.data for a in st]) == 0
    return [a[:len(b)] for a, b in zip(st, (M.jac_I, M.jac_J, M.hess_I, M.hess_J))]


def launch_mask(M):
    """which callback launches hold a tape with an opcode from 16 on, from the opcodes of the launch's tapes"""
    mask = 0
    for p in M.patterns:
        for w, t in enumerate(p.tapes):
            if t.nout and R.opcodes(t) & T.OP_EXTENDED:
                mask |= HESS if w == 2 else ((OBJ, GRAD) if p.kind == 0 else (CONS, JAC))[w]
    return mask


# ------------------------------------------------------------------------------------------------- a. random patterns
@functools.lru_cache(maxsize=None)
def random_model():
    M, x, pats = R.random_device_model()
    for pat in pats:                 # the reference of the NREF rows: value and the kept derivatives, computed once
        d1, d2 = pat.tapes[1].out_j.tolist(), list(zip(pat.tapes[2].out_j.tolist(), pat.tapes[2].out_l.tolist()))
        pat.ref = {r: ([R.derivative(pat.tree, *pat.points[r], [0] * pat.k)],
                       [R.derivative(pat.tree, *pat.points[r], R.orders_of(pat.k, j)) for j in d1],
                       [R.derivative(pat.tree, *pat.points[r], R.orders_of(pat.k, j, l)) for j, l in d2]) for r in pat.ref_rows}
    return M, x, pats


def by_key(I, J):
    where = {}
    for e, key in enumerate(zip(I.tolist(), J.tolist())):
        where.setdefault(key, []).append(e)
    return where


def summed_reference(contributions):
    """(sum, bound) of contributions (reference, bound) added one after the other from 0.0: their bounds plus the roundings of
    the partial sums"""
    total = sum(ref for ref, _ in contributions)
    size = sum(abs(ref) + b for ref, b in contributions)
    return total, sum(b for _, b in contributions) + (len(contributions) - 1) * (R.U / 2) * size


def check_against_reference(M, pats, x, y, sigma, dev, structure):
    f, terms, g, c, jv, hv = dev
    jac_at, hess_at = by_key(structure[0], structure[1]), by_key(structure[2], structure[3])
    grad_refs, cons_refs, jac_refs, hess_refs = {}, {}, {}, {}
    grad_all, cons_all = {}, {}              # destination -> number of contributions, reference rows or not
    tbase, worst = 0, 0.0
    for pat in pats:
        for r in range(pat.R):
            for j in (pat.tapes[1].out_j.tolist() if pat.kind == 0 else ()):
                grad_all[pat.var_index[r, j]] = grad_all.get(pat.var_index[r, j], 0) + 1
            if pat.kind == 1:
                cons_all[pat.rows[r]] = cons_all.get(pat.rows[r], 0) + 1
        for r in pat.ref_rows:
            xs, ps = pat.points[r]
            gv = pat.var_index[r].tolist()
            weight = float(sigma) if pat.kind == 0 else float(y[pat.rows[r]])
            outs = [R.run_tape(pat.tapes[0], xs, ps), R.run_tape(pat.tapes[1], xs, ps), R.run_tape(pat.tapes[2], xs, ps, weight=weight)]
            bound = lambda w, o: outs[w][o][3]  # noqa: E731
            if pat.kind == 0:
                got = terms[tbase + r]
                assert R.within(got, pat.ref[r][0][0], bound(0, 0)), ("term", pat.tree, xs, ps, got)
                worst = max(worst, float(abs(mpf(float(got)) - pat.ref[r][0][0]) / bound(0, 0))) if bound(0, 0) > 0 else worst
                for o, j in enumerate(pat.tapes[1].out_j.tolist()):
                    grad_refs.setdefault(gv[j], []).append((pat.ref[r][1][o], bound(1, o)))
            else:
                cons_refs.setdefault(pat.rows[r], []).append((pat.ref[r][0][0], bound(0, 0)))
                for o, j in enumerate(pat.tapes[1].out_j.tolist()):
                    jac_refs.setdefault((pat.rows[r], gv[j]), []).append((pat.ref[r][1][o], bound(1, o), pat.tree, xs, ps))
            for o, (j, l) in enumerate(zip(pat.tapes[2].out_j.tolist(), pat.tapes[2].out_l.tolist())):
                key = (max(gv[j], gv[l]), min(gv[j], gv[l]))
                hess_refs.setdefault(key, []).append((weight * pat.ref[r][2][o], bound(2, o), pat.tree, xs, ps))
        tbase += pat.R if pat.kind == 0 else 0
    # COO entries: the reference's own scatter, read through the structure the device reports.  Entries of one (row, column)
    # come in pattern order on both sides (the COO layout is pattern-major).
    checked = 0
    for refs, at, vals, what in ((jac_refs, jac_at, jv, "jac"), (hess_refs, hess_at, hv, "hess")):
        for key, contrib in refs.items():
            assert len(at[key]) >= len(contrib), (what, key)
            if len(at[key]) != len(contrib):          # a (row, column) other, unreferenced pattern rows feed too
                continue
            for e, (ref, b, *info) in zip(at[key], contrib):
                assert R.within(vals[e], ref, b), (what, key, info, vals[e], ref, b)
                worst = max(worst, float(abs(mpf(float(vals[e])) - ref) / b)) if b > abs(ref) * mpf(2) ** -60 else worst
                checked += 1
    for refs, count, vals, what in ((grad_refs, grad_all, g, "grad"), (cons_refs, cons_all, c, "cons")):
        for dest, contrib in refs.items():
            if len(contrib) != count[dest]:
                continue
            total, b = summed_reference([t[:2] for t in contrib])
            assert R.within(vals[dest], total, b), (what, dest, vals[dest], total, b)
            checked += 1
    return checked, worst


def check_against_host(M, pats, x, y, sigma, dev):
    """the existing rule for ALL rows: bit-identical where no library function feeds the entry, 1e-13 of the vector's scale else"""
    f, terms, g, c, jv, hv = dev
    host = (M.obj_terms(x), M.grad(x), M.cons(x), M.jac_coord(x), M.hess_coord(x, y, sigma))
    plain = lambda t: not (R.opcodes(t) & R.LIBRARY_OPS)  # noqa: E731
    tm = np.concatenate([np.full(p.R, plain(p.tapes[0])) for p in pats if p.kind == 0])
    jm = np.concatenate([np.full(p.R * p.tapes[1].nout, plain(p.tapes[1])) for p in pats if p.kind == 1])
    hm = np.concatenate([np.full(p.R * p.tapes[2].nout, plain(p.tapes[2])) for p in pats])
    gm, cm = np.ones(M.n, dtype=bool), np.ones(M.m, dtype=bool)
    for p in pats:
        if p.kind == 0 and not plain(p.tapes[1]):
            gm[p.var_index.ravel()] = False
        if p.kind == 1 and not plain(p.tapes[0]):
            cm[p.rows] = False
    for name, got, ref, mask in (("terms", terms, host[0], tm), ("grad", g, host[1], gm), ("cons", c, host[2], cm),
                                 ("jac", jv, host[3], jm), ("hess", hv, host[4], hm)):
        assert np.array_equal(got[mask], ref[mask]), name
        assert np.abs(got - ref).max() <= 1e-13 * np.abs(ref).max(), name
    assert abs(f - M.obj(x)) <= 1e-13 * np.abs(host[0]).sum()
    assert (c[-3:] == 0.0).all()                  # rows no pattern feeds
    return sum(int(m.sum()) for m in (tm, jm, hm))


@pytest.mark.gpu
def test_random_patterns_match_the_independent_reference_on_the_device(gpu_ctx):
    from madnlp_jl_amd.ipm_dev import DeviceTapeCallbacks
    M, x, pats = random_model()
    assert len(pats) == 24 and [p.kind for p in pats] == [0, 1] * 12
    assert {p.R for p in pats} == {1, R.BS, R.BS + 1, 3 * R.BS - 1}
    assert set().union(*(R.opcodes(t) for p in pats for t in p.tapes)) == set(range(10)) | set(range(16, 25))
    fed = np.bincount(np.concatenate([p.rows for p in pats if p.kind == 1]), minlength=M.m)
    assert fed.max() == 3 and (fed == 2).sum() >= R.BS - 1 and (fed[-3:] == 0).all()
    cb, K = make_callbacks(gpu_ctx, M, DeviceTapeCallbacks)
    structure = device_structure(cb, M)
    for got, own in zip(structure, (M.jac_I, M.jac_J, M.hess_I, M.hess_J)):
        assert np.array_equal(got, own)
    assert cb.extended() == launch_mask(M)
    rng = np.random.default_rng(12)
    for sigma in (1.0, 0.0, 0.37):
        y = rng.standard_normal(M.m)
        y[::7] = 0.0
        dev = device_eval(gpu_ctx, cb, M, x, y, sigma)
        checked, worst = check_against_reference(M, pats, x, y, sigma, dev, structure)
        exact = check_against_host(M, pats, x, y, sigma, dev)
        print(f"sigma {sigma}: {checked} entries against the reference, worst |device - reference| / bound = {worst:.3f}; "
              f"{exact} entries bit-identical to the host interpreter")
        assert checked >= 24 * 8
    cb.close()
    K.close()


# ------------------------------------------------------------------------------------------------- b. the full footprint
@pytest.mark.gpu
def test_full_footprint_pattern_gives_the_exact_integers_on_the_device(gpu_ctx):
    """each of the three tapes of the k = 8, q = 8 pattern needs SLOT_MAX slots: 48 LDS columns, 48 KiB per workgroup, in the
    base kernel (obj, grad) and in the extended one (cons, jac, hess), next to a one-slot pattern in the same launches"""
    from madnlp_jl_amd.ipm_dev import DeviceTapeCallbacks
    M = R.footprint_model()
    R.assert_footprint_shape(M)
    cb, K = make_callbacks(gpu_ctx, M, DeviceTapeCallbacks)
    assert cb.extended() == launch_mask(M) == CONS | JAC | HESS
    structure = device_structure(cb, M)
    for got, own in zip(structure, (M.jac_I, M.jac_J, M.hess_I, M.hess_J)):
        assert np.array_equal(got, own)
    for x, y, w in R.footprint_points(M):
        f, terms, g, c, jv, hv = device_eval(gpu_ctx, cb, M, x, y, w)
        R.check_footprint_outputs(M, x, y, w, f, g, c, jv, hv, structure)
        assert np.array_equal(terms, M.obj_terms(x))
    cb.close()
    K.close()


# ------------------------------------------------------------------------------------------------- c. edge arguments
# Entries where the device's library and the 60-digit value of the tape legitimately differ in class:
# {(function, tape, output, arguments): (class on the device, class of the reference)}; DESIGN.md section 14 lists them.
DEVICE_CLASS_DIFFERENCES = {}


@pytest.mark.gpu
def test_library_functions_at_edge_arguments_on_the_device(gpu_ctx):
    """class (NaN, +-Inf, signed zero, finite) of every value, first and second derivative against the 60-digit value of the
    same tape under IEEE range rules, then the finite values within the bound; the numpy interpreter on the same entries"""
    from madnlp_jl_amd.ipm_dev import DeviceTapeCallbacks
    M, x, names = R.edge_model()
    cb, K = make_callbacks(gpu_ctx, M, DeviceTapeCallbacks)
    y = np.ones(M.m)
    _, _, _, c, jv, hv = device_eval(gpu_ctx, cb, M, x, y, 1.0)
    cb.close()
    K.close()
    classes, misses = R.edge_findings(M, x, c, jv, hv, names)
    with np.errstate(all="ignore"):
        host_classes, host_misses = R.edge_findings(M, x, M.cons(x), M.jac_coord(x), M.hess_coord(x, y), names)
    for key, val in classes.items():
        print("device class differs:", key, val)
    for miss in misses:
        print("device value outside the bound:", miss)
    assert host_classes == {} and host_misses == []
    assert misses == []
    assert classes == DEVICE_CLASS_DIFFERENCES
    for ip, name in enumerate(names):             # at most 5 % of a function's rows
        rows = {key[3] for key in DEVICE_CLASS_DIFFERENCES if key[0] == name}
        assert len(rows) <= 0.05 * M.patterns[ip].R, name
