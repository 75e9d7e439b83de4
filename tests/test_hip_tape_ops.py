"""The device interpreter (`mnk_tape_*`, csrc/tape_eval.hip) on the tape vocabulary beyond + - * / and sin cos exp log sqrt --
real powers, tan atan tanh, abs_ sign step minimum maximum -- against the numpy interpreter (`madnlp_jl_amd.tape_model`): values,
which of the two interpreter kernels a callback launch runs (`mnk_tape_extended`), malformed tapes, and three NLPs with closed-form
optima end to end in `DeviceMadNLPSolver`.  Model builders: tests/tape_ops_cases.py."""
import ctypes as C

import numpy as np
import pytest

from madnlp_jl_amd import tape_model as T
from madnlp_jl_amd.tape_model import V, TapeModel
from tests import tape_ops_cases as K
from tests.test_hip_tape import _pattern_args, _set, device_eval, make_callbacks
from tests.test_tape_model_cpu import _options, integer_model

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


# ------------------------------------------------------------------------------------------------- 1. device vs host interpreter
@pytest.mark.gpu
def test_device_interpreter_matches_the_host_interpreter_on_the_new_operations(gpu_ctx):
    """Selection and arithmetic patterns: bit-identical in all five callbacks, also where they share a launch with patterns of
    pow / tan / atan / tanh; those: another math library, 1e-13 of the vector's scale -- the rule of
    test_device_interpreter_matches_the_host_interpreter."""
    from madnlp_jl_amd.ipm_dev import DeviceTapeCallbacks
    M = K.ops_edge_model()
    assert sorted({p.R for p in M.patterns}) == [1, K.BS, K.BS + 1, 3 * K.BS - 1] and {p.k for p in M.patterns} == {1, 2, 3, 4, 5}
    ops = lambda i: {op for t in M.patterns[i].tapes for op in t.code[:, 0].tolist()}  # noqa: E731
    functions = {T.OP_POW, T.OP_TAN, T.OP_ATAN, T.OP_TANH}
    assert all(ops(i) & {T.OP_ABS, T.OP_SIGN, T.OP_STEP, T.OP_MIN, T.OP_MAX} and not ops(i) & functions for i in K.SEL_PATTERNS)
    assert set().union(*(ops(i) for i in K.EXT_PATTERNS)) >= functions and set().union(*(ops(i) for i in range(8))) >= T.OP_EXTENDED
    assert all(max(ops(i)) <= T.OP_NEG for i in K.ARITH_PATTERNS)
    fed = lambda idx: np.bincount(np.concatenate([M.patterns[i].rows for i in idx if M.patterns[i].kind == 1]), minlength=M.m) > 0  # noqa: E731
    assert (fed(K.EXT_PATTERNS) & fed(K.SEL_PATTERNS)).any() and (fed(K.EXT_PATTERNS) & fed(K.ARITH_PATTERNS)).any()
    cb, Kd = make_callbacks(gpu_ctx, M, DeviceTapeCallbacks)
    assert cb.extended() == OBJ | GRAD | CONS | JAC | HESS
    jmask, hmask, rmask, tmask, vmask = K.ops_edge_masks(M)
    for mask in (jmask, hmask, rmask, tmask, vmask):
        assert mask.sum() and (~mask).sum()
    assert (rmask & fed(K.SEL_PATTERNS)).sum() >= 100
    rng = np.random.default_rng(9)
    for sigma in (1.0, 0.0, 0.37):
        x, y = rng.uniform(0.5, 1.5, M.n), rng.standard_normal(M.m)
        y[::7] = 0.0
        f, terms, g, c, jv, hv = device_eval(gpu_ctx, cb, M, x, y, sigma)
        rt, rg, rc, rj, rh = M.obj_terms(x), M.grad(x), M.cons(x), M.jac_coord(x), M.hess_coord(x, y, sigma)
        assert np.array_equal(terms[tmask], rt[tmask])
        assert np.array_equal(g[vmask], rg[vmask])
        assert np.array_equal(c[rmask], rc[rmask])
        assert np.array_equal(jv[jmask], rj[jmask])
        assert np.array_equal(hv[hmask], rh[hmask])
        for name, got, ref in (("terms", terms, rt), ("grad", g, rg), ("cons", c, rc), ("jac", jv, rj), ("hess", hv, rh)):
            err = np.abs(got - ref).max()
            print(f"sigma {sigma} {name}: max |got - ref| = {err:.3e}, scale {np.abs(ref).max():.3e}")
            assert err <= 1e-13 * np.abs(ref).max()
        assert abs(f - M.obj(x)) <= 1e-13 * np.abs(rt).sum()
    cb.close()
    Kd.close()


@pytest.mark.gpu
def test_selection_operations_give_the_hand_written_values_on_the_device(gpu_ctx):
    """signed zeros and ties as VARIABLES (tests/test_tape_ops_cpu.py holds the host interpreter to the same numbers)"""
    from madnlp_jl_amd.ipm_dev import DeviceTapeCallbacks
    M = K.selection_model()
    cb, Kd = make_callbacks(gpu_ctx, M, DeviceTapeCallbacks)
    assert cb.extended() == CONS | JAC           # (it has no Hessian entry: no such launch)
    x = np.array(K.SEL_A + K.SEL_B)
    _, _, _, c, jv, hv = device_eval(gpu_ctx, cb, M, x, np.ones(M.m), 1.0)
    assert c.tolist() == [0.0, 0.0, 2.0, 1.5, 3.0, 0.0, 0.0, 1.0, 1.0, -1.0, 1.0, 1.0, 1.0, 1.0, 0.0,
                          0.0, 0.0, 2.0, -2.5, -3.0, 0.0, 0.0, 2.0, 1.5, 4.0]
    assert jv.tolist() == [0.0, 0.0, 1.0, 1.0, -1.0, 1.0, 1.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0,
                           1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]
    assert np.array_equal(jv, M.jac_coord(x)) and len(hv) == 0
    cb.close()
    Kd.close()


# ------------------------------------------------------------------------------------------------- 2. kernel selection
@pytest.mark.gpu
def test_only_launches_with_an_opcode_from_16_on_run_the_extended_kernel(gpu_ctx):
    from madnlp_jl_amd.ipm_dev import DeviceTapeCallbacks
    for M, want in ((T.acopf_tape_model("case30"), 0), (integer_model(), 0), (K.tanh_in_one_constraint_model(), CONS | JAC | HESS)):
        cb, Kd = make_callbacks(gpu_ctx, M, DeviceTapeCallbacks)
        assert cb.extended() == want, (M.name, cb.extended())
        cb.close()
        Kd.close()


# ------------------------------------------------------------------------------------------------- 3. malformed tapes
@pytest.mark.gpu
def test_unassigned_opcodes_and_an_unwritten_pow_operand_are_refused(gpu_ctx):
    import madnlp_jl_amd as mj
    from madnlp_jl_amd import _lib as L
    lib = mj.lib()
    M = TapeModel(3, 1, np.ones(3), 0.5, 2.0, 0.0, 0.0)
    M.add_constraint(V(0) ** V(1) + V(2) * V(0), np.array([0]), np.array([[0, 1, 2]]))
    M.finalize()
    p = M.patterns[0]
    assert p.tapes[0].code[0, 0] == T.OP_POW and p.tapes[0].nslot == 2 and p.tapes[0].code[0, 1] == 0
    h = C.c_void_p()
    L.check(lib.mnk_tape_create(gpu_ctx.handle, M.n, M.m, C.byref(h)), "mnk_tape_create")
    bad = [(_set("code0", (0, 0), op), b"bad opcode") for op in (11, 15, 25, -1)]
    bad += [(_set("code1", (0, 0), 12), b"bad opcode"), (_set("code2", (0, 0), 1 << 20), b"bad opcode")]
    bad += [(_set("code0", (0, 3), T.KIND_SLOT << 24 | 1), b"slot 1 is read before it is written")]      # pow reads `b`
    for edit, msg in bad:
        args, keep = _pattern_args(p, edit)
        rc = lib.mnk_tape_add_pattern(h, *args)
        err = lib.mnk_last_error_string()
        assert rc != 0 and msg in err, (msg, rc, err)
    mask = C.c_int(-1)
    assert lib.mnk_tape_extended(h, C.byref(mask)) != 0          # not finalized
    args, keep = _pattern_args(p)
    assert lib.mnk_tape_add_pattern(h, *args) == 0
    assert lib.mnk_tape_finalize(h) == 0
    assert lib.mnk_tape_extended(h, C.byref(mask)) == 0 and mask.value == CONS | JAC | HESS
    assert lib.mnk_tape_extended(h, None) != 0
    assert lib.mnk_tape_destroy(h) == 0


# ------------------------------------------------------------------------------------------------- 4. end to end
@pytest.mark.gpu
@pytest.mark.parametrize("name,launches", [("hinge", OBJ | GRAD | HESS), ("powers", OBJ | GRAD | CONS | JAC | HESS),
                                           ("tanh", OBJ | GRAD | CONS | JAC | HESS)])
def test_device_resident_runs_reach_the_closed_form_optimum(gpu_ctx, name, launches):
    """`DeviceMadNLPSolver` against the host driver with the numpy interpreter on the SAME HIP back end (equal iteration,
    factorization and back-solve counts, x within 1e-7) and against the closed form (sqrt(tol) = 1e-3), in the shape of
    test_device_resident_tape_acopf_run.  The hinge problem has `maximum` in its objective and linear constraints: its cons and
    jac launches run the base kernel, the other three the extended one."""
    import madnlp_jl_amd as mj
    from madnlp_jl_amd.ipm import MadNLPSolver
    from madnlp_jl_amd.ipm_dev import DeviceMadNLPSolver, DeviceTapeCallbacks
    M, xstar = K.NLPS[name]()

    def factory(info):
        return mj.SparseCondensedKKTSystem(info["n"], info["m"], M.jac_I, M.jac_J, M.hess_I, M.hess_J,
                                           info["ind_ineq"], info["ind_lb"], info["ind_ub"], ctx=gpu_ctx,
                                           opt_linear_solver=mj.HipSolverOptions(lapack_algorithm=mj.BUNCHKAUFMAN),
                                           device_kkt_ops=True)
    sh = MadNLPSolver(M, factory, _options(tol=1e-6), sparse=True)
    sh.solve()
    sd = DeviceMadNLPSolver(M, factory, _options(tol=1e-6))
    sd.solve()
    assert isinstance(sd.cb, DeviceTapeCallbacks)
    assert sd.cb.extended() == launches
    x = sd.host_state()[0]
    counts = lambda s: (s.cnt.k, s.cnt.factorization_cnt, s.cnt.backsolve_cnt)  # noqa: E731
    print(name, sd.status, "device counts", counts(sd), "host counts", counts(sh), "device - host", np.abs(x - sh.x).max(),
          "device - closed form", np.abs(x[:M.n] - xstar).max())
    assert sd.status == sh.status == "SOLVE_SUCCEEDED"
    assert counts(sd) == counts(sh)
    np.testing.assert_allclose(x, sh.x, rtol=0, atol=1e-7 * max(1.0, np.abs(sh.x).max()))
    assert np.abs(x[:M.n] - xstar).max() <= 1e-3
    sd.cb.close(); sd.K.close(); sd.kkt.close()
    sh.kkt.close()
