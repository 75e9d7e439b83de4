"""The IPM driver is written once: `MadNLPSolver` holds the algorithm (regular!, the inertia correction loop, the line searches,
the second-order correction, restore!, robust!), a back-end supplies `ipm.BACKEND_PRIMITIVES`.  These tests pin that split, so
that a copy of the control flow cannot grow back in the device class and a new primitive cannot fall back to numpy on device
tensors without a test failing.  No GPU: `ipm_dev` imports without one."""
import inspect
import re

from madnlp_jl_amd.ipm import BACKEND_PRIMITIVES, MadNLPSolver
from madnlp_jl_amd.ipm_dev import DeviceMadNLPSolver


def test_the_device_class_holds_no_copy_of_the_control_flow():
    for name in ("filter_line_search", "_second_order_correction", "inertia_correction", "_solve_newton", "_dx", "_dy", "_dzl",
                 "_dzu", "filter_line_search_RR", "restore", "robust", "regular", "_next_perturbation", "_trial", "_alpha_min"):
        assert name in MadNLPSolver.__dict__, name
        assert name not in DeviceMadNLPSolver.__dict__, name
    for name in ("dv", "pv", "w1v", "w4v"):      # the device KKT vectors are self.d, self.p, self._w1, self._w4
        assert not re.search(rf"\bself\.{name}\b", inspect.getsource(DeviceMadNLPSolver)), name


def test_one_correction_loop_for_the_three_methods():
    assert "_inertia_correction_free" not in MadNLPSolver.__dict__
    assert "_inertia_correction_ignore" not in MadNLPSolver.__dict__
    for method in ("inertia_based", "inertia_free", "ignore"):
        assert "_trial_" + method in MadNLPSolver.__dict__


def test_every_backend_primitive_is_overridden_by_the_device_class():
    assert len(set(BACKEND_PRIMITIVES)) == len(BACKEND_PRIMITIVES)
    for name in BACKEND_PRIMITIVES:
        assert name in MadNLPSolver.__dict__, name
        assert name in DeviceMadNLPSolver.__dict__, name


# methods of the host class that use numpy and are NOT primitives, each for a reason: they run before the upload (construction,
# initialize!), belong to the host-only inertia-free corrector, or to the host quasi-Newton mirror (the device class replaces
# `eval_lag_hess`, their only caller)
HOST_ONLY = {"__init__", "initialize", "_initialize_dual_least_squares", "x_lr", "x_ur", "xl_r", "xu_r", "zl_r", "zu_r",
             "_set_g_ifr", "_set_aug_rhs_ifr", "_ifr_solves", "_trial_inertia_free", "_model_jtprod", "_eval_lag_hess_qn"}


def test_numpy_is_used_in_primitives_only():
    """Shared control flow must not touch a vector except through a primitive: any method of the host class whose body names
    numpy or slices / fills a vector in place is a declared primitive (or host-only, see above)."""
    for name, fn in MadNLPSolver.__dict__.items():
        if isinstance(fn, property):
            fn = fn.fget
        if not inspect.isfunction(fn) or name in HOST_ONLY or name in BACKEND_PRIMITIVES:
            continue
        src = inspect.getsource(fn)
        body = src.split('"""')[2] if src.count('"""') >= 2 else src      # docstrings may speak of numpy
        assert not re.search(r"\bnp\.|\[:\]|\.values\b|\.primal\(\)|\.dual\(\)|\.dual_lb\(\)|\.dual_ub\(\)", body), name
