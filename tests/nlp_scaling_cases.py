"""Models shared by the NLP-scaling tests (tests/test_nlp_scaling_cpu.py, tests/test_hip_nlp_scaling.py)."""
import numpy as np

from madnlp_jl_amd.problems import DenseQPModel, HS15Model


def solcmp(a, b, tol):
    """The suite's `solcmp` rule (tests/test_ipm_oracle.py): max abs difference below tol, or below tol relative to max |b|."""
    d = np.abs(np.asarray(a) - np.asarray(b)).max()
    return d < tol or d / np.abs(b).max() < tol


def jl_isapprox(a, b, rtol=0.0, atol=0.0):
    """Julia's `isapprox` on vectors: norm(a - b) <= max(atol, rtol max(norm(a), norm(b)))."""
    a, b = np.atleast_1d(np.asarray(a, float)), np.atleast_1d(np.asarray(b, float))
    return np.linalg.norm(a - b) <= max(atol, rtol * max(np.linalg.norm(a), np.linalg.norm(b)))


def hs15_from(x0):
    nlp = HS15Model()
    nlp.x0 = np.array(x0, dtype=float)      # on the instance: the class keeps the reference's start
    return nlp


def rescaled_dense_qp(n=20, m=15, n_eq=2):
    """`DenseQPModel` with badly scaled data: constraint rows and their bounds times factors spanning 1 .. 1e4, P and q times
    1e3.  The minimizer is the un-scaled model's; objective and multipliers carry the factors."""
    nlp = DenseQPModel(n, m, n_eq)
    r = np.logspace(0.0, 4.0, m)
    nlp.A = nlp.A * r[:, None]
    nlp.lcon, nlp.ucon = nlp.lcon * r, nlp.ucon * r
    nlp.P, nlp.q = nlp.P * 1e3, nlp.q * 1e3
    return nlp
