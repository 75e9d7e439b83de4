"""(-m gpu) The hand-written device AC-OPF evaluator (`mnk_opf_*`, csrc/opf_eval.hip) against the mpmath reference of
tests/callback_cases.py, entry by entry and within the float64 bound derived there (sin / cos at 2 ulp): networks with
ngen > narc (the generator tail of the Jacobian and Hessian kernels runs past the arcs) and with more than one ragged
256-thread workgroup, points at d = 0, at random, at the voltage bounds with |d| up to about 3, and with angles of hundreds of
radians.  The largest observed |got - ref| / bound per callback and network goes to profiles/opf_accuracy.json when
MNK_OPF_ACCURACY_OUT names a file."""
import json
import os

import numpy as np
import pytest

from tests import callback_cases as CC
from tests.test_hip_tape import device_eval, gpu_ctx, make_callbacks  # noqa: F401  (gpu_ctx is a fixture)

_measured = {}


@pytest.fixture(scope="module", autouse=True)
def accuracy_record():
    yield
    out = os.environ.get("MNK_OPF_ACCURACY_OUT")
    if out and _measured:
        with open(out, "w") as f:
            json.dump({"bound": "(r + 2 u) 2^-53 sum |t_k| per entry, u = 2 ulp for sin / cos (tests/callback_cases.py)",
                       "ratio": "largest |device - mpmath| / bound over the points and objective weights",
                       "cases": _measured}, f, indent=1, sort_keys=True)


def _check_shape(model, network):
    nbus, ngen, nbr = network
    per_bus = np.bincount(model.gen_bus, minlength=nbus)
    if network == (3, 9, 2):
        assert ngen > model.narc                  # nmax = ngen: the generator tail runs in threads beyond the arcs
    if network == (70, 20, 150):
        assert model.narc == 300 and model.m > 512 and model.narc % 256 and model.m % 256 and len(model.hess_I) % 256
        assert per_bus.max() >= 2 and per_bus.min() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("point", CC.POINTS)
@pytest.mark.parametrize("network", CC.NETWORKS, ids=lambda t: "x".join(map(str, t)))
def test_every_entry_is_within_the_float64_bound_of_the_reference(gpu_ctx, network, point):
    """Reference share: on (2, 1, 1) and (3, 9, 2) every entry.  On (70, 20, 150): all 780 gradient entries, the 591 constraint
    rows, 1681 Jacobian and 690 Hessian entries that are no flow-row entries (angle, thermal, balance, diagonal), and the
    flow rows of 32 arcs (0, 255, 256, 299 and 28 drawn with a fixed seed): 64 rows, 320 Jacobian and 640 Hessian entries.
    The other 268 arcs are covered by the norm-wise comparison with numpy, repeated here."""
    from madnlp_jl_amd.device_callbacks import DeviceOPFCallbacks
    model, x, y, ref = CC.acopf_case(network, point)
    _check_shape(model, network)
    arcs = CC.sampled_arcs(model)
    if arcs is not None:
        narc, nbr = model.narc, model.nbr
        assert len(arcs) == 32 and {0, 255, 256, narc - 1} <= set(arcs)
        assert ref.cons.computed().sum() == model.m - 2 * narc + 64 == 591 + 64
        assert ref.jac.computed().sum() == len(model.jac_I) - 10 * narc + 320 == 1681 + 320
        assert sum(p is not None for p in ref.hess_parts) == len(model.hess_I) - 20 * narc + 640 == 690 + 640
    else:
        assert ref.cons.computed().all() and ref.jac.computed().all() and all(p is not None for p in ref.hess_parts)
    cb, K = make_callbacks(gpu_ctx, model, DeviceOPFCallbacks)
    worst = _measured.setdefault("x".join(map(str, network)), {})
    try:
        for w in CC.WEIGHTS:
            cb.jv.fill_(np.nan)            # device_eval starts g and c as NaN; the callbacks own jv and hv
            cb.hv.fill_(np.nan)
            f, _, g, c, jv, hv = device_eval(gpu_ctx, cb, model, x, y, w)        # (synchronizes torch's stream first)
            for name, got in (("g", g), ("c", c), ("jv", jv), ("hv", hv)):
                assert not np.isnan(got).any(), name
            terms, rg, rc, rj, rh = CC.acopf_reference(model, x, y, w, ref=ref)
            fval, fbound = CC.objective_bound(ref)
            ferr = abs(CC.mpf(float(f)) - fval)
            print(f"{network} {point} w={w}: f ratio {float(ferr / fbound):.3f}")
            assert ferr <= fbound
            worst["eval_f"] = max(worst.get("eval_f", 0.0), float(ferr / fbound))
            for name, got, blk in (("eval_grad", g, rg), ("eval_cons", c, rc), ("eval_jac", jv, rj), ("eval_lag_hess", hv, rh)):
                q = CC.worst(got, blk, CC.U_DEVICE)
                print(f"{network} {point} w={w}: {name} ratio {q:.3f}")
                CC.assert_within(got, blk, CC.U_DEVICE, name)
                worst[name] = max(worst.get(name, 0.0), q)
            # entries without a transcendental factor: bit-identical to numpy (tests/test_acopf.py), and every arc norm-wise
            cr, jr, hr = model.cons(x), model.jac_coord(x), model.hess_coord(x, y, w)
            assert np.array_equal(g, model.grad(x))
            o, oj, oh = 1 + 2 * model.narc, 1 + 10 * model.narc, 20 * model.narc
            assert np.array_equal(c[o:], cr[o:]) and c[0] == cr[0]
            assert np.array_equal(jv[oj:], jr[oj:]) and np.array_equal(hv[oh:], hr[oh:])
            for got, r in ((c, cr), (jv, jr), (hv, hr)):
                assert np.abs(got - r).max() <= 1e-13 * max(1.0, np.abs(r).max())
    finally:
        cb.close()
        K.close()
