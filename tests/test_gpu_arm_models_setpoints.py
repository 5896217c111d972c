"""Setpoints and the execution audit on the arm models other than the stock one (tests/arm_model_cases.py: `tilted`, stock arms on a rotated
base, and `calibrated`, DH offsets that differ per arm): the interpolation does not know the model, but the constraint gap and isSatisfied of
every tick run through the GENERAL instantiations of the function kernels there.  The 17-row path of the ragged batch (257 ticks) under
each model's problem: q, qd, tau and the speed and acceleration audit equal the plain-Python restatement, f, satisfied and their peaks the det
oracle's `function` and `is_satisfied` under that model, bit for bit, through the device and the host mirror forms.  The rows lie on the
STOCK manifold, so under these models the gap is large and most ticks are refused — which is what makes the comparison tell."""
import numpy as np
import pytest

import arm_model_cases as A
import setpoint_cases as sc
from setpoint_cases import PANDA_AMAX, PANDA_VMAX, same_setpoints
from test_gpu_parity import _constraint, _oracle_problem

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a, order="C", copy=True)).cuda()


@pytest.mark.parametrize("model", ["tilted", "calibrated"])
def test_setpoints_and_audit(gpu_ctx, oracle_det, model):
    case = sc.reference()["ragged"]["case"]
    pf = case["path_first"]
    rows, time, first = case["rows"][pf[4]:pf[5]], case["time"][pf[4]:pf[5]], np.array([0, 17], dtype=np.int32)
    c = _constraint(A.OBJ, gpu_ctx, mode=1)
    with A.apply(c, gpu_ctx, model):
        P = _oracle_problem(oracle_det, c)
        want = sc.setpoints_py(rows, first, time, PANDA_VMAX, PANDA_AMAX, case["period"], O=oracle_det, P=P)
        stock = sc.reference()["ragged"]["want"]
        assert want["ticks"] == 257 and not sc.same_f64(want["f"], stock["f"][stock["tick_first"][4]:stock["tick_first"][5]])  # the model changes the gap
        print("%s: max |dp| %.4f at tick %d, max angle %.4f at tick %d, %d of 257 ticks refused" % (
            model, want["peak"][0, sc.DP], want["peak_tick"][0, sc.DP], want["peak"][0, sc.ANGLE], want["peak_tick"][0, sc.ANGLE], want["counts"][0, 0]))
        same_setpoints(c.setpoint_paths(_dev(rows), _dev(first), _dev(time), PANDA_VMAX, PANDA_AMAX, period=case["period"]), want, (model, "device"))
        same_setpoints(c.setpoint_paths(rows, first, time, PANDA_VMAX, PANDA_AMAX, period=case["period"]), want, (model, "host"))
