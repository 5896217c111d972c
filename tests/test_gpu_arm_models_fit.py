"""The fit on the arm models other than the stock one (tests/arm_model_cases.py: `tilted`, stock arms on a rotated base, and `calibrated`, DH
offsets that differ per arm).  The rule knows rows, stamps and limits, not the model: under each model's context the 17-row path of
fit_cases.ragged_batch (six dilations) and its three-row path give the restatement's bits through the device and the host mirror forms, and
the audit of the fitted stamps under that model — whose constraint gap and isSatisfied run through the GENERAL instantiations of the
function kernels — reports the fit's speed and acceleration peaks bit for bit."""
import numpy as np
import pytest

import arm_model_cases as A
import fit_cases as fc
import setpoint_cases as sc
from fit_cases import NAMES, PANDA_AMAX, PANDA_VMAX, same_fit
from test_gpu_parity import _constraint

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a, order="C", copy=True)).cuda()


@pytest.mark.parametrize("model", ["tilted", "calibrated"])
def test_fit_and_the_audit_of_its_stamps(gpu_ctx, model):
    ref = fc.reference()
    case, want_all = ref["case"], ref["want"]
    pf = case["path_first"]
    pick = [NAMES.index("three"), NAMES.index("seventeen")]
    rows, first, time = sc.pack([(case["rows"][pf[f]:pf[f + 1]], case["time"][pf[f]:pf[f + 1]]) for f in pick])
    want = fc.fit_py(rows, first, time, PANDA_VMAX, PANDA_AMAX, **fc.options(case))
    assert want["status"].tolist() == [fc.FITTED] * 2 and want["passes"].tolist() == [int(want_all["passes"][f]) for f in pick]
    c = _constraint(A.OBJ, gpu_ctx, mode=1)
    with A.apply(c, gpu_ctx, model):
        dev = c.fit_timestamps(_dev(rows), _dev(first), _dev(time), PANDA_VMAX, PANDA_AMAX, **fc.options(case))
        same_fit(dev, want, (model, "device"))
        same_fit(c.fit_timestamps(rows, first, time, PANDA_VMAX, PANDA_AMAX, **fc.options(case)), want, (model, "host"))
        sp = c.setpoint_paths(_dev(rows), _dev(first), dev["time"], PANDA_VMAX, PANDA_AMAX, period=case["period"], max_ticks=case["max_ticks"])
        peak = sp["peak"].cpu().numpy()
        assert sc.same_f64(peak[:, :2], want["peak"]) and (sp["stretch"].cpu().numpy() == 1.0).all()
        print("%s: %s dilations, audit of the fitted stamps: %d of %d ticks refused" % (model, want["passes"].tolist(), int(sp["counts"].cpu().numpy()[:, 0].sum()), sp["ticks"]))
