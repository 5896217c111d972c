"""Resample and time stamps on the arm models other than the stock one (tests/arm_model_cases.py: `tilted`, stock arms on a rotated base,
and `calibrated`, DH offsets that differ per arm): the blends go through the projector, which chooses its kernel by the model, and the
dense paths come from the extend step, which does too.  The four synthetic paths of the model's own manifold (2, 3, 6 and 1 waypoints,
the seeds of the densify test) are densified, resampled by spacing and by count, and time-stamped; everything equals the plain-Python
restatement of tests/retime_cases.py on the det oracle, bit for bit, through the device and the host mirror forms."""
import numpy as np
import pytest

import arm_model_cases as A
import retime_cases as rc
from retime_cases import PANDA_AMAX, PANDA_VMAX, same_sampled, same_stamps
from test_gpu_parity import _constraint, _oracle_problem

pytestmark = pytest.mark.gpu
SPACING, COUNT = 0.125, 9


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a, order="C", copy=True)).cuda()


@pytest.mark.parametrize("model", ["tilted", "calibrated"])
@pytest.mark.parametrize("mode", [0, 1])
def test_resample_and_timestamps(gpu_ctx, oracle_det, mode, model):
    c = _constraint(A.OBJ, gpu_ctx, mode=mode)
    with A.apply(c, gpu_ctx, model):
        P = _oracle_problem(oracle_det, c)
        pj, pl = A.waypoint_paths(c, oracle_det, P, A.F_PATHS, A.L_PATHS, A.PATH_SEED[(model, mode)])
        R = rc.Restatement(oracle_det, P)
        dense_want = R.dense(pj, pl)
        wants = [(dict(spacing=SPACING), R.resample(dense_want, spacing=SPACING)), (dict(count=COUNT), R.resample(dense_want, count=COUNT))]
        ok_paths = int((wants[0][1]["status"] == rc.OK).sum())
        print("%s mode %d: status %s, counts %s" % (model, mode, wants[0][1]["status"].tolist(), wants[0][1]["counts"].sum(axis=0).tolist()))
        assert wants[0][1]["status"][3] == rc.POINT and ok_paths >= 2 and rc.interior_projected_share(wants[0][1]) >= 0.9
        assert wants[0][1]["counts"][:, rc.PROJECTED].sum() >= 16
        for device in (True, False):
            dense = c.densify_paths(_dev(pj) if device else pj, _dev(pl) if device else pl, keep_handle=True)
            try:
                for kw, want in wants:
                    got = c.resample_paths(dense, **kw)
                    same_sampled(got, want, (model, mode, device, kw))
                    stamps = c.timestamp_paths(got["joints"], got["path_first"], PANDA_VMAX, PANDA_AMAX, profile=True)
                    same_stamps(stamps, rc.timestamps_py(want["joints"], want["path_first"], PANDA_VMAX, PANDA_AMAX, fill=0.0), (model, mode, device, kw))
            finally:
                dense["handle"].close()
