"""Drop-in boundary: the shim library exports the reference's class surface, and this repo's equivalent of the
reference's apps/offline app, built against the shim headers, must reproduce the committed apps/offline CoM-x trace
on the GPU."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shim_library_builds():
    from linearmpchumanoid_amd import build as b
    so, app = b.build_shim()
    assert os.path.exists(so) and os.path.exists(app)
    syms = subprocess.check_output(["nm", "-DC", so]).decode()
    for s in ("Controller::standStep", "Controller::WBC", "Kinematics::compute", "footCoeffTrajectory", "Robot::Robot", "ZMP::ZMP"):
        assert s in syms


@pytest.mark.gpu
def test_offline_app_reproduces_golden_trace():
    from linearmpchumanoid_amd import build as b
    _, app = b.build_shim()
    out = subprocess.check_output([app, "1.0", "0.01", "0.5"], timeout=300).decode().splitlines()
    xs = np.array([float(l) for l in out if l and (l[0] in "-0123456789")])
    g = np.load(os.path.join(ROOT, "tests", "golden", "offline_trace.npz"))
    # T = 1 s -> 100 ticks (ZMP arrays are shorter than for T = 5 but constant: same trace prefix)
    assert len(xs) >= 99
    n = min(len(xs), 100)
    assert np.abs(xs[:n] - g["comx"][:n]).max() < 1e-10
