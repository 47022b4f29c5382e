"""Child process of tests/test_gpu_params.py::test_workgroup_reuse_in_a_child_process (started with LMH_ROLLOUT_GROUPS_PER_CU=1, which the
library reads once per process): 300 robots alternate between two parameter sets on one handle, 260 ticks -- every resident workgroup
runs more than one robot and units change hands through the ring -- and every robot must be bit-equal to its counterpart in two shared
handles run on all 300 states.  Prints "reuse ok: ..." and exits 0, or raises."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

from helpers import oracle_system, perturbed_velocities
from params_cases import REUSE_SETS, columns, make_controller

assert os.environ.get("LMH_ROLLOUT_GROUPS_PER_CU") == "1"
B, nt = 300, 260
dt, th = 1e-3, 0.016
o = oracle_system(dt, th)
q0, zcom = o.robot()["q"].copy(), o.zcom
v = perturbed_velocities(B, seed=4242)
which = np.arange(B) % len(REUSE_SETS)


def roll(ctl):
    ctl.set_refs_stance(nt * dt + 1.0, 2)
    st = ctl.new_state(q0, v, t=0.0)
    out, status, log = ctl.rollout(st, nt, log=True)
    ctl.synchronize()
    r = dict(out=out.cpu().numpy()[:, :78], state=st.cpu().numpy(), status=status.cpu().numpy(), log=log.cpu().numpy())
    ctl.close()
    return r


ctl = make_controller(B, dt, th, zcom, warm_start=1)
assert B > torch.cuda.get_device_properties(0).multi_processor_count, "every workgroup must run more than one robot"
ctl.set_params(**columns([REUSE_SETS[w] for w in which], ctl.cfg))
assert ctl.params_per_instance()
mixed = roll(ctl)
assert (mixed["status"][:, 2] & 2 == 0).all(), mixed["status"][mixed["status"][:, 2] & 2 != 0][:8]      # no NaN anywhere: array_equal means bit-equal
shared = [roll(make_controller(B, dt, th, zcom, warm_start=1, **s)) for s in REUSE_SETS]
assert not np.array_equal(shared[0]["state"], shared[1]["state"])
for i in range(B):
    ref = shared[which[i]]
    for name in ("out", "state", "status"):
        assert np.array_equal(mixed[name][i], ref[name][i]), (i, name)
    assert np.array_equal(mixed["log"][:, i], ref["log"][:, i]), (i, "log")
print("reuse ok: %d robots x %d ticks, %d parameter sets, bit-equal to the shared handles" % (B, nt, len(REUSE_SETS)))
