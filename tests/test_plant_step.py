"""CPU side of the torque-driven plant (lmh_contact_wrench / lmh_plant_derivative / lmh_plant_step): the record layout and the ABI, the
oracle helper every GPU parity test rests on, and the contact regimes the GPU inputs cover.  No GPU is used."""
import os
import re

import numpy as np

import plant_step_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_contact_record_layout_and_exports(hip_lib):
    """LMH_CONTACT_STRIDE / LMH_CONTACT_OFF_* of the header are capi.CONTACT_STRIDE / CONTACT_FIELDS, the fields tile [0, 40),
    split_contact returns those views, and the three calls are declared, listed in capi.EXPORTS and exported by the built library."""
    from linearmpchumanoid_amd import capi
    from linearmpchumanoid_amd.controller import BatchedController
    src = open(os.path.join(ROOT, "include", "lmh.h")).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+LMH_CONTACT_(\w+)\s+(\d+)", src)}
    assert defs == {"STRIDE": 40, "OFF_W": 0, "OFF_VF": 12, "OFF_PAD": 36}
    assert capi.CONTACT_STRIDE == defs["STRIDE"]
    assert {k: o for k, (o, _) in capi.CONTACT_FIELDS.items()} == {"w": defs["OFF_W"], "vertex_force": defs["OFF_VF"], "pad": defs["OFF_PAD"]}
    cover = np.zeros(capi.CONTACT_STRIDE, dtype=int)
    for o, shape in capi.CONTACT_FIELDS.values():
        cover[o:o + int(np.prod(shape))] += 1
    assert (cover == 1).all()
    rec = np.arange(3 * 40, dtype=np.float64).reshape(3, 40)
    s = BatchedController.split_contact(rec)
    assert s["w"].shape == (3, 12) and s["vertex_force"].shape == (3, 8, 3) and s["pad"].shape == (3, 4)
    assert np.array_equal(s["w"][1], rec[1, 0:12]) and np.array_equal(s["vertex_force"][2, 7], rec[2, 33:36]) and np.array_equal(s["pad"][0], rec[0, 36:40])
    assert np.shares_memory(s["vertex_force"], rec)
    decl = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("lmh_contact_wrench", "lmh_plant_derivative", "lmh_plant_step"):
        assert re.search(r"\bint\s+%s\s*\(" % name, decl) and name in capi.EXPORTS and hasattr(hip_lib, name)
    assert "External forces on the plant\n * are not modelled" not in src


def test_helper_reproduces_the_oracles_plant():
    """oracle_plant_xdot, fed at every stage with the torques Oracle.eval returns there (Robot::v_ still the previous stage's velocity, as
    inside the oracle's own tick), advanced by one RK4 tick, against Oracle.rollout(.., 1) with set_plant(True), on three of the contact
    postures (a foot in the air, a sticking one, a sliding one).  Same arithmetic up to the order of the 30 x 30 solve (numpy's LU against
    the oracle's Gaussian elimination).  Agreement found, max|difference| / max|state|: 4.0e-14, 2.7e-12, 1.3e-12; asserted at ten times
    the largest, 2.7e-11."""
    S = pc.contact_states()
    worst = 0.0
    for i in (0, 3, 5):
        o_own, o_helper = pc.make_oracle(), pc.make_oracle()
        x0 = np.concatenate([S["q"][i], S["v"][i]])
        ref = o_own.rollout(x0, 0.0, 1)["state"]

        def xdot(stage, s):
            ts = (0.0, 0.5 * pc.DT, 0.5 * pc.DT, pc.DT)[stage]
            tau = o_helper.eval(s[:30], s[30:], ts)["tau"]
            return pc.oracle_plant_xdot(o_helper, s[:30], s[30:], np.concatenate([np.zeros(6), tau]), ts)[0]

        got = pc.rk4_tick(x0, pc.DT, xdot)
        err = float(np.abs(got - ref).max() / np.abs(ref).max())
        print("\nhelper tick vs the oracle's plant, state %d: %.2e" % (i, err))
        worst = max(worst, err)
    assert worst <= 2.7e-11, worst


def test_gpu_inputs_cover_every_contact_regime():
    """On BOTH feet the 16 states show a vertex out of the ground, a sticking one (tangential force unclamped, non-zero), a sliding one
    (clamped onto mu f_n) and a penetrating one whose normal force is clamped to 0 -- read off the oracle's own vertex forces."""
    S = pc.contact_states()
    assert S["q"].shape == (16, 30) and np.abs(S["v"][:, 0:3]).max() < 1.0
    for foot in range(2):
        seen = {r for reg in S["regimes"] for r in reg[4 * foot:4 * foot + 4]}
        assert seen == set(pc.REGIMES), (foot, seen)             # and no "?": every penetrating vertex is in a named regime
    o = pc.make_oracle()
    g = pc.GROUND
    for i in range(16):                                           # the friction disc and the clamps, vertex by vertex
        pos, vel = pc.vertex_kinematics(o, S["q"][i], S["v"][i])
        _, vf = o.contact()
        for n, reg in enumerate(S["regimes"][i]):
            ft, raw = np.hypot(vf[n, 0], vf[n, 1]), g["dt"] * np.hypot(vel[n, 0], vel[n, 1])
            if reg == "out":
                assert pos[n, 2] >= 0.0 and not vf[n].any()
            elif reg == "stick":
                assert vf[n, 2] > 0.0 and 0.0 < ft <= g["mu"] * vf[n, 2] and abs(ft - raw) <= 1e-12 * raw
            elif reg == "slide":
                assert vf[n, 2] > 0.0 and raw > g["mu"] * vf[n, 2] and abs(ft - g["mu"] * vf[n, 2]) <= 1e-12 * ft
            else:
                assert pos[n, 2] < 0.0 and not vf[n].any()
