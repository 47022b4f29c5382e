"""CPU side of the per-robot ground planes (lmh_set_ground): the record layout and the ABI, the numpy statement of the contact model
(trajectories.ground_contact) against the oracle's flat contact and against its own symmetries, the record builder, and the regimes the
GPU inputs of ground_cases.tilted_states() cover.  No GPU is used."""
import os
import re

import numpy as np

import ground_cases as gc
import plant_step_cases as pc
from linearmpchumanoid_amd import capi, trajectories

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = pc.GROUND


def _contact(pos, vel, planes):
    return trajectories.ground_contact(pos, vel, planes, G["k"], G["d"], G["dt"], G["mu"])


def test_ground_record_layout_and_exports(hip_lib):
    """LMH_GROUND_STRIDE / LMH_GROUND_OFF_* of the header are capi's constants, and the three calls are declared, listed in capi.EXPORTS and
    exported by the built library."""
    src = open(os.path.join(ROOT, "include", "lmh.h")).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+LMH_GROUND_(\w+)\s+(\d+)", src)}
    assert defs == {"STRIDE": 8, "OFF_N_R": 0, "OFF_H_R": 3, "OFF_N_L": 4, "OFF_H_L": 7}
    assert (capi.GROUND_STRIDE, capi.GROUND_OFF_N_R, capi.GROUND_OFF_H_R, capi.GROUND_OFF_N_L, capi.GROUND_OFF_H_L) == (8, 0, 3, 4, 7)
    decl = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("lmh_set_ground", "lmh_ground_per_instance", "lmh_get_ground"):
        assert re.search(r"\bint\s+%s\s*\(" % name, decl) and name in capi.EXPORTS and hasattr(hip_lib, name)


def test_tilted_states_cover_every_regime_with_margin():
    """Every aimed vertex is in its regime, every regime occurs on each foot, no vertex is closer than 10 um to its plane, and every
    penetrating vertex is at least 10 % (relative) away from the fn = 0 threshold and from the friction disc: round-off cannot move a
    vertex across a threshold between the statement and the kernels."""
    S = gc.tilted_states()
    seen = [dict.fromkeys(pc.REGIMES, 0), dict.fromkeys(pc.REGIMES, 0)]
    min_pen, min_fn, min_disc = np.inf, np.inf, np.inf
    for i, (foot, j, want) in enumerate(S["aimed"]):
        assert foot == i % 2 and want == pc.REGIMES[(i // 2) % 4] and j // 4 == foot
        assert S["regimes"][i][j] == want, (i, j, want, S["regimes"][i])
        for n, r in enumerate(S["regimes"][i]):
            seen[n // 4][r] += 1
        pen, m_fn, m_disc = gc.thresholds(S["pos"][i], S["vel"][i], S["planes"][i])
        min_pen, min_fn, min_disc = min(min_pen, np.abs(pen).min()), min(min_fn, m_fn.min()), min(min_disc, m_disc.min())
    print("\nregimes right %s left %s; min |pen| %.3g m, margins fn %.3f disc %.3f" % (seen[0], seen[1], min_pen, min_fn, min_disc))
    for foot in range(2):
        assert all(seen[foot][r] > 0 for r in pc.REGIMES), seen
    assert min_pen >= 10.0e-6, min_pen
    assert min_fn >= 0.1 and min_disc >= 0.1, (min_fn, min_disc)
    normals = S["planes"].reshape(16, 2, 4)[:, :, :3]
    tilt = np.rad2deg(np.arccos(normals[:, :, 2]))
    assert (np.abs((normals ** 2).sum(-1) - 1.0) <= 1e-12).all() and (tilt >= 2.0 - 1e-9).all() and (tilt <= 6.0 + 1e-9).all()


def test_statement_is_the_oracles_contact_on_flat_ground():
    """ground_contact with the flat record against Oracle.contact() on the 16 flat states: forces within 1e-12 x the force scale (k x 2 mm =
    40 N), the same zero pattern, the regimes of contact_states().  The two differ in the rounding of the tangential norm alone."""
    S = pc.contact_states()
    o = pc.make_oracle()
    worst = 0.0
    for i in range(pc.B):
        pos, vel = pc.vertex_kinematics(o, S["q"][i], S["v"][i])
        _, vf = o.contact()
        f, regimes = _contact(pos, vel, gc.FLAT)
        worst = max(worst, float(np.abs(f - vf).max()))
        assert np.array_equal(f == 0.0, vf == 0.0), i
        assert list(regimes) == list(S["regimes"][i]), (i, regimes, S["regimes"][i])
    print("\nstatement vs Oracle.contact on flat ground: %.2e N (scale %.0f N)" % (worst, gc.FORCE_SCALE))
    assert worst <= 1e-12 * gc.FORCE_SCALE, worst


def test_statement_step_height_identity():
    """Horizontal planes at h_R, h_L give, foot by foot, exactly the forces of flat ground under vertices lowered by the foot's h."""
    S = gc.tilted_states()
    for i in range(pc.B):
        pos, vel = S["pos"][i], S["vel"][i]
        hr, hl = 3.0e-3, -2.0e-3
        f, rg = _contact(pos, vel, trajectories.ground_planes(0.0, 0.0, hr, hl))
        low = pos.copy()
        low[:4, 2] -= hr; low[4:, 2] -= hl
        f0, rg0 = _contact(low, vel, gc.FLAT)
        assert np.allclose(f, f0, rtol=0.0, atol=1e-13 * gc.FORCE_SCALE) and rg == rg0 and np.array_equal(f == 0.0, f0 == 0.0)


def test_statement_rotation_covariance():
    """Planes and vertex data rotated together give the rotated forces, to 1e-13 of the force scale, in the same regimes."""
    S = gc.tilted_states()
    rng = np.random.default_rng(20261021)
    worst = 0.0
    for i in range(pc.B):
        axis = rng.normal(size=3); axis /= np.linalg.norm(axis)
        ang = rng.uniform(0.2, 1.2)
        K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        R = np.eye(3) + np.sin(ang) * K + (1.0 - np.cos(ang)) * K @ K
        rec = S["planes"][i].copy()
        rec[0:3], rec[4:7] = R @ rec[0:3], R @ rec[4:7]
        f, rg = _contact(S["pos"][i] @ R.T, S["vel"][i] @ R.T, rec)
        worst = max(worst, float(np.abs(f - S["force"][i] @ R.T).max()))
        assert rg == S["regimes"][i]
    print("\nrotation covariance: %.2e N" % worst)
    assert worst <= 1e-13 * gc.FORCE_SCALE, worst


def test_ground_planes_round_trip():
    """ground_planes -> unit normals pointing up, the same under both feet, offsets in their words; ground_slope gives the arguments back;
    slope 0 is the flat record; a slope of pi / 2 is refused."""
    rng = np.random.default_rng(20261022)
    slope, az = np.deg2rad(rng.uniform(0.5, 10.0, 32)), rng.uniform(-np.pi, np.pi, 32)
    hr, hl = rng.uniform(-0.01, 0.01, 32), rng.uniform(-0.01, 0.01, 32)
    rec = trajectories.ground_planes(slope, az, hr, hl)
    assert rec.shape == (32, 8) and np.array_equal(rec[:, 0:3], rec[:, 4:7]) and (rec[:, 2] > 0.0).all()
    assert (np.abs((rec[:, 0:3] ** 2).sum(-1) - 1.0) <= 1e-12).all()
    s2, a2, hr2, hl2 = trajectories.ground_slope(rec)
    assert np.allclose(s2, slope, rtol=0, atol=1e-14) and np.allclose(a2, az, rtol=0, atol=1e-13) and np.array_equal(hr2, hr) and np.array_equal(hl2, hl)
    # the ground rises towards the azimuth: a point uphill at the plane's height lies on the plane
    up = np.stack([np.cos(az), np.sin(az), np.tan(slope)], axis=-1)
    assert np.allclose((rec[:, 0:3] * up).sum(-1), 0.0, atol=1e-15)
    assert np.array_equal(trajectories.ground_planes(0.0, 0.0), gc.FLAT)
    assert trajectories.ground_planes(np.zeros(5), 0.3, 0.001, np.arange(5.0)).shape == (5, 8)
    try:
        trajectories.ground_planes(0.5 * np.pi, 0.0)
    except ValueError:
        pass
    else:
        raise AssertionError("a vertical ground must be refused")
