"""Three stepper configurations that between them switch every optional term on, and one run of each: shared by
tools/make_golden_stepper_terms.py (which records the run of the commit before the table of terms) and
tests/test_gpu_stepper_terms.py (which compares the current tree with it).  Only the stepper's public surface is used, so the
same code drives both trees.

The batch is the 8-row fixture mala_allegro_sphere_b8_n4.npz (two objects, four rows each), the surface samples are those of
energy_allegro_sphere_b4_n4.npz, the scene is the wall of tests/test_gpu_approach.py, the arm is arm7 of tests/_arm_oracle.py.

  A  all ten terms; reach_stations=2, reach_iterations=8, track_waypoints=4, track_updates=2, arm_on_track=True,
     lift_object_samples=64
  B  a grid per object (clutter) with scene, approach, squeeze, reach and arm: the arm reads reach_q, squeeze has no tabletop
     constant, g_theta is written and not added
  C  pre-grasp and lift only, scene=None with pregrasp_scene= and lift_scene= given: the fall-backs, and pre-grasp alone supplies
     g_theta"""
import functools
import os

import numpy as np
import torch

import _arm_oracle as ao
import _scene_oracle as so

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
S_SHAPE, S_ORIGIN, S_H = (100, 100, 100), (-0.5013, -0.4987, -0.5021), 0.01  # the wall of tests/test_gpu_approach.py
STATE = ("hand_pose", "contact_idx", "energy", "grad", "terms", "ema", "step_count", "accept")  # as tests/test_gpu_approach.py
EXTRA = ("reach_q", "track_q", "squeeze_theta", "lift_object")
ARM_BASE = np.array([[1.0, 0.0, 0.0, -0.45], [0.0, 1.0, 0.0, 0.10], [0.0, 0.0, 1.0, -0.25]], dtype=np.float32)
RESET_MASK = (False, True, False, False, False, False, True, False)
CASES = ("A", "B", "C")


@functools.lru_cache(maxsize=None)
def _load(name):
    return np.load(os.path.join(GOLDEN, name), allow_pickle=False)


@functools.lru_cache(maxsize=None)
def _wall(c=0.02):
    from graspqp_amd import ops

    f = so.affine(S_SHAPE, S_ORIGIN, S_H, c=c)
    return ops.SceneSDF(f.values.cuda(), [float(o) for o in f.origin], float(f.voxel))


@functools.lru_cache(maxsize=None)
def _walls():
    """A grid per object of the fixture: the wall and the wall moved by a centimetre."""
    from graspqp_amd import ops

    return ops.SceneSDFSet(torch.stack([_wall(0.02).values, _wall(0.03).values]).contiguous(), _wall().origin, _wall().voxel)


@functools.lru_cache(maxsize=None)
def _arm():
    from graspqp_amd import ops

    return ops.ArmHandle(ao.arm_spec("arm7"))


def config(case):
    """-> the keyword arguments of GraspStepper for ``case`` ("five": no optional term)."""
    reach = dict(arm=_arm(), arm_base=ARM_BASE, reach_distance=0.08)
    if case == "five":
        return {}
    if case == "A":
        return dict(weights={"E_prior": 2.0, "E_wall": 3.0, "E_scene": 50.0, "E_approach": 20.0, "E_pregrasp": 30.0, "E_squeeze": 1000.0,
                             "E_reach": 1e4, "E_arm": 100.0, "E_track": 1e4, "E_lift": 40.0},
                    scene=_wall(), scene_margin=0.01, approach_distance=0.10, approach_stations=4, pregrasp_distance=0.08,
                    pregrasp_stations=2, reach_stations=2, reach_iterations=8, track_waypoints=4, track_updates=2, arm_on_track=True,
                    lift_object_samples=64, **reach)
    if case == "B":
        return dict(weights={"E_scene": 50.0, "E_approach": 20.0, "E_squeeze": 1000.0, "E_reach": 1e4, "E_arm": 100.0},
                    scene=_walls(), scene_margin=0.01, approach_distance=0.10, approach_stations=4, reach_stations=1, reach_iterations=8,
                    **reach)
    if case == "C":
        return dict(weights={"E_pregrasp": 30.0, "E_lift": 40.0}, scene=None, pregrasp_scene=_wall(0.02), lift_scene=_wall(0.03),
                    scene_margin=0.005, pregrasp_margin=0.01, lift_object_samples=64)
    return single(case)


def single(name):
    """One optional term alone (with what it cannot be without: E_arm and E_track need E_reach)."""
    kw = dict(weights={name: 10.0}, scene=_wall(), scene_margin=0.01)
    if name in ("E_reach", "E_arm", "E_track"):
        kw.update(arm=_arm(), arm_base=ARM_BASE, reach_distance=0.08, reach_stations=1, reach_iterations=4, track_waypoints=2,
                  track_updates=1)
        kw["weights"]["E_reach"] = 1e4
    return kw


def stepper(case):
    from graspqp_amd import ops
    from graspqp_amd.stepper import GraspStepper

    g, ge = _load("mala_allegro_sphere_b8_n4.npz"), _load("energy_allegro_sphere_b4_n4.npz")
    n_obj, be = int(g["n_obj"]), int(g["batch_size_each"])
    fvs = [g[f"obj{i}_face_verts"] for i in range(n_obj)]
    sps = np.stack([g[f"obj{i}_surface_points"] for i in range(n_obj)])
    hand = _hand()
    return GraspStepper(hand, ops.MeshSet(fvs), torch.tensor(sps), be, 4, surface_samples=(ge["opt_surface_points"], ge["opt_surface_link"]),
                        **config(case))


@functools.lru_cache(maxsize=None)
def _hand():
    from graspqp_amd import ops
    from graspqp_amd.hands import get_hand_spec

    return ops.HandHandle(get_hand_spec("allegro"))


def start():
    g = _load("mala_allegro_sphere_b8_n4.npz")
    return torch.tensor(g["hand_pose0"], dtype=torch.float32).cuda(), torch.tensor(g["contact_idx0"]).cuda()


def draws(s):
    g = _load("mala_allegro_sphere_b8_n4.npz")
    f32 = lambda k: torch.tensor(g[k], dtype=torch.float32).cuda()
    return f32(f"s{s}_u_switch"), torch.tensor(g[f"s{s}_new_idx"]).cuda(), f32(f"s{s}_u_accept")


def _snapshot(st, tag, out):
    torch.cuda.synchronize()
    for k in STATE:
        out[f"{tag}.{k}"] = getattr(st, k).cpu().numpy()
    for k in EXTRA:
        if getattr(st, k) is not None:
            out[f"{tag}.{k}"] = getattr(st, k).cpu().numpy()


def three_steps(st, captured=False):
    """reset + the three golden steps with the fixture's draws -> the state; ``captured``: the steps replay a captured graph."""
    hp, idx = start()
    st.reset(hp, idx)
    if captured:
        st.capture()
    for s in (1, 2, 3):
        st.step(draws=draws(s))
    out = {}
    _snapshot(st, "steps", out)
    return out


def run(case):
    """One fresh stepper of ``case``: evaluate at the fixture's start, reset + three steps, one step_reset with a fixed mask.
    -> {name: numpy array}."""
    st = stepper(case)
    hp, idx = start()
    terms, total, grad = st.evaluate(hp, idx)
    torch.cuda.synchronize()
    out = {f"evaluate.{k}": v.cpu().numpy() for k, v in terms.items()}
    out["evaluate.total"], out["evaluate.grad"] = total.cpu().numpy(), grad.cpu().numpy()
    out.update(three_steps(st))
    st.step_reset(torch.tensor(RESET_MASK), hp.roll(3, 0), idx.roll(3, 0), draws=draws(4))
    _snapshot(st, "reset", out)
    return out
