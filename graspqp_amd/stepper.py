"""GraspStepper -- one MALA* iteration (reference scripts/fit.py:399-458) as a fixed sequence of HIP launches.

No autograd, no host synchronisation, no allocation inside ``step``: all buffers are created once, so the
whole iteration is capturable into a hipGraph (``capture()``).  It runs exactly the kernels that the autograd
route (``graspqp_amd.core``) runs, in the reference's order:

    propose (+z-score) -> FK+contacts -> { object SDF -> contact terms -> E_fc fwd -> E_fc bwd | hand penetration
    fwd -> bwd (+E_pen) | self penetration } -> FK bwd (+E_dis, E_joints, total) -> accept

State (device tensors): hand_pose (B,D), contact_idx (B,n) i64, grad (B,D), energy (B), ema (B,D), step (B) i64,
terms (5,B) = accepted [E_dis, E_fc, E_pen, E_spen, E_joints].

Tabletop mode (a weight on "E_prior" or "E_wall", scripts/fit.py:77-78,369-373; core/energy.py:68-78): the two terms are one
more launch (gq_tabletop_terms) between the joined branches and the FK backward, which adds their link wrenches and
global-pose gradients to the penetration branch's; ``terms`` is then (7,B) with [E_prior, E_wall] appended, and the
proposal and the accept step are the stand-alone launches.

Scene mode (a weight on "E_scene" and an ``ops.SceneSDF``): the hand's surface samples must stay outside a signed-distance grid
of the surroundings.  One more launch (gq_scene_terms) after the joined branches -- after gq_tabletop_terms when both modes are
on -- adds its link wrenches and gRt the same way; ``terms`` gets [E_scene] appended last, and the proposal and the accept step
are the stand-alone launches.  The grid's values may be overwritten in place between iterations (moving obstacles), also
between replays of a captured graph.

Approach mode (a weight on "E_approach" and an ``ops.SceneSDF``, with or without a weight on "E_scene"): the corridor the hand
travels along its approach axis must be free of the same grid.  One more launch (gq_approach_terms) after gq_scene_terms adds
its link wrenches and gRt the same way; ``terms`` gets [E_approach] appended last, after E_scene; its share of the row total is
one more gq_scene_total launch, and the proposal and the accept step are the stand-alone launches.

Pre-grasp mode (a weight on "E_pregrasp" and a grid, ``pregrasp_scene`` or else ``scene``): the hand travels the corridor OPEN, so the
hand with its joints opened by ``pregrasp_opening`` must be free of the grid at every station d_k = D k / K, k = 0..K, the grasp
pose included -- which is why this term's grid may contain the target and E_scene's must not.  One more launch (gq_pregrasp_terms:
opened kinematics, stations and joint gradient of the row) after gq_approach_terms adds its gRt to the shared buffer and overwrites
``g_theta``, the direct joint gradient the FK backward takes in this mode only; ``terms`` gets [E_pregrasp] appended last, its share
of the row total is one more gq_scene_total launch, and the proposal and the accept step are the stand-alone launches.

Squeeze mode (a weight on "E_squeeze"): can the fingers close onto the object from this pose?  Every contact moves along the outward
object normal by max(|distance|, ``squeeze_min_travel``); the damped pseudo-inverse of the stacked contact Jacobian gives the joint
velocities that produce this motion best (``squeeze_theta``), and the term charges the mean squared part of the motion the joints
cannot produce.  At the defaults (5 mm, damping 1e-3) it is the reference's E_manipulativity (core/energy.py:80-87) in value and
gradient -- that name stays refused as a stepper weight; the class surface (``calculate_energy``) keeps it for the composed route.
One more launch (gq_squeeze_terms: Jacobian, fp64 normal equations, both solves, residual and the three gradient parts of the row)
after the joined branches and the obstacle terms adds to ``g_cpts``, which the contact branch has written by then, writes ``g_theta``
(adds to it when E_pregrasp is on too) and writes the per-iteration ``g_R`` buffer the FK backward reads (E_prior's constant plus this
term's part; the constant itself is never modified); ``terms`` gets [E_squeeze] appended last, its share of the row total is one more
gq_scene_total launch, and the proposal and the accept step are the stand-alone launches.

Reach mode (a weight on "E_reach", with ``arm`` and ``arm_base``): can the arm the hand sits on bring it to this pose, and to the
stations of its retreat?  Station k = 0..``reach_stations`` is the root pose moved back by ``reach_distance`` k / ``reach_stations``
along the grasp axis (station 0: the grasp pose); per station and per seed of the arm ``reach_iterations`` damped-least-squares
updates of the arm's joints (``reach_damping``, rotation weighed by ``reach_rot_scale`` metres per radian, steps capped at 0.5 and
clamped to the limits) are followed by one more FK, and the term is the mean over the stations of the smallest squared pose error over
the seeds, in m^2.  ``arm_base`` places the arm base in the frame of each object.  One more launch (gq_reach_terms: eight lanes per
IK problem, the stations and seeds of a row side by side in one block) after gq_squeeze_terms and before gq_fk_backward ADDS its
gradient to ``gRt``; ``g_R`` and ``g_theta`` are not touched.  The gradient is the partial derivative with respect to the target with
the final joints held fixed: the gradient of the converged energy where the iteration has converged, an approximation elsewhere
(the Metropolis test sees the value, which is a pure function of the pose: no joint state is carried between evaluations).
``reach_q`` (B,K+1,N) and ``reach_seed`` (B,K+1) hold the winning arm configuration and its seed of the last evaluation; ``terms`` gets
[E_reach] appended last, its share of the row total is one more gq_scene_total launch, and the proposal and the accept step are the
stand-alone launches.

Arm mode (a weight on "E_arm", in reach mode, with an arm that has collision spheres and ``arm_scene`` or ``scene``): where does the arm
configuration of the reach term put the arm?  E_arm is the mean over the reach term's stations of sum_s max(``arm_margin`` + r_s -
phi(x_s), 0) over the arm's collision spheres at ``reach_q``, in metres, on the grid of ``arm_scene`` (one grid, or one per object; it
may contain the target).  One more launch right after the reach launch (gq_arm_terms: a block per row, a wavefront per station,
lane = sphere) ADDS its gradient to ``gRt``: the minimum-norm tracking of the target at the term's own damping ``arm_damping``
(include/graspqp_hip.h, "arm clearance": exact along that tracking for a reached target with no joint on a limit, an approximation
elsewhere).  ``terms`` gets [E_arm] appended after [E_reach]; ``select`` gates it at 0 by default; with weight 0 nothing changes.

Track mode (a weight on "E_track", in reach mode with ``reach_stations`` >= 1): can the arm FOLLOW the straight approach line?  The reach
term's stations are independent IK problems, so ``reach_q`` is not a path; this term tracks ``track_waypoints`` + 1 waypoints from the
retreated pose to the grasp pose, starting at ``reach_q[:, K]`` and warm-starting every waypoint from the one before with
``track_updates`` updates of the reach term's update (its distance, damping, rotation scale and axis).  E_track is the mean of |e_i|^2
over the waypoints, in m^2.  One more launch right after the reach launch (gq_track_terms: eight lanes per row, eight rows per
wavefront) ADDS its gradient to ``gRt`` (the partial derivative with respect to the targets with the path held fixed: include/
graspqp_hip.h, "approach tracking").  ``track_q`` (B,T+1,N), ``track_step`` (B) and ``track_worst`` (B) hold the path, its largest
joint move between waypoints and its worst waypoint; ``terms`` gets [E_track] appended last; ``select`` does not gate it by default.
``arm_on_track`` = True makes E_arm read the path's configurations at the stations (``track_station_q``) in place of ``reach_q``: the
launch order is then reach, track, arm.  With weight 0 and the switch off nothing changes.

Lift mode (a weight on "E_lift" and a grid, ``lift_scene`` or else ``scene``; the grid must not contain the target): every obstacle term
above follows the hand on its way in; this one asks whether hand and object get out.  Station k = 1..``lift_stations`` is the rigid body
"hand + held object" carried by (k / K) (``lift_height`` u - ``lift_retreat`` R a), u = ``lift_direction`` in the object's frame, a the
grasp axis; E_lift is the mean over the stations of the hinge sums of the hand's surface samples (margin ``lift_margin``) and of the
object's points (``lift_object_points``, or an even stride of ``surf``; margin ``lift_object_margin``, which may be negative).  One more
launch (gq_lift_terms) with the other hand-surface launches before gq_fk_backward adds its link wrenches and gRt; ``lift_object`` (B)
holds the object's share of the last evaluation; ``terms`` gets [E_lift] appended last, its share of the row total is one more
gq_scene_total launch, ``select`` gates it at 0 by default, and the proposal and the accept step are the stand-alone launches.  With
weight 0 nothing changes.

Clutter (``scene`` is an ``ops.SceneSDFSet`` with one grid per object): the same two launches read a stack of grids and pick the
grid from the row, row // batch_each (gq_clutter_terms / gq_clutter_corridor_terms, the same row bodies: bit for bit the single-grid
launch's numbers on that grid).  ``ops.scene_compose`` refills the stack in place, also between replays of a captured graph.

Objects as oriented point clouds (an ``ops.PointCloudSet`` in the place of the ``ops.MeshSet``): the object SDF of the contacts is
gq_cloud_forward, always a launch of its own; it fills the same four buffers, so every other launch is the one of a mesh object.
"""

from __future__ import annotations

import collections
import ctypes
import types

import torch

from . import _C, ops

TERM_NAMES = ("E_dis", "E_fc", "E_pen", "E_spen", "E_joints")
TABLETOP_TERMS = ("E_prior", "E_wall")
SCENE_TERMS = ("E_scene",)
APPROACH_TERMS = ("E_approach",)
PREGRASP_TERMS = ("E_pregrasp",)
SQUEEZE_TERMS = ("E_squeeze",)
REACH_TERMS = ("E_reach",)
ARM_TERMS = ("E_arm",)
TRACK_TERMS = ("E_track",)
LIFT_TERMS = ("E_lift",)
DEFAULT_WEIGHTS = {"E_dis": 100.0, "E_fc": 1.0, "E_pen": 100.0, "E_spen": 10.0, "E_joints": 1.0}  # fit.py:51-55


OBSTACLE_TERMS = SCENE_TERMS + APPROACH_TERMS + PREGRASP_TERMS

# The optional terms, one row each, in DECLARATION order: the order of their rows in ``term_names`` / ``terms`` and of their shares in
# the fp32 total ("how a term enters the stepper").  A term is on when one of its weights is > 0.
#   key      the term's pieces in GraspStepper: _check_<key>, _bind_<key>, _launch_<key>
#   names    its rows of ``terms``
#   flag     the public attribute that says whether it is on
#   gated    ``select`` gates it at 0.0 by default
#   samples  it reads the hand's surface samples
#   g_theta  its launch writes ``g_theta``, which the FK backward must then be handed
#   total    the entry that adds its share to the total: gq_scene_total once per name, gq_tabletop_total once for both names
#   off      the public attributes that are None while the term is off
Term = collections.namedtuple("Term", "key names flag gated samples g_theta total off")
TERMS = (
    Term("tabletop", TABLETOP_TERMS, "tabletop", False, True, False, "gq_tabletop_total", ()),
    Term("scene", SCENE_TERMS, "scene_mode", True, True, False, "gq_scene_total", ()),
    Term("approach", APPROACH_TERMS, "approach_mode", True, True, False, "gq_scene_total", ()),
    Term("pregrasp", PREGRASP_TERMS, "pregrasp_mode", True, True, True, "gq_scene_total", ()),
    Term("squeeze", SQUEEZE_TERMS, "squeeze_mode", False, False, True, "gq_scene_total", ("squeeze_theta",)),
    Term("reach", REACH_TERMS, "reach_mode", False, False, False, "gq_scene_total", ("arm", "arm_base", "reach_q", "reach_seed")),
    Term("arm", ARM_TERMS, "arm_mode", True, False, False, "gq_scene_total", ("arm_scene",)),
    Term("track", TRACK_TERMS, "track_mode", False, False, False, "gq_scene_total",
         ("track_q", "track_step", "track_worst", "track_station_q")),
    Term("lift", LIFT_TERMS, "lift_mode", True, True, False, "gq_scene_total", ("lift_scene", "lift_object", "lift_object_points")),
)
# LAUNCH order, between the joined branches and gq_fk_backward: the hand-surface launches (they add to the link wrenches), then
# squeeze (it adds to the g_theta of pre-grasp), then reach, then track before arm (track starts at reach_q, arm may read the path)
LAUNCH_ORDER = ("tabletop", "scene", "approach", "pregrasp", "lift", "squeeze", "reach", "track", "arm")
assert sorted(LAUNCH_ORDER) == sorted(t.key for t in TERMS)
# the order in which merge_weights lists the switched weights (it shows in its error message): the youngest term first, the
# obstacle terms at the end
_SWITCHED = tuple(k for t in reversed(TERMS) if t.names[0] not in OBSTACLE_TERMS for k in t.names) + OBSTACLE_TERMS


def term_plan(weights):
    """What a dict of weights (missing keys: 0) makes of the table, on the host alone: ``term_names`` (TERM_NAMES + the names of the
    terms that are on, declaration order), ``launch`` (their keys in launch order), ``fuse_loop`` (no optional term is on: proposal
    and accept step ride in the FK launches), ``needs_samples`` and ``g_theta`` (some term that is on has the column set)."""
    on = [t for t in TERMS if any(weights.get(k, 0.0) > 0 for k in t.names)]
    keys = {t.key for t in on}
    return types.SimpleNamespace(term_names=TERM_NAMES + tuple(k for t in on for k in t.names),
                                 launch=tuple(k for k in LAUNCH_ORDER if k in keys), fuse_loop=not on,
                                 needs_samples=any(t.samples for t in on), g_theta=any(t.g_theta for t in on))


def select_tolerances(term_names, gates=None):
    """The gates of ``GraspStepper.select`` as one tolerance per term of ``term_names`` (+inf: not gated).  ``gates`` = {term name:
    tol}; None gates every obstacle term that is switched on (E_scene, E_approach, E_pregrasp, E_arm for the arm, E_lift for the
    way out) at 0.0 and nothing else -- the "collision-free" of ``init_avoid_scene``.  A name that is no term of the stepper, or
    that names a switched-off term, raises, and so does a NaN tolerance."""
    if gates is None:
        gates = {k: 0.0 for t in TERMS if t.gated for k in t.names if k in term_names}
    tol = [float("inf")] * len(term_names)
    for k, v in gates.items():
        if k not in term_names:
            raise ValueError(f"GraspStepper.select: unknown or switched-off energy term {k!r} in gates (on: {', '.join(term_names)})")
        if float(v) != float(v):
            raise ValueError(f"GraspStepper.select: gates[{k!r}] is NaN")
        tol[term_names.index(k)] = float(v)
    return tol


def merge_weights(weights=None):
    """DEFAULT_WEIGHTS (+ zero weights of the tabletop terms, of the scene term, of the approach term, of the pre-grasp term, of
    the squeeze term, of the reach term, of the arm clearance term, of the tracking term and of the lift term) updated with
    ``weights``; a key that names no term of the stepper raises (it would otherwise be accepted and never used), and so does a
    negative weight of one of the terms that are switched by their weight."""
    w = dict(DEFAULT_WEIGHTS)
    w.update({k: 0.0 for k in _SWITCHED})
    for k, v in (weights or {}).items():
        if k not in w:
            raise ValueError(f"GraspStepper: unknown energy term {k!r} in weights (known: {', '.join(w)})")
        w[k] = float(v)
        if k in _SWITCHED and not w[k] >= 0.0:  # these terms are switched by their weight: > 0 on, 0 off
            raise ValueError(f"GraspStepper: weights[{k!r}] = {v!r} must be >= 0")
    return w


def _check_corridor(name, margin, distance, stations, first):
    """The corridor of the approach term (``name`` = "approach", stations ``first`` = 1..32) or of the pre-grasp term ("pregrasp",
    0..32: d = 0 is a station there)."""
    if not float(margin) >= 0.0:
        raise ValueError(f"GraspStepper: {name}_margin = {margin!r} must be >= 0")
    if not 0.0 < float(distance) < float("inf"):
        raise ValueError(f"GraspStepper: {name}_distance = {distance!r} must be finite and > 0")
    if int(stations) != stations or not first <= int(stations) <= 32:
        raise ValueError(f"GraspStepper: {name}_stations = {stations!r} must be an integer in {first}..32")


class GraspStepper:
    def __init__(self, hand: ops.HandHandle, object_meshes, surface_points: torch.Tensor, batch_each: int,
                 n_contact: int, weights=None, fc_cfg=None, mala_cfg=None, device="cuda", seed=1,
                 penetration_only: bool = True, energy_type: str = "graspqp", optimizer: str = "mala_star",
                 tdg_directions=None, point_grid: int = 0, split_self_pen: bool = True, n_surface_points: int = 512,
                 surface_samples=None, table_z: float = 0.0, scene=None, scene_margin: float = 0.0,
                 approach_distance: float = 0.10, approach_stations: int = 4, approach_margin=None,
                 pregrasp_opening: float = 0.5, pregrasp_joints=None, pregrasp_scene=None, pregrasp_distance=None,
                 pregrasp_stations=None, pregrasp_margin=None, squeeze_min_travel: float = 5e-3, squeeze_damping: float = 1e-3,
                 arm=None, arm_base=None, reach_distance: float = 0.10, reach_stations: int = 0, reach_iterations: int = 24,
                 reach_damping: float = 1e-4, reach_rot_scale: float = 0.1, arm_scene=None, arm_margin=None, arm_damping: float = 1e-6,
                 track_waypoints: int = 8, track_updates: int = 3, arm_on_track: bool = False,
                 lift_height: float = 0.05, lift_retreat: float = 0.0, lift_stations: int = 4, lift_direction=(0.0, 0.0, 1.0),
                 lift_margin=None, lift_object_margin: float = 0.0, lift_object_samples: int = 512, lift_object_points=None,
                 lift_scene=None, init_avoid_scene: bool = False):
        """object_meshes: an ``ops.MeshSet``, or an ``ops.PointCloudSet`` for objects given as oriented point clouds -- the
        contact query is then gq_cloud_forward, always a launch of its own (the FK forward launch gets no SDF descriptor);
        everything downstream reads the same four buffers.
        energy_type: "graspqp" (default) | "dexgrasp" | "tdg" (scripts/fit.py:343-347); every type has the fused four-
        launch form (the force-closure role of the first stage launch is the contact terms + that energy) and the per-role
        form on two graph branches.  optimizer: "mala_star" | "dexgraspnet"
        (AnnealingDexGraspNet, core/optimizer.py:11-149: no z-score in the temperature, no re-initialisation).
        weights["E_prior"] / weights["E_wall"] > 0 select the tabletop mode (module docstring): the hand surface is sampled
        with ``n_surface_points`` (as HandModel does) unless ``surface_samples`` = (points (Ns,3) in the link frames, link ids
        (Ns)) is given; ``table_z`` is the height of the table plane.
        weights["E_scene"] > 0 selects the scene mode (module docstring) and needs ``scene``, an ``ops.SceneSDF``; the term is
        sum over the same surface samples of max(scene_margin - phi, 0).  With weight 0 a scene changes nothing.
        weights["E_approach"] > 0 selects the approach mode (module docstring) and needs ``scene`` too, with or without a weight
        on "E_scene": the mean over the stations d_k = approach_distance k / approach_stations (k = 1..approach_stations <= 32)
        of the same hinge sum with the whole hand moved back by d_k along the spec's grasp_axis; ``approach_margin`` = None
        takes ``scene_margin``.  With weight 0 the three arguments change nothing.
        ``scene`` may be an ``ops.SceneSDFSet`` with one grid per object (``n_grids`` == n_obj, rows object-major): row b of both
        terms then reads grid b // batch_each (module docstring, "Clutter").
        weights["E_pregrasp"] > 0 selects the pre-grasp mode (module docstring): the mean over the stations k = 0..pregrasp_stations
        of the hinge sum of the hand OPENED to (1 - pregrasp_opening) theta + pregrasp_opening pregrasp_joints and moved back by
        pregrasp_distance k / pregrasp_stations.  ``pregrasp_joints`` (J) = None takes the spec's default state clamped to the joint
        limits; ``pregrasp_scene`` / ``pregrasp_distance`` / ``pregrasp_stations`` / ``pregrasp_margin`` = None take ``scene``,
        ``approach_distance``, ``approach_stations`` and ``scene_margin``.  ``pregrasp_scene`` (an ``ops.SceneSDF``, or an
        ``ops.SceneSDFSet`` with ``n_grids`` == n_obj) exists because this term's grid usually contains the target and the grid of
        E_scene must not.  With weight 0 the six arguments change nothing.
        weights["E_squeeze"] > 0 selects the squeeze mode (module docstring): the mean squared part of the contacts' closing motion
        n_i max(|distance_i|, squeeze_min_travel) that the joints cannot produce, with the damped pseudo-inverse (squeeze_damping) of
        the contact Jacobian; at the defaults the reference's E_manipulativity.  Both must be finite and > 0 (J'J alone is singular
        for 3 n_contact < n_dofs).  ``squeeze_theta`` (B,J) holds the joint velocities of the last evaluation.  With weight 0 the two
        arguments change nothing.
        weights["E_reach"] > 0 selects the reach mode (module docstring) and needs ``arm``, an ``ops.ArmSpec`` or ``ops.ArmHandle``,
        and ``arm_base``, (3,4) or (n_obj,3,4): the arm base in the frame of each object.  ``reach_stations`` in 0..3 stations beyond
        the grasp pose over ``reach_distance`` metres (> 0 when there are stations), ``reach_iterations`` in 0..4096,
        ``reach_damping`` (m^2) and ``reach_rot_scale`` (metres per radian) finite and > 0.  ``reach_q`` / ``reach_seed`` hold the arm
        configurations of the last evaluation.  No default weight is set.  With weight 0 the seven arguments change nothing.
        weights["E_arm"] > 0 selects the arm mode (module docstring): it needs weights["E_reach"] > 0, an ``arm`` with collision spheres
        and ``arm_scene`` (None: ``scene``), an ``ops.SceneSDF`` or an ``ops.SceneSDFSet`` with one grid per object; ``arm_margin`` >= 0
        (None: ``scene_margin``), ``arm_damping`` finite and > 0 (the term's own lambda_a, not ``reach_damping``).
        weights["E_track"] > 0 selects the track mode (module docstring): it needs weights["E_reach"] > 0 with ``reach_stations`` >= 1;
        ``track_waypoints`` in 1..64 waypoints beyond the first, ``track_updates`` in 1..16 updates per waypoint.  ``track_q``,
        ``track_step`` and ``track_worst`` hold the last evaluation.  No default weight is set.  ``arm_on_track`` = True makes E_arm read
        the tracked path's configurations at the stations (``track_station_q``) in place of ``reach_q``: it needs both terms on and
        ``reach_stations`` dividing ``track_waypoints``.  With weight 0 and the switch off the three arguments change nothing.
        weights["E_lift"] > 0 selects the lift mode (module docstring): ``lift_scene`` (an ``ops.SceneSDF``, or an ``ops.SceneSDFSet``
        with one grid per object; None takes ``scene``) must not contain the target; ``lift_height`` and ``lift_retreat`` >= 0 in
        metres, not both zero; ``lift_stations`` in 1..32; ``lift_direction`` in the object's frame, normalised here; ``lift_margin``
        = None takes ``scene_margin``; ``lift_object_margin`` may be negative.  ``lift_object_points`` (n_obj,M,3) are the object's
        points in its own frame; None takes M = min(``lift_object_samples``, P) points of ``surface_points`` at the indices
        floor(j P / M) (the stored order is Morton order, so an even stride is an even cover); M = 0 is the hand alone.
        ``lift_object`` (B) holds the object's share of the last evaluation.  No default weight is set; with weight 0 the
        arguments change nothing."""
        a = types.SimpleNamespace(**locals())  # the arguments, for the terms' checks (which fill in the fall-backs) and binds
        if energy_type not in ("graspqp", "dexgrasp", "tdg") or optimizer not in ("mala_star", "dexgraspnet"):
            raise NotImplementedError(f"energy_type={energy_type!r} / optimizer={optimizer!r}")
        self.energy_type, self.optimizer = energy_type, optimizer
        self.penetration_only = ops.pen_mode(penetration_only)  # 1: E_pen only needs dis > 0 (energy.py:59-61)
        self.split_self_pen = bool(split_self_pen)  # False: A/B switch, self penetration stays in the FK forward launch
        self.hand, self.objs = hand, object_meshes
        self.cloud = isinstance(object_meshes, ops.PointCloudSet)
        self.dev = torch.device(device)
        self.surf = surface_points.to(self.dev, torch.float32).contiguous()  # (n_obj,P,3)
        self.n_obj, self.P = self.surf.shape[0], self.surf.shape[1]
        self.be, self.n = int(batch_each), int(n_contact)
        self.B = self.n_obj * self.be
        self.J, self.L, self.S = hand.J, hand.L, hand.S
        self.D = 9 + self.J
        self.w = merge_weights(weights)
        self._plan = plan = term_plan(self.w)
        self.term_names = plan.term_names
        self._row = {k: i for i, k in enumerate(self.term_names)}
        for t in TERMS:
            setattr(self, t.flag, t.key in plan.launch)
            for k in t.off:
                setattr(self, k, None)
        self.scene, self.scene_margin, self.clutter = None, 0.0, False  # of the terms that read ``scene`` (_check_scene, _bind_scene_arg)
        # every check in declaration order, for the terms that are off too (a rule between terms stands in the later one's check):
        # which error comes first is part of the interface, and all of them come before the first device allocation
        for t in TERMS:
            getattr(self, "_check_" + t.key)(a, getattr(self, t.flag))
        self.init_avoid_scene = bool(init_avoid_scene)
        if self.init_avoid_scene and not (self.scene_mode or self.approach_mode):
            raise ValueError('GraspStepper: init_avoid_scene=True needs weights["E_scene"] > 0 or weights["E_approach"] > 0')
        nT = len(self.term_names)
        self.fc = dict(ops.FC_DEFAULTS)
        if fc_cfg:
            self.fc.update(fc_cfg)
        self.mala = dict(switch_possibility=0.4, starting_temperature=18.0, temperature_decay=0.95, annealing_period=30,
                         step_size=0.005, stepsize_period=50, mu=0.98, clip_grad=False)  # fit.py:42-48
        if mala_cfg:
            self.mala.update(mala_cfg)
        self.cog = self.surf.mean(dim=1).repeat_interleave(self.be, dim=0).contiguous()  # object_model.py:64-68
        self.jlo = torch.tensor(hand.spec.joints_lower, device=self.dev)
        self.jhi = torch.tensor(hand.spec.joints_upper, device=self.dev)
        self.gen = torch.Generator(device=self.dev)
        self.gen.manual_seed(seed)
        B, D, n, P, L, S = self.B, self.D, self.n, self.P, self.L, max(self.S, 1)
        f = lambda *s: torch.zeros(*s, device=self.dev)
        # state
        self.hand_pose, self.grad, self.ema = f(B, D), f(B, D), f(B, D)
        self.contact_idx = torch.zeros(B, n, dtype=torch.long, device=self.dev)
        self.energy = f(B)
        self.step_count = torch.zeros(B, dtype=torch.long, device=self.dev)
        self.terms = f(nT, B)
        # proposal / scratch
        self.pose_new, self.grad_new = f(B, D), f(B, D)
        self.idx_new = torch.zeros(B, n, dtype=torch.long, device=self.dev)
        self.Rg, self.link_T = f(B, 9), f(B, L, 12)
        self.cpts, self.cnrm, self.spheres = f(B, n, 3), f(B, n, 3), f(B, S, 3)
        self.d2, self.onrm, self.closest = f(B, n), f(B, n, 3), f(B, n, 3)
        self.sgn = torch.zeros(B, n, dtype=torch.int32, device=self.dev)
        self.obj_normal, self.g_cpts, self.g_cnrm, self.g_cpts_fc = f(B, n, 3), f(B, n, 3), f(B, n, 3), f(B, n, 3)
        self.pen_dis, self.pen_gvec, self.g_pen = f(B, P), f(B, P, 3), f(B, P)
        self.pen_link = torch.zeros(B, P, dtype=torch.int32, device=self.dev)
        self.wrench, self.gRt = f(B, L, 6), f(B, 12)
        self.e_spen, self.g_sph, self.g_sph_w = f(B), f(B, S, 3), f(B, S, 3)
        self.terms_new, self.total_new = f(nT, B), f(B)
        self.g_theta, self.w_fc_vec = f(B, self.J), torch.full((B,), float(self.w["E_fc"]), device=self.dev)
        self.z, self.temperature, self.s_out = f(B), f(B), f(B)
        self.accept = torch.zeros(B, dtype=torch.uint8, device=self.dev)
        self.g2 = f(D)
        self.u_switch, self.u_accept = f(B, n), f(B)
        self.new_idx = torch.zeros(B, n, dtype=torch.long, device=self.dev)
        self._u_sw, self._u_ac = f(64, B, n), f(64, B)
        self._n_ix = torch.zeros(64, B, n, dtype=torch.long, device=self.dev)
        self._draw_pos = 0
        self._cur = (self.u_switch, self.new_idx, self.u_accept)
        self.n_iter = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self.x_sum = f(B, n)
        self.fk_ws, self.fk_nb = hand.fk_ws(B, self.dev)
        self.fc_nb = ops._size_call("gq_fc_workspace_bytes", ctypes.c_int64(B), n, int(self.fc["n_cone_vecs"]),
                                    int(self.fc["max_iter"]))
        self.fc_ws = ops._ws(self.fc_nb, self.dev).zero_()  # zero once: block counter of the large-batch stop rule
        self._graph, self._graph_iters, self._graph_pending = None, 1, 0
        self._after_reset = False
        self._reinit = None  # 0-dim device flag of the last step_reset: did its mask select any row (fit.py:412)
        self.kernel_events = None
        self._span = torch.zeros(64, 2, dtype=torch.int64, device=self.dev)
        self._span[:, 0] = -1  # {~0, 0}: armed
        self._span_acc = torch.zeros(2, dtype=torch.int64, device=self.dev)
        self._side = None
        self._can_fuse = self.penetration_only == 1  # every energy type has a fused form (gq_fc_pen_step / gq_alt_pen_step)
        # bounding spheres of the 256-point slices of the surface points: block-level link pre-cull of the penetration query
        self.patch = torch.empty(self.n_obj, (self.P + 255) // 256, 4, device=self.dev)
        _C.call("gq_surface_patches", _C.f32(self.surf), ctypes.c_int64(self.n_obj), ctypes.c_int64(self.P), _C.f32(self.patch),
                _C.stream_ptr())
        # link-driven penetration query through a coarse grid over the objects' surface points (0 = the point-driven one)
        self.grid = None
        if self.penetration_only == 1 and point_grid and self.P <= 4096:
            self.grid = ops.PointGrid(self.surf, int(point_grid))
        self.tdg_dirs = None
        if energy_type == "tdg":
            if tdg_directions is None:
                from .metrics.ops.tdg import random_sample_points_on_sphere

                tdg_directions = random_sample_points_on_sphere(3, 1000)
            self.tdg_dirs = torch.as_tensor(tdg_directions, dtype=torch.float32).to(self.dev).contiguous()
        e = _C.RowEnergyDesc()
        e.dist_sq, e.sign, e.obj_dir, e.hand_normals = (t.data_ptr() for t in (self.d2, self.sgn, self.onrm, self.cnrm))
        e.joints_lower, e.joints_upper = self.jlo.data_ptr(), self.jhi.data_ptr()
        e.e_fc, e.e_pen, e.e_spen = (self.terms_new[i].data_ptr() for i in (1, 2, 3))
        e.n = n
        e.w_dis, e.w_fc, e.w_pen, e.w_spen, e.w_joints = (float(self.w[k]) for k in TERM_NAMES)
        e.e_dis, e.e_joints, e.total = self.terms_new[0].data_ptr(), self.terms_new[4].data_ptr(), self.total_new.data_ptr()
        self._row_energy = e
        # descriptors of the fused force-closure + penetration launches (gq_fc_pen_step)
        fc, fd = self.fc, _C.FcStepDesc()
        fd.dist_sq, fd.sign, fd.obj_dir, fd.closest = (t.data_ptr() for t in (self.d2, self.sgn, self.onrm, self.closest))
        fd.contact_pts, fd.hand_normals, fd.cog = self.cpts.data_ptr(), self.cnrm.data_ptr(), self.cog.data_ptr()
        fd.batch, fd.n_contact, fd.n_cone = B, n, int(fc["n_cone_vecs"])
        fd.friction, fd.torque_weight, fd.max_limit = float(fc["friction"]), float(fc["torque_weight"]), float(fc["max_limit"])
        fd.svd_gain, fd.values_gain, fd.eps, fd.max_iter = (float(fc["svd_gain"]), float(fc["values_gain"]), float(fc["eps"]),
                                                            int(fc["max_iter"]))
        fd.w_dis, fd.w_fc = float(self.w["E_dis"]), float(self.w["E_fc"])
        fd.obj_normal, fd.g_contact_pts, fd.g_hand_normals = (t.data_ptr() for t in (self.obj_normal, self.g_cpts, self.g_cnrm))
        fd.e_fc, fd.x_sum, fd.n_iter = self.terms_new[1].data_ptr(), self.x_sum.data_ptr(), self.n_iter.data_ptr()
        fd.workspace, fd.workspace_bytes = self.fc_ws.data_ptr(), self.fc_nb
        pd = _C.PenStepDesc()
        pd.links, pd.surface_points = self.hand.links.handle, self.surf.data_ptr()
        pd.n_obj, pd.n_surface, pd.batch_each, pd.pose_dim = self.n_obj, P, self.be, D
        pd.Rg, pd.link_T = self.Rg.data_ptr(), self.link_T.data_ptr()
        pd.dis, pd.link, pd.gvec = self.pen_dis.data_ptr(), self.pen_link.data_ptr(), self.pen_gvec.data_ptr()
        pd.link_wrench, pd.gRt, pd.w_pen, pd.e_pen = (self.wrench.data_ptr(), self.gRt.data_ptr(), float(self.w["E_pen"]),
                                                      self.terms_new[2].data_ptr())
        pd.span, pd.span_acc = self._span.data_ptr(), self._span_acc.data_ptr()
        pd.grid = self.grid.handle if self.grid is not None else None
        pd.patch_spheres = self.patch.data_ptr()
        if self.S > 0:  # sphere centres + self penetration as a third role of the second fused launch
            pd.hand, pd.w_spen = self.hand.handle, float(self.w["E_spen"])
            pd.e_spen, pd.g_sphere_centers, pd.sphere_centers = (self.terms_new[3].data_ptr(), self.g_sph_w.data_ptr(),
                                                                  self.spheres.data_ptr())
        self._fc_desc, self._pen_desc = fd, pd
        self._alt_desc = None
        if energy_type != "graspqp":  # the fused launches of the other energy types (gq_alt_pen_step)
            ad = _C.AltFcDesc()
            ad.dist_sq, ad.sign, ad.obj_dir, ad.closest = fd.dist_sq, fd.sign, fd.obj_dir, fd.closest
            ad.contact_pts, ad.hand_normals, ad.cog = fd.contact_pts, fd.hand_normals, fd.cog
            ad.batch, ad.n_contact = B, n
            ad.energy = 1 if energy_type == "dexgrasp" else 2
            ad.torque_weight = 0.0  # the reference's call site (core/energy.py:35-42)
            if energy_type == "tdg":
                ad.directions, ad.n_directions = self.tdg_dirs.data_ptr(), int(self.tdg_dirs.shape[0])
                ad.friction, ad.obb_length, ad.enable_density, ad.scale = 0.2, 0.2, 1, 100.0  # as _eval_contacts
            ad.w_dis, ad.w_fc = float(self.w["E_dis"]), float(self.w["E_fc"])
            ad.obj_normal, ad.g_contact_pts, ad.g_hand_normals = fd.obj_normal, fd.g_contact_pts, fd.g_hand_normals
            ad.e_fc = self.terms_new[1].data_ptr()
            self._alt_desc = ad
        # MalaStar.try_step / accept_step as head / tail of the FK kernels
        self._fuse_loop = plan.fuse_loop
        self.samples, self.g_R = None, None
        self._n_surface_points, self._select_fk = int(n_surface_points), None
        self._close_par = (float(a.squeeze_min_travel), float(a.squeeze_damping))  # close() reads them whether the term is on or off
        if plan.needs_samples:  # one set of surface samples for all modes
            if surface_samples is None:
                from .utils import meshes as mesh_utils

                surface_samples = mesh_utils.hand_surface_samples(hand.spec, int(n_surface_points))
            self.samples = ops.SurfaceSamples(hand, surface_samples[0], surface_samples[1], device=self.dev)
            self._axis = ops._axis_c(hand.spec.grasp_axis)  # the float[3] every launch of these modes reads
            # ... and the device pointers of the buffers they read and write, which stay where they are (as the descriptors above
            # hold them): converted and checked here, once, not at every launch
            self._ptr = types.SimpleNamespace(link=_C.i32(self.samples.link), Rg=_C.f32(self.Rg), LT=_C.f32(self.link_T),
                                              wrench=_C.f32(self.wrench), gRt=_C.f32(self.gRt), g_theta=_C.f32(self.g_theta),
                                              e=[_C.f32(self.terms_new[i]) for i in range(nT)])
        on = [t for t in TERMS if getattr(self, t.flag)]
        for t in on:
            getattr(self, "_bind_" + t.key)(a)
        self._launches = [getattr(self, "_launch_" + k) for k in plan.launch]
        # the shares of the total after the FK backward, whose own total holds the five terms: total += w e in declaration order
        # (the order decides the rounding of the fp32 total)
        self._shares = []
        for t in on:
            pairs = [(_C.f32(self.terms_new[self._row[k]]), float(self.w[k])) for k in t.names]
            for group in ([(p,) for p in pairs] if t.total == "gq_scene_total" else [pairs]):
                self._shares.append((t.total, _C.f32(self.total_new), *(x for p in group for x in p), ctypes.c_int64(B)))
        self.init_feasible = torch.zeros(self.n_obj, dtype=torch.int32, device=self.dev)
        self._slot_ctr = torch.zeros(2, dtype=torch.int32, device=self.dev)
        m, pr = self.mala, _C.ProposeDesc()
        pr.hand_pose, pr.grad, pr.contact_idx = self.hand_pose.data_ptr(), self.grad.data_ptr(), self.contact_idx.data_ptr()
        pr.u_switch, pr.new_idx = self._u_sw.data_ptr(), self._n_ix.data_ptr()
        pr.ema, pr.step, pr.step_size_out = self.ema.data_ptr(), self.step_count.data_ptr(), self.s_out.data_ptr()
        pr.g2_scratch = self.g2.data_ptr()
        pr.energy, pr.batch_each, pr.z_out = self.energy.data_ptr(), self.be, self.z.data_ptr()
        pr.step_size, pr.stepsize_period, pr.decay = float(m["step_size"]), int(m["stepsize_period"]), float(m["temperature_decay"])
        pr.mu, pr.switch_possibility, pr.clip_grad = float(m["mu"]), float(m["switch_possibility"]), int(bool(m["clip_grad"]))
        pr.slot_ctr, pr.slots = self._slot_ctr.data_ptr(), 64
        ac = _C.AcceptDesc()
        ac.u_accept, ac.reset_mask, ac.step = self._u_ac.data_ptr(), None, self.step_count.data_ptr()
        ac.z = self.z.data_ptr() if optimizer == "mala_star" else None  # AnnealingDexGraspNet: plain annealing
        ac.starting_temperature, ac.decay, ac.annealing_period = (float(m["starting_temperature"]), float(m["temperature_decay"]),
                                                                  int(m["annealing_period"]))
        ac.energy, ac.pose, ac.idx, ac.grad = (t.data_ptr() for t in (self.energy, self.hand_pose, self.contact_idx, self.grad))
        ac.accept, ac.temperature = self.accept.data_ptr(), self.temperature.data_ptr()
        # the fused accept tail merges the five terms of the FK backward's own total; with an optional term on (six to fifteen
        # terms) the stepper never takes the fused loop (_fuse_loop above) and merges its terms in the stand-alone accept launch
        ac.n_terms, ac.terms_new, ac.terms = len(TERM_NAMES), self.terms_new.data_ptr(), self.terms.data_ptr()
        ac.slot_ctr, ac.slots = self._slot_ctr.data_ptr(), 64
        self._propose_desc, self._accept_desc = pr, ac
        self._sdf_desc = None  # clouds: the query is never attached to the FK forward launch
        if not self.cloud:
            sd = _C.SdfDesc()
            sd.meshes, sd.queries_per_mesh = self.objs.handle, self.be * n
            sd.dist_sq, sd.sign, sd.obj_dir, sd.closest = (t.data_ptr() for t in (self.d2, self.sgn, self.onrm, self.closest))
            self._sdf_desc = sd

    # ---- energy + gradient of the pose in (pose, idx) -> terms_new (5,B), total_new (B), grad_new (B,D) ----------
    # Four pieces: FK (+ self penetration), then two independent branches (contacts -> object SDF -> E_fc fwd+bwd |
    # hand penetration fwd+bwd), then FK backward with the row energies.  ``_evaluate`` runs the branches on two
    # streams when ``fork`` is set (inside a hipGraph capture they become parallel graph branches).
    def _eval_fk(self, pose, idx, st, loop=False, sdf=False, spheres=True):
        B, n = self.B, self.n
        sph = self.S > 0 and spheres  # the fused path computes spheres + self penetration in gq_fc_pen_step instead
        _C.call("gq_fk_forward", self.hand.handle, _C.f32(pose), _C.i64(idx), B, n, _C.f32(self.Rg), _C.f32(self.link_T),
                _C.f32(self.cpts), _C.f32(self.cnrm), _C.f32(self.spheres) if sph else None,
                float(self.w["E_spen"]), _C.f32(self.terms_new[3]) if sph else None,
                _C.f32(self.g_sph_w) if sph else None, ctypes.byref(self._propose_desc) if loop else None,
                ctypes.byref(self._sdf_desc) if sdf else None, _C.ptr(self.fk_ws), self.fk_nb, st)
        self._fk_sdf_attached = bool(sdf)  # whether the last FK forward launch carried the object query
        if self.S == 0:
            _C.call("gq_fill", _C.f32(self.terms_new[3]), 0.0, self.B, st)

    def _eval_object_query(self, st):
        """dist_sq / sign / direction / closest point of the B n contact points on their objects: mesh set or point clouds."""
        _C.call("gq_cloud_forward" if self.cloud else "gq_sdf_forward_meshset", self.objs.handle, _C.f32(self.cpts),
                self.B * self.n, self.be * self.n, _C.f32(self.d2), _C.i32(self.sgn), _C.f32(self.onrm), _C.f32(self.closest), st)

    def _eval_contacts(self, st):
        B, n, w, fc = self.B, self.n, self.w, self.fc
        C, f32, i32 = _C.call, _C.f32, _C.i32
        e_fc = self.terms_new[1]
        self._eval_object_query(st)
        if self.energy_type != "graspqp":
            # E_dis terms (+ outward object normals), then the other force-closure energy adds w_fc dE/dp in one launch
            C("gq_contact_terms", f32(self.d2), i32(self.sgn), f32(self.onrm), f32(self.closest), f32(self.cpts),
              f32(self.cnrm), ctypes.c_int64(B), n, float(w["E_dis"]), f32(self.obj_normal), f32(self.g_cpts), f32(self.g_cnrm), st)
            if self.energy_type == "dexgrasp":  # torque_weight = 0 at the reference's call site (core/energy.py:35-42)
                C("gq_dexgrasp_energy", f32(self.cpts), f32(self.obj_normal), f32(self.cog), ctypes.c_int64(B), n, 0.0, None,
                  float(w["E_fc"]), 1, f32(e_fc), f32(self.g_cpts), st)
            else:
                C("gq_tdg_energy", f32(self.cpts), f32(self.obj_normal), f32(self.cog), f32(self.tdg_dirs), self.tdg_dirs.shape[0],
                  ctypes.c_int64(B), n, 0.2, 0.2, 1, 100.0, None, float(w["E_fc"]), 1, f32(e_fc), f32(self.g_cpts), st)
            return
        C("gq_fc_step", f32(self.d2), i32(self.sgn), f32(self.onrm), f32(self.closest), f32(self.cpts), f32(self.cnrm),
          f32(self.cog), B, n, int(fc["n_cone_vecs"]), float(fc["friction"]), float(fc["torque_weight"]),
          float(fc["max_limit"]), float(fc["svd_gain"]), float(fc["values_gain"]), float(fc["eps"]), int(fc["max_iter"]),
          float(w["E_dis"]), float(w["E_fc"]), f32(self.obj_normal), f32(self.g_cpts), f32(self.g_cnrm), f32(e_fc),
          f32(self.x_sum), i32(self.n_iter), _C.ptr(self.fc_ws), self.fc_nb, st)

    def _eval_spen(self, pose, st):
        _C.call("gq_spheres_self_pen", self.hand.handle, _C.f32(pose), self.D, _C.f32(self.Rg), _C.f32(self.link_T),
                ctypes.c_int64(self.B), float(self.w["E_spen"]), _C.f32(self.spheres), _C.f32(self.terms_new[3]),
                _C.f32(self.g_sph_w), st)

    def _eval_pen(self, pose, st, timer=None):
        """Hand-penetration query (the roofline kernel of bench.py) + its backward.  ``timer`` = HIP event pair around
        the query (hipExtLaunchKernelGGL start/stop events).  The query also records its own execution span in
        100 MHz s_memrealtime ticks (64 shards of {min block start, max block end}); the backward launch folds them
        into ``_span_acc`` = {sum, launches}, which works inside a hipGraph replay too."""
        if self.grid is not None:
            _C.call("gq_hand_pen_forward_cells", self.hand.links.handle, self.grid.handle, _C.f32(self.surf), self.n_obj, self.P,
                    self.be, _C.f32(pose), self.D, _C.f32(self.Rg), _C.f32(self.link_T), _C.f32(self.pen_dis),
                    _C.i32(self.pen_link), _C.f32(self.pen_gvec), timer, _C.ptr(self._span), st)
        else:
            _C.call("gq_hand_pen_forward", self.hand.links.handle, _C.f32(self.surf), self.n_obj, self.P, self.be,
                    _C.f32(pose), self.D, _C.f32(self.Rg), _C.f32(self.link_T), int(self.penetration_only),
                    _C.f32(self.pen_dis), _C.i32(self.pen_link), _C.f32(self.pen_gvec),
                    None, 0, timer, _C.ptr(self._span), _C.f32(self.patch), st)
        _C.call("gq_hand_pen_backward", self.L, _C.f32(self.surf), self.n_obj, self.P, self.be, _C.f32(pose), self.D,
                _C.f32(self.Rg), None, _C.i32(self.pen_link), _C.f32(self.pen_gvec), _C.f32(self.wrench), _C.f32(self.gRt),
                _C.f32(self.pen_dis), float(self.w["E_pen"]), _C.f32(self.terms_new[2]), _C.ptr(self._span),
                _C.ptr(self._span_acc), st)

    # ---- the optional terms (module table TERMS): per key a check (host only: the constructor's arguments ``a``, fall-backs filled
    # in, errors raised; called whether the term is ``on`` or not), a bind (buffers, public attributes, pointers converted once, the
    # grid struct; only when on) and a launch (pose, idx, st) -------------------------------------------------------------------
    def term_row(self, name):
        """The row of ``terms`` / ``terms_new`` that holds the term ``name``; KeyError when it is switched off."""
        return self._row[name]

    def _zeros(self, *shape):
        return torch.zeros(*shape, device=self.dev)

    def _check_n_grids(self, name, scene):
        if isinstance(scene, ops.SceneSDFSet) and scene.n_grids != self.n_obj:
            raise ValueError(f"GraspStepper: {name} has n_grids = {scene.n_grids}, the stepper has n_obj = {self.n_obj} objects")

    def _scene_arg(self, term, name, given, fallback=None):
        """The grid that ``term`` reads: its argument ``name``, or ``fallback`` (the argument ``scene``) where that is None -- an
        ops.SceneSDF, or an ops.SceneSDFSet with one grid per object (of ``scene`` itself the clutter rule of _check_scene asks that)."""
        scene = fallback if given is None else given
        if not isinstance(scene, (ops.SceneSDF, ops.SceneSDFSet)):
            arg = "scene=" if name == "scene" else f"{name}= or scene="
            raise ValueError(f'GraspStepper: weights["{term}"] > 0 needs {arg}ops.SceneSDF(...) or ops.SceneSDFSet(...)')
        if name != "scene":
            self._check_n_grids(name, scene)
        return scene

    def _bind_scene_arg(self, a):
        """What scene and approach share: the public ``scene`` / ``scene_margin`` and the grid struct of both launches, the stack
        (clutter) or the one grid."""
        self.scene, self.scene_margin = a.scene, float(a.scene_margin)
        self._scene_grid = a.scene.grid_set if self.clutter else a.scene.grid

    def _check_tabletop(self, a, on):
        pass

    def _bind_tabletop(self, a):
        self.g_R = self._zeros(self.B, 9)
        self.table_z = float(a.table_z)
        # d (w_prior E_prior) / d R = w_prior * grasp_axis in row 2 does not depend on the pose: set here, once; the launch
        # of every evaluation adds to wrench / gRt and is given no g_R
        self.g_R[:, 6:9] = float(self.w["E_prior"]) * torch.tensor(list(self._axis), device=self.dev)

    def _launch_tabletop(self, pose, idx, st):
        """E_prior / E_wall -> terms_new[5:7]; the gradient of w_wall E_wall is added to the penetration branch's link
        wrenches and gRt (inputs of the FK backward, like the constant g_R of w_prior E_prior)."""
        p = self._ptr
        ops._tabletop_call(pose, self.samples.points, p.link, self.L, p.Rg, p.LT, self._axis, self.table_z, None, self.w["E_wall"],
                           None, self.w["E_prior"], p.e[self._row["E_wall"]], p.e[self._row["E_prior"]], 1, p.wrench, p.gRt, None, st)

    def _check_scene(self, a, on):
        if on:
            self._scene_arg("E_scene", "scene", a.scene)
        # two rules of the argument that scene and approach share, whichever of them is on.  scene_margin is the fall-back of
        # every grid term's margin; clutter: one grid per object, the two launches pick the grid from the row (row // batch_each)
        if not float(a.scene_margin) >= 0.0:
            raise ValueError(f"GraspStepper: scene_margin = {a.scene_margin!r} must be >= 0")
        self.clutter = (on or self.approach_mode) and isinstance(a.scene, ops.SceneSDFSet)
        if self.clutter:
            self._check_n_grids("scene", a.scene)

    def _bind_scene(self, a):
        self._bind_scene_arg(a)
        B, L, Ns = self.B, self.L, self.samples.Ns
        a.scene.check(B, self.be, L, Ns) if self.clutter else a.scene.check(B, L, Ns)

    def _launch_scene(self, pose, idx, st):
        """E_scene -> its row of terms_new; the gradient of w_scene E_scene is added to the link wrenches and gRt that the FK
        backward reads."""
        p = self._ptr
        ops._scene_call(self._scene_grid, self.scene_margin, pose, self.samples.points, p.link, self.L, p.Rg, p.LT, None,
                        self.w["E_scene"], p.e[self._row["E_scene"]], 1, p.wrench, p.gRt, st)

    def _check_approach(self, a, on):
        if on:
            self._scene_arg("E_approach", "scene", a.scene)
            a.approach_margin = a.scene_margin if a.approach_margin is None else a.approach_margin
            _check_corridor("approach", a.approach_margin, a.approach_distance, a.approach_stations, 1)

    def _bind_approach(self, a):
        self._bind_scene_arg(a)
        self.approach_distance, self.approach_stations = float(a.approach_distance), int(a.approach_stations)
        self.approach_margin = float(a.approach_margin)
        ops.approach_check(a.scene, self.B, self.L, self.samples.Ns, self.approach_distance, self.approach_stations,
                           self.hand.spec.grasp_axis)

    def _launch_approach(self, pose, idx, st):
        """E_approach -> its row of terms_new; the gradient of w_approach E_approach is added to the link wrenches and gRt that the
        FK backward reads."""
        p = self._ptr
        ops._approach_call(self._scene_grid, self.approach_margin, self.approach_distance, self.approach_stations, pose,
                           self.samples.points, p.link, self.L, p.Rg, p.LT, self._axis, None, self.w["E_approach"],
                           p.e[self._row["E_approach"]], 1, p.wrench, p.gRt, st)

    def _check_pregrasp(self, a, on):
        if on:
            a.pregrasp_scene = self._scene_arg("E_pregrasp", "pregrasp_scene", a.pregrasp_scene, a.scene)
            a.pregrasp_margin = a.scene_margin if a.pregrasp_margin is None else a.pregrasp_margin
            a.pregrasp_distance = a.approach_distance if a.pregrasp_distance is None else a.pregrasp_distance
            a.pregrasp_stations = a.approach_stations if a.pregrasp_stations is None else a.pregrasp_stations
            _check_corridor("pregrasp", a.pregrasp_margin, a.pregrasp_distance, a.pregrasp_stations, 0)
            if not 0.0 <= float(a.pregrasp_opening) <= 1.0:
                raise ValueError(f"GraspStepper: pregrasp_opening = {a.pregrasp_opening!r} must be in [0, 1]")

    def _bind_pregrasp(self, a):
        self.pregrasp_scene = a.pregrasp_scene
        self.pregrasp_distance, self.pregrasp_stations = float(a.pregrasp_distance), int(a.pregrasp_stations)
        self.pregrasp_margin, self.pregrasp_opening = float(a.pregrasp_margin), float(a.pregrasp_opening)
        if a.pregrasp_joints is None:
            self.pregrasp_joints = ops.default_open_joints(self.hand.spec, self.dev)
        else:
            self.pregrasp_joints = torch.as_tensor(a.pregrasp_joints, dtype=torch.float32).detach().to(self.dev).contiguous()
        if self.pregrasp_joints.shape != (self.J,):
            raise ValueError(f"GraspStepper: pregrasp_joints must be ({self.J},), got {tuple(self.pregrasp_joints.shape)}")
        ops.pregrasp_check(a.pregrasp_scene, self.B, self.L, self.samples.Ns, self.pregrasp_distance, self.pregrasp_stations,
                           self.hand.spec.grasp_axis, self.pregrasp_opening)
        self._ptr.joints = _C.f32(self.pregrasp_joints)
        # the stack view of the grid (a single grid is the stack of one): row b reads grid b // (B / n_grids)
        self._pregrasp_grids = ops._pregrasp_grids(a.pregrasp_scene.values, a.pregrasp_scene.origin, a.pregrasp_scene.voxel)

    def _launch_pregrasp(self, pose, idx, st):
        """E_pregrasp -> its row of terms_new; the root-pose part of the gradient of w_pregrasp E_pregrasp is added to the gRt that the
        FK backward reads (the opened hand shares the closed hand's root pose), the joint part overwrites ``g_theta``."""
        p = self._ptr
        ops._pregrasp_call(self.hand, self._pregrasp_grids, self.pregrasp_margin, self.pregrasp_distance, self.pregrasp_stations,
                           self.pregrasp_opening, p.joints, pose, self.samples.points, p.link, p.Rg, self._axis, None,
                           self.w["E_pregrasp"], p.e[self._row["E_pregrasp"]], 1, p.g_theta, p.gRt, st)

    def _check_squeeze(self, a, on):
        if on:
            ops.squeeze_check(a.hand, a.n_contact, a.squeeze_min_travel, a.squeeze_damping, "GraspStepper")

    def _bind_squeeze(self, a):
        self.squeeze_min_travel, self.squeeze_damping = float(a.squeeze_min_travel), float(a.squeeze_damping)
        self.squeeze_theta = self._zeros(self.B, self.J)
        # the g_R the FK backward reads in this mode: written by every evaluation (E_prior's constant + this term's part)
        self._g_R_const, self.g_R = self.g_R, self._zeros(self.B, 9)

    def _launch_squeeze(self, pose, idx, st):
        """E_squeeze -> its row of terms_new, the joint velocities -> ``squeeze_theta``; the gradient of w_squeeze E_squeeze is added to
        ``g_cpts`` (the contact branch has written it), written to ``g_theta`` (added when the pre-grasp launch has written it) and
        written, on top of E_prior's constant, to the ``g_R`` the FK backward reads."""
        ops._squeeze_call(self.hand, idx, self.Rg, self.link_T, self.fk_ws, self.d2, self.obj_normal, self.closest, self.cpts,
                          self.squeeze_min_travel, self.squeeze_damping, None, self.w["E_squeeze"], self.terms_new[self._row["E_squeeze"]],
                          self.squeeze_theta, 3 if self.pregrasp_mode else 1, self.g_theta, self.g_R, self._g_R_const, self.g_cpts, st)

    def _check_reach(self, a, on):
        if on:
            if not isinstance(a.arm, (ops.ArmSpec, ops.ArmHandle)):
                raise ValueError('GraspStepper: weights["E_reach"] > 0 needs arm=ops.ArmSpec(...) or ops.ArmHandle(...)')
            if a.arm_base is None:
                raise ValueError('GraspStepper: weights["E_reach"] > 0 needs arm_base, (3,4) or (n_obj,3,4)')
            ops.reach_check(a.arm, a.reach_distance, a.reach_stations, a.reach_iterations, a.reach_damping, a.reach_rot_scale,
                            a.hand.spec.grasp_axis, "GraspStepper")
            a.arm_base = ops.reach_base(a.arm_base, self.n_obj, "GraspStepper")

    def _bind_reach(self, a):
        self.arm = a.arm if isinstance(a.arm, ops.ArmHandle) else ops.ArmHandle(a.arm, self.dev)
        self.arm_base = a.arm_base.to(self.dev)
        self.reach_distance, self.reach_stations, self.reach_iterations = float(a.reach_distance), int(a.reach_stations), int(a.reach_iterations)
        self.reach_damping, self.reach_rot_scale = float(a.reach_damping), float(a.reach_rot_scale)
        self.reach_q = self._zeros(self.B, self.reach_stations + 1, self.arm.N)
        self.reach_seed = torch.zeros(self.B, self.reach_stations + 1, dtype=torch.int32, device=self.dev)
        self._reach_axis = (ctypes.c_float * 3)(*(float(x) for x in self.hand.spec.grasp_axis))

    def _launch_reach(self, pose, idx, st):
        """E_reach -> its row of terms_new, the winning arm configurations -> ``reach_q`` / ``reach_seed``; the gradient of w_reach E_reach
        is ADDED to ``gRt`` (the penetration branch has written it).  g_R and g_theta are not touched."""
        ops._reach_call(self.arm, pose, self.Rg, self.arm_base, self.be, self._reach_axis, self.reach_distance, self.reach_stations,
                        self.reach_iterations, self.reach_damping, self.reach_rot_scale, None, self.w["E_reach"],
                        self.terms_new[self._row["E_reach"]], self.reach_q, self.reach_seed, 1, self.gRt, st)

    def _check_arm(self, a, on):
        if on:
            if not self.reach_mode:
                raise ValueError('GraspStepper: weights["E_arm"] > 0 needs weights["E_reach"] > 0: the term reads the reach term\'s reach_q')
            if not (a.arm.spec if isinstance(a.arm, ops.ArmHandle) else a.arm).n_spheres:
                raise ValueError('GraspStepper: weights["E_arm"] > 0 needs an arm with collision spheres (ArmSpec.with_spheres / '
                                 'with_link_spheres)')
            a.arm_scene = self._scene_arg("E_arm", "arm_scene", a.arm_scene, a.scene)
            a.arm_margin = a.scene_margin if a.arm_margin is None else a.arm_margin
            ops.arm_check(a.arm, ops._arm_scene_grids(a.arm_scene, "GraspStepper"), self.B, a.arm_margin, a.arm_damping, a.reach_rot_scale,
                          a.reach_distance, a.reach_stations, a.hand.spec.grasp_axis, "GraspStepper")

    def _bind_arm(self, a):
        self.arm_scene, self.arm_margin, self.arm_damping = a.arm_scene, float(a.arm_margin), float(a.arm_damping)
        self._arm_grids = ops._arm_scene_grids(a.arm_scene, "GraspStepper")  # the stack view: a single grid is the stack of one

    def _launch_arm(self, pose, idx, st):
        """E_arm -> its row of terms_new from the ``reach_q`` the reach launch of this evaluation has just written (``track_station_q``
        of the track launch with ``arm_on_track``); the gradient of w_arm E_arm is ADDED to ``gRt``.  g_R and g_theta are not touched."""
        ops._arm_call(self.arm, self._arm_grids, self.arm_margin, self.arm_damping, self.reach_rot_scale, pose, self.Rg, self.arm_base,
                      self.be, self._reach_axis, self.reach_distance, self.reach_stations,
                      self.track_station_q if self.arm_on_track else self.reach_q, None, self.w["E_arm"],
                      self.terms_new[self._row["E_arm"]], 1, self.gRt, st)

    def _check_track(self, a, on):
        if on:
            if not self.reach_mode:
                raise ValueError('GraspStepper: weights["E_track"] > 0 needs weights["E_reach"] > 0: the path starts at the reach term\'s '
                                 'reach_q[:, reach_stations]')
            if int(a.reach_stations) < 1:
                raise ValueError('GraspStepper: weights["E_track"] > 0 needs reach_stations >= 1: the path starts at the retreated station')
            ops.track_check(a.arm, a.reach_distance, a.track_waypoints, a.track_updates, a.reach_damping, a.reach_rot_scale,
                            a.hand.spec.grasp_axis, a.reach_stations, False, "GraspStepper")
        self.arm_on_track = bool(a.arm_on_track)  # the switch between arm and track: checked with the later of the two
        if self.arm_on_track:
            if not (on and self.arm_mode):
                raise ValueError('GraspStepper: arm_on_track=True needs weights["E_track"] > 0 and weights["E_arm"] > 0')
            if int(a.track_waypoints) % int(a.reach_stations):
                raise ValueError(f"GraspStepper: arm_on_track=True needs reach_stations = {a.reach_stations} to divide track_waypoints = "
                                 f"{a.track_waypoints}")

    def _bind_track(self, a):
        self.track_waypoints, self.track_updates = int(a.track_waypoints), int(a.track_updates)
        self.track_q = self._zeros(self.B, self.track_waypoints + 1, self.arm.N)
        self.track_step, self.track_worst = self._zeros(self.B), self._zeros(self.B)
        if self.arm_on_track:
            self.track_station_q = self._zeros(self.B, self.reach_stations + 1, self.arm.N)

    def _launch_track(self, pose, idx, st):
        """E_track -> its row of terms_new from the start configuration ``reach_q[:, K]`` the reach launch of this
        evaluation has just written (a view: pointer and row stride, no copy); the path -> ``track_q``, ``track_step``,
        ``track_worst`` (and ``track_station_q`` for ``arm_on_track``); the gradient of w_track E_track is ADDED to ``gRt``.  g_R and
        g_theta are not touched."""
        ops._track_call(self.arm, pose, self.Rg, self.arm_base, self.be, self._reach_axis, self.reach_distance, self.track_waypoints,
                        self.track_updates, self.reach_damping, self.reach_rot_scale, self.reach_q[:, self.reach_stations],
                        self.reach_stations, None, self.w["E_track"], self.terms_new[self._row["E_track"]], self.track_q, self.track_worst,
                        self.track_step, self.track_station_q, 1, self.gRt, st)

    def _check_lift(self, a, on):
        if not on:
            return
        a.lift_scene = self._scene_arg("E_lift", "lift_scene", a.lift_scene, a.scene)
        a.lift_margin = a.scene_margin if a.lift_margin is None else a.lift_margin
        pts = a.lift_object_points
        if pts is None:
            if int(a.lift_object_samples) != a.lift_object_samples or int(a.lift_object_samples) < 0:
                raise ValueError(f"GraspStepper: lift_object_samples = {a.lift_object_samples!r} must be an integer >= 0")
            M = min(int(a.lift_object_samples), self.P)
            pick = (torch.arange(M, device=self.dev) * self.P) // max(M, 1)  # floor(j P / M)
            pts = self.surf[:, pick]
        a.lift_object_points = pts = torch.as_tensor(pts, dtype=torch.float32).detach().to(self.dev).contiguous()
        if pts.dim() != 3 or pts.shape[0] != self.n_obj or pts.shape[2] != 3:
            raise ValueError(f"GraspStepper: lift_object_points must be ({self.n_obj}, M, 3), got {tuple(pts.shape)}")
        try:
            a.lift_direction = ops.lift_direction(a.lift_direction)
        except ValueError:
            raise ValueError(f"GraspStepper: lift_direction = {a.lift_direction!r} must be three finite numbers, not all zero") from None
        for name in ("lift_height", "lift_retreat"):
            if not 0.0 <= float(getattr(a, name)) < float("inf"):
                raise ValueError(f"GraspStepper: {name} = {getattr(a, name)!r} must be finite and >= 0")
        if not float(a.lift_height) + float(a.lift_retreat) > 0.0:
            raise ValueError("GraspStepper: lift_height and lift_retreat must not both be zero")
        if int(a.lift_stations) != a.lift_stations or not 1 <= int(a.lift_stations) <= 32:
            raise ValueError(f"GraspStepper: lift_stations = {a.lift_stations!r} must be an integer in 1..32")
        if not 0.0 <= float(a.lift_margin) < float("inf"):
            raise ValueError(f"GraspStepper: lift_margin = {a.lift_margin!r} must be finite and >= 0")
        if not abs(float(a.lift_object_margin)) < float("inf"):
            raise ValueError(f"GraspStepper: lift_object_margin = {a.lift_object_margin!r} must be finite")

    def _bind_lift(self, a):
        self.lift_scene, self.lift_object_points, self.lift_object = a.lift_scene, a.lift_object_points, self._zeros(self.B)
        self.lift_height, self.lift_retreat, self.lift_stations = float(a.lift_height), float(a.lift_retreat), int(a.lift_stations)
        self.lift_margin, self.lift_object_margin = float(a.lift_margin), float(a.lift_object_margin)
        self.lift_direction = tuple(a.lift_direction)
        self._lift_u = ops._axis_c(a.lift_direction)
        self._lift_grids = ops._pregrasp_grids(a.lift_scene.values, a.lift_scene.origin, a.lift_scene.voxel)  # a single grid: the stack of one
        ops.lift_check(a.lift_scene, self.B, self.L, self.samples.Ns, self.n_obj, self.be, a.lift_object_points.shape[1], self.lift_height,
                       self.lift_retreat, self.lift_stations, self.hand.spec.grasp_axis, a.lift_direction, self.lift_margin,
                       self.lift_object_margin, "GraspStepper")
        self._ptr.lift_points, self._ptr.lift_object = _C.f32(self.lift_object_points), _C.f32(self.lift_object)

    def _launch_lift(self, pose, idx, st):
        """E_lift -> its row of terms_new, the object's share -> ``lift_object``; the gradient of w_lift E_lift is added
        to the link wrenches and gRt that the FK backward reads.  g_R and g_theta are not touched."""
        p = self._ptr
        ops._lift_call(self._lift_grids, self.lift_margin, self.lift_object_margin, self.lift_height, self.lift_retreat, self.lift_stations,
                       pose, self.samples.points, p.link, self.L, p.Rg, p.LT, p.lift_points, self.n_obj, self.be,
                       self.lift_object_points.shape[1], self._axis, self._lift_u, None, self.w["E_lift"], p.e[self._row["E_lift"]],
                       p.lift_object, 1, p.wrench, p.gRt, st)

    def _eval_tail(self, pose, idx, st, loop=False):
        B, n = self.B, self.n
        f32 = _C.f32
        _C.call("gq_fk_backward", self.hand.handle, f32(pose), _C.i64(idx), B, n, f32(self.Rg), f32(self.link_T),
                f32(self.g_cpts), f32(self.g_cnrm), f32(self.g_sph_w) if self.S > 0 else None, f32(self.wrench),
                f32(self.gRt), f32(self.g_theta) if self._plan.g_theta else None, f32(self.g_R), f32(self.grad_new),
                ctypes.byref(self._row_energy),
                ctypes.byref(self._accept_desc) if loop else None, _C.ptr(self.fk_ws), self.fk_nb, st)

    def _evaluate(self, pose, idx, st, fork=False, timer=None, fused=False, loop=False):
        """loop=True: one whole MALA* iteration -- the proposal is the head of the FK forward kernel (pose / idx are its
        outputs), the accept step the tail of the FK backward kernel."""
        # small batches: the contact queries ride along with the kinematics (latency); large ones: their own launch
        # (throughput -- query wavefronts should not hold slots while wavefront 0 of their block does the kinematics)
        attach = fused and self.B <= 512 and not self.cloud
        # per-role launches, 384..1023 rows: sphere centres + self penetration leave the FK forward launch (which both
        # branches wait for) and ride on the penetration branch, as in the fused form (same device code, same bits):
        # +3.9 % at 512 rows.  From 2048 rows on that branch is the longer one (-1.1 %), and a third graph branch for the
        # role loses at every size (-3.6 % at 512, -1 % at 1024, 0 at 2048), so there it stays in the FK forward launch.
        split_spen = not fused and self.S > 0 and 384 <= self.B < 1024 and self.split_self_pen
        self._eval_fk(pose, idx, st, loop, sdf=attach, spheres=not fused and not split_spen)
        if fused:
            if not attach:
                self._eval_object_query(st)
            # both branches side by side in two launches
            self._pen_desc.hand_pose = pose.data_ptr()
            if self._alt_desc is None:
                _C.call("gq_fc_pen_step", ctypes.byref(self._fc_desc), ctypes.byref(self._pen_desc), st)
            else:
                _C.call("gq_alt_pen_step", ctypes.byref(self._alt_desc), ctypes.byref(self._pen_desc), st)
        elif not fork:
            self._eval_contacts(st)
            if split_spen:
                self._eval_spen(pose, st)
            self._eval_pen(pose, st, timer)
        else:
            main = torch.cuda.current_stream()
            sb = self._side
            sb.wait_stream(main)
            self._eval_contacts(st)
            if split_spen:
                self._eval_spen(pose, ctypes.c_void_p(sb.cuda_stream))
            self._eval_pen(pose, ctypes.c_void_p(sb.cuda_stream), timer)
            main.wait_stream(sb)
        for launch in self._launches:  # the optional terms that are on, in launch order: they add to what the FK backward reads
            launch(pose, idx, st)
        self._eval_tail(pose, idx, st, loop)
        for args in self._shares:  # the FK backward's total holds the five terms: total += w e, in declaration order
            _C.call(*args, st)

    def evaluate(self, pose, idx):
        """Energy terms, total and d total / d pose at an arbitrary (pose, idx); returns clones."""
        self.pose_new.copy_(pose)
        self.idx_new.copy_(idx)
        self._evaluate(self.pose_new, self.idx_new, _C.stream_ptr())
        return ({k: self.terms_new[i].clone() for i, k in enumerate(self.term_names)}, self.total_new.clone(),
                self.grad_new.clone())

    def reset(self, hand_pose, contact_idx):
        """fit.py:381-396: first energy evaluation; the first gradient is zeroed (optimizer.zero_grad())."""
        self.hand_pose.copy_(hand_pose)
        self.contact_idx.copy_(contact_idx)
        self._evaluate(self.hand_pose, self.contact_idx, _C.stream_ptr())
        self.energy.copy_(self.total_new)
        self.terms.copy_(self.terms_new)
        self.grad.zero_()
        self.ema.zero_()
        self.step_count.zero_()

    def draw(self, draws=None):
        """Random draws of one iteration (optimizer.py:253-257,305): full-size draws + select (no host sync),
        generated 64 iterations at a time (3 generator launches per 64 iterations).  The kernels pick the current slot
        themselves (device counter ``_slot_ctr``, mirrored by ``_draw_pos``).  ``draws`` injects one iteration."""
        k = self._draw_pos
        if draws is not None:
            self._u_sw[k].copy_(draws[0])
            self._n_ix[k].copy_(draws[1])
            self._u_ac[k].copy_(draws[2])
        elif k == 0:
            self._u_sw.uniform_(generator=self.gen)
            self._n_ix.random_(0, self.hand.spec.n_contact_candidates, generator=self.gen)
            self._u_ac.uniform_(generator=self.gen)
        self._cur = (self._u_sw[k], self._n_ix[k], self._u_ac[k])
        self._draw_pos = (k + 1) % 64

    def _propose(self, st):
        """MalaStar.try_step + z-score of the old energies; launched eagerly so that it can read this iteration's slice
        of the pre-generated random draws directly (no copy)."""
        B, D, n, m = self.B, self.D, self.n, self.mala
        C, f32, i64 = _C.call, _C.f32, _C.i64
        C("gq_mala_propose", f32(self.hand_pose), f32(self.grad), i64(self.contact_idx), f32(self._cur[0]),
          i64(self._cur[1]), B, D, n, float(m["step_size"]), int(m["stepsize_period"]), float(m["temperature_decay"]),
          float(m["mu"]), float(m["switch_possibility"]), int(bool(m["clip_grad"])), f32(self.ema), i64(self.step_count),
          f32(self.pose_new), i64(self.idx_new), f32(self.s_out), f32(self.g2), f32(self.energy), self.be, f32(self.z),
          st)  # the z-score of the OLD energies (fit.py:403-406) rides in the same launch

    def _accept(self, st, reset_mask=None):
        """MalaStar.accept_step + state merge; the rows of ``reset_mask`` (uint8, device) are accepted unconditionally."""
        B, D, n, m = self.B, self.D, self.n, self.mala
        C, f32, i64 = _C.call, _C.f32, _C.i64
        C("gq_mala_accept", f32(self.total_new), f32(self._cur[2]), f32(self.z) if self.optimizer == "mala_star" else None,
          _C.u8(reset_mask), i64(self.step_count), f32(self.pose_new), i64(self.idx_new), f32(self.grad_new), B, D, n,
          float(m["starting_temperature"]), float(m["temperature_decay"]), int(m["annealing_period"]), f32(self.energy),
          f32(self.hand_pose), i64(self.contact_idx), f32(self.grad), _C.u8(self.accept), f32(self.temperature),
          len(self.term_names), f32(self.terms_new), f32(self.terms), st)

    def start_kernel_timing(self):
        """Time the hand-penetration query from now on (bench.py): clears the in-kernel span accumulator; outside a
        hipGraph every launch additionally gets a HIP event pair."""
        self._span_acc.zero_()
        self.kernel_events = []

    def kernel_times_ms(self):
        """-> (event_ms list, span_ms mean, launches): HIP-event durations of the eagerly launched queries and the mean
        in-kernel s_memrealtime span (100 MHz) of all queries since ``start_kernel_timing``."""
        ev_ms = []
        for t in self.kernel_events or []:
            ms = ctypes.c_float(0)
            _C.call("gq_timer_elapsed_ms", t, ctypes.byref(ms))
            _C.call("gq_timer_destroy", t)
            ev_ms.append(float(ms.value))
        acc = self._span_acc.cpu()
        n = int(acc[1])
        span_ms = (float(acc[0]) / max(n, 1)) / 1e5  # ticks of 10 ns -> ms
        self.kernel_events = None
        return ev_ms, span_ms, n

    def _iteration(self, st, timer=None, fork=False, fused=False):
        """One MALA* iteration as launches on ``st`` (eager, or under hipGraph capture)."""
        if self._fuse_loop:
            self._evaluate(self.pose_new, self.idx_new, st, fork=fork, timer=timer, fused=fused, loop=True)
        else:
            self._propose(st)
            self._evaluate(self.pose_new, self.idx_new, st, fork=fork, timer=timer, fused=fused)
            self._accept(st)

    def step(self, draws=None):
        """One MALA* iteration.  ``draws`` = (u_switch, new_idx, u_accept) to inject random numbers (tests)."""
        if self._after_reset:
            return self._step_after_reset(draws)
        if self._graph_pending and self._draw_pos == 0:
            self.flush()  # queued iterations still need the draws that the refill below would overwrite
        self.draw(draws)
        st = _C.stream_ptr()
        if self._graph is not None and self._fuse_loop:
            if self._graph_iters > 1:  # the captured graph holds several iterations: replay it once per group
                self._graph_pending += 1
                if self._graph_pending == self._graph_iters:
                    self._graph.replay()
                    self._graph_pending = 0
                return
            self._graph.replay()
        elif self._graph is not None:
            self._propose(st)
            self._graph.replay()
            self._accept(st)
        else:
            timer = None
            if self.kernel_events is not None and len(self.kernel_events) < 4096:
                timer = ctypes.c_void_p(0)
                _C.call("gq_timer_create", ctypes.byref(timer))
                self.kernel_events.append(timer)
            self._iteration(st, timer=timer)

    def _step_after_reset(self, draws=None):
        """The iteration that follows a re-initialisation.  Reference quirk: HandModel.set_parameters(env_mask=...) makes
        hand_pose a leaf tensor (hand_model.py:846-851), and in the next iteration autograd accumulates the new gradient
        IN PLACE into that leaf's .grad -- the tensor MalaStar keeps as old_grad_hand_pose (optimizer.py:266) -- so the
        rows rejected in that iteration get old + new gradient back (optimizer.py:333-338).  Launched eagerly with the
        stand-alone propose / accept kernels; pinned by tests/golden/mala_ext_*.npz."""
        self.flush()
        self.draw(draws)
        st = _C.stream_ptr()
        self._propose(st)
        self._evaluate(self.pose_new, self.idx_new, st)
        self._accept(st)
        # ``_reinit`` (0-dim bool, device): whether the reset iteration re-initialised any row at all -- after an empty mask
        # no leaf pose was created (fit.py:412) and this is an ordinary iteration
        rej = ((self.accept == 0) & self._reinit).unsqueeze(1)
        self.grad.add_(torch.where(rej, self.grad_new, torch.zeros_like(self.grad_new)))
        self._slot_ctr += 1
        self._after_reset = False

    def step_reset(self, reset_mask, new_pose, new_idx, draws=None, z_threshold=None):
        """One iteration of fit.py:399-458 in which the rows of ``reset_mask`` are re-initialised (fit.py:408-422): after
        the proposal their pose / contact indices are replaced by ``new_pose`` / ``new_idx`` (what the reference's
        initialize_convex_hull writes, full batch size; see ``graspqp_amd.core.initializations``), MalaStar.reset_envs zeroes their step
        counter, gradient EMA and old gradient and makes the new pose the "old" one, and the accept step accepts them
        unconditionally.  ``reset_mask=None`` takes the reference's rule z_score > ``z_threshold`` (fit.py:409) from the
        z-scores the proposal kernel has just computed -- on the device, without a host round trip.  Launched eagerly with
        the stand-alone propose / accept kernels (this happens every few hundred iterations); the device-side draw-slot
        counter is advanced by hand so that graph replays stay in step.  A mask that selects no row (possible when
        batch_size_each is small: the largest z-score of b rows is (b-1)/sqrt(b)) makes this an ordinary iteration, as in
        the reference (fit.py:412); pinned by steps R_s4 / R_s5 of tests/golden/mala_ext_*.npz."""
        self.flush()
        self.draw(draws)
        st = _C.stream_ptr()
        self._propose(st)
        if reset_mask is None:
            m = self.z > float(z_threshold)  # NaN z (one-row objects) never resets, like the reference's comparison
        else:
            m = reset_mask.to(self.dev, torch.bool)
        self.reset_mask = m
        mc = m.unsqueeze(1)
        # fit.py:412 ``if reset_mask.sum() > 0``: with an EMPTY mask nothing is re-initialised and the iteration is an ordinary
        # one (the masked merges below are no-ops then; the evaluation must use the proposal's indices and the next
        # iteration must not see a leaf pose).  Kept on the device as a 0-dim flag: no host round trip.
        self._reinit = m.any()
        idx_all = torch.where(self._reinit, new_idx.to(self.dev), self.idx_new).contiguous()
        # masked merges with torch.where: boolean-mask indexing would synchronise with the host
        self.pose_new.copy_(torch.where(mc, new_pose.to(self.dev, torch.float32), self.pose_new))
        self.idx_new.copy_(torch.where(mc, idx_all, self.idx_new))
        mala = self.optimizer == "mala_star"
        if mala:  # MalaStar.reset_envs (optimizer.py:275-284); AnnealingDexGraspNet.reset_envs is a no-op (:148-149)
            self.step_count.masked_fill_(m, 0)
            self.ema.masked_fill_(mc, 0.0)
            self.hand_pose.copy_(torch.where(mc, self.pose_new, self.hand_pose))
            self.contact_idx.copy_(torch.where(mc, self.idx_new, self.contact_idx))
            self.grad.masked_fill_(mc, 0.0)
        # reference quirk (hand_model.py:815-831): set_parameters(..., env_mask) gathers the contact points of ALL rows with
        # the freshly drawn indices it is handed (initializations.py:190-193), while the rows outside the mask keep
        # their proposal's indices as state -- so this iteration's energies are evaluated at ``new_idx`` everywhere
        # (``idx_all`` is the proposal's ``idx_new`` when the mask is empty, see above)
        self._evaluate(self.pose_new, idx_all, st)
        # AnnealingDexGraspNet.accept_step ignores reset_mask
        self._accept(st, m.to(torch.uint8).contiguous() if mala else None)
        self._slot_ctr += 1
        self._after_reset = True

    def realign_draws(self):
        """Run queued iterations, then restart the 64-slot buffer of random draws at slot 0 (the next ``step`` refills
        it): afterwards a multi-iteration graph replays whole groups until the buffer wraps, so a timed region that
        starts here contains no eager remainder iterations (bench.py)."""
        self.flush()
        self._slot_ctr.zero_()
        self._draw_pos = 0

    # ---- on-device (re-)initialisation: initialize_convex_hull, scripts/fit.py:315,408-422 ------------------------------
    def set_hulls(self, hulls, init_args=None):
        """``hulls`` = ObjectModel.convex_hulls() (device triangles, area table, offsets); ``init_args`` = the ranges of
        scripts/fit.py:59-71 (Namespace / dict; reference defaults otherwise)."""
        self._hulls, self._init_args = hulls, init_args

    def fresh_state(self):
        """hand_pose (B,D) and contact indices (B,n) of initialize_convex_hull for ALL rows, drawn with the stepper's
        generator -- device tensors, nothing touches the host.  With ``init_avoid_scene`` the poses are screened against the
        scene (constructor docstring) and ``init_feasible`` is refreshed."""
        from .core.initializations import convex_hull_poses, convex_hull_poses_screened

        if getattr(self, "_hulls", None) is None:
            raise RuntimeError("GraspStepper.set_hulls(object_model.convex_hulls()) must be called first")
        if self.init_avoid_scene:
            approach = None
            if self.approach_mode:
                approach = dict(distance=self.approach_distance, stations=self.approach_stations, margin=self.approach_margin,
                                axis=self.hand.spec.grasp_axis, weight=self.w["E_approach"])
            pose, info = convex_hull_poses_screened(self.hand, self._hulls, self.n_obj, self.be, self.samples, self.scene,
                                                    self.scene_margin, self.w["E_scene"], approach, self._init_args, self.gen,
                                                    return_info=True)
            self.init_feasible.copy_(info["n_feasible"])
        else:
            pose = convex_hull_poses(self.hand.spec, self._hulls, self.n_obj, self.be, self._init_args, self.gen, self.dev)
        idx = torch.randint(self.hand.spec.n_contact_candidates, (self.B, self.n), device=self.dev, generator=self.gen)
        return pose, idx

    def initialize(self):
        """fit.py:315 + 381-396: initialize_convex_hull for every row, then the first energy evaluation."""
        pose, idx = self.fresh_state()
        self.reset(pose, idx)

    def run(self, n_iter, reset_epochs=600, z_score_threshold=1.0, callback=None):
        """The reference's schedule (fit.py:399-458): ``n_iter`` MALA* iterations; every ``reset_epochs`` iterations
        (while step < n_iter - 2 * reset_epochs) the rows whose per-object z-score exceeds ``z_score_threshold`` are
        re-initialised on the convex hull.  Ordinary iterations replay from the captured hipGraph, reset iterations are
        launched eagerly; the host never waits for the device.  ``callback(step)`` (e.g. export_poses every 500
        iterations, fit.py:518-521) is called after the iteration ``step``."""
        for step in range(1, n_iter + 1):
            if reset_epochs is not None and step % reset_epochs == 0 and step < n_iter - 2 * reset_epochs:
                pose, idx = self.fresh_state()
                self.step_reset(None, pose, idx, z_threshold=z_score_threshold)
            else:
                self.step()
            if callback is not None:
                self.flush()
                callback(step)
        self.flush()

    def select(self, k, radius=0.01, gates=None, score=None):
        """The ``k`` best grasps of every object that are feasible and different grasps -> ``ops.GraspSelection`` (device tensors;
        the host does not wait).  The state read is the ACCEPTED one: ``hand_pose`` / ``contact_idx``, ``terms`` and ``energy`` are
        what gq_mala_accept (or the accept tail of the FK backward launch) merged, and ``run`` ends with ``flush``.  One FK forward
        launch gives Rg / link_T of ``hand_pose`` into buffers of the selection's own, then ``ops.grasp_select``.
        ``gates`` = {term name: tol}: a row is feasible iff its (unweighted) term is <= tol for every gated term; None gates the
        obstacle terms that are on at 0.0 (``select_tolerances``).  ``score`` (B), lower is better: None takes ``energy``.
        ``radius`` (metres): picks of one object are at least this far apart in ``ops.grasp_distances``; 0 keeps duplicates.
        The hand surface is the stepper's ``samples`` (built with ``n_surface_points`` if no mode needed them so far).  Nothing of
        the chain's state is written: stepping on afterwards gives the bits of a stepper that never selected."""
        tol = select_tolerances(self.term_names, gates)
        self.flush()
        if self.samples is None:
            from .utils import meshes as mesh_utils

            pts, link = mesh_utils.hand_surface_samples(self.hand.spec, self._n_surface_points)
            self.samples = ops.SurfaceSamples(self.hand, pts, link, device=self.dev)
        if self._select_fk is None:
            self._select_fk = (torch.zeros(self.B, 9, device=self.dev), torch.zeros(self.B, self.L, 12, device=self.dev))
        Rg, LT = self._select_fk
        score = self.energy if score is None else score
        if tuple(score.shape) != (self.B,) or not score.is_floating_point():
            raise ValueError(f"GraspStepper.select: score must be a float tensor of shape ({self.B},), got {tuple(score.shape)}")
        # contact points / normals go to the proposal's scratch, which every evaluation rewrites before it reads it
        _C.call("gq_fk_forward", self.hand.handle, _C.f32(self.hand_pose), _C.i64(self.contact_idx), self.B, self.n, _C.f32(Rg),
                _C.f32(LT), _C.f32(self.cpts), _C.f32(self.cnrm), None, float(self.w["E_spen"]), None, None, None, None,
                _C.ptr(self.fk_ws), self.fk_nb, _C.stream_ptr())
        return ops.grasp_select(self.hand_pose, Rg, LT, self.samples, self.be, score.to(self.dev, torch.float32), self.terms, tol,
                                k, radius)

    def _surface_samples(self):
        if self.samples is None:
            from .utils import meshes as mesh_utils

            pts, link = mesh_utils.hand_surface_samples(self.hand.spec, self._n_surface_points)
            self.samples = ops.SurfaceSamples(self.hand, pts, link, device=self.dev)
        return self.samples

    def close(self, grid, direction=None, steps=32, step=None, touch=5e-4):
        """Close the fingers of the ACCEPTED grasps until they touch -> ``ops.CloseResult`` (device tensors; the host does not wait):
        the closed joints, which links touch, at which step, where and with which object normal (``ops.close_fingers``).  It is the
        step between ``select`` and ``hold``: close, then ask the payload question on the contacts that exist
        (``hold(..., closed=c)``).  ``grid`` is an ``ops.SceneSDF``, or an ``ops.SceneSDFSet`` with one grid per object, that
        CONTAINS THE TARGET (as ``pregrasp_scene``).  ``direction`` (B,JA) = None is the squeeze command of the accepted state: the
        joint velocities the E_squeeze launch computes at ``squeeze_min_travel`` / ``squeeze_damping`` (whether or not the term is
        on), NEGATED -- ``squeeze_theta`` follows the object's outward normals, the opening sense, and the closing sense moves the
        contacts INTO the object: one closing step along the default direction lowers the smallest phi of the fingertip links
        (tests/test_gpu_close.py::test_default_direction_closes).  Like ``select`` and ``hold`` it reads ``hand_pose`` /
        ``contact_idx`` after ``flush``, with one FK forward (and for the default direction one object query and one squeeze
        launch) into buffers of its own.  Nothing of the chain's state is written: stepping on afterwards gives the bits of a
        stepper that never called it."""
        grid = self._scene_arg("close", "grid", grid)
        st_np = ops._close_step(self.hand, step)
        samples = self._surface_samples()
        ops.close_check(grid, self.B, self.hand, samples.Ns, steps, st_np, touch)
        if direction is not None and tuple(direction.shape) != (self.B, self.J):
            raise ValueError(f"GraspStepper.close: direction must be ({self.B}, {self.J}), got {tuple(direction.shape)}")
        self.flush()
        with torch.no_grad():
            Rg, LT, cp, _, _, ws = ops.fk_contacts(self.hand_pose, self.contact_idx, self.hand)
            if direction is None:
                query = ops.sdf_cloud if self.cloud else ops.sdf_meshset
                d2, sgn, nrm, _ = query(cp.reshape(-1, 3), self.objs, self.be * self.n)
                _, onrm = ops.signed_distance(d2, sgn, nrm)
                theta = torch.empty(self.B, self.J, device=self.dev)
                ops._squeeze_call(self.hand, self.contact_idx, Rg.contiguous(), LT.contiguous(), ws, d2.reshape(self.B, self.n).contiguous(),
                                  onrm.reshape(self.B, self.n, 3).contiguous(), None, None, self._close_par[0], self._close_par[1], None,
                                  0.0, None, theta, 0, None, None, None, None)
                direction = -theta
            direction = direction.detach().to(self.dev, torch.float32).contiguous()
            out = ops._close_outputs(self.hand_pose, self.L)
            ops._close_call(self.hand, ops._pregrasp_grids(grid.values, grid.origin, grid.voxel), samples.points, samples.link,
                            self.hand_pose, Rg.contiguous(), direction, int(steps), torch.from_numpy(st_np).to(self.dev), float(touch),
                            ops.close_stop_masks(self.hand), *out)
            return ops.CloseResult(*out, out[1] >= 0)

    def hold(self, loads, max_force, torque_limits=None, iterations=16, closed=None, contacts=None):
        """Can the ACCEPTED grasps carry ``loads``?  -> ``ops.HoldResult`` (device tensors; the host does not wait): E_hold, the
        residual share per load, the cone-edge coefficients, the contact forces (N, world frame) and the joint torques they ask
        of the hand, with ``torque_limits`` (JA) also the effort.  ``loads`` (L,6) or (n_obj,L,6) from ``ops.hold_loads``,
        ``max_force`` the bound on every cone-edge coefficient in newtons; friction, cone edges and torque weight are the
        stepper's force-closure parameters.  Like ``select`` it reads ``hand_pose`` / ``contact_idx`` after ``flush``: one FK forward
        and one object query into buffers of its own, then the hold launch.  Nothing of the chain's state is written: stepping on
        afterwards gives the bits of a stepper that never called it.  To keep only grasps that hold the load:

            h = st.hold(ops.hold_loads(0.5), max_force=20.0)
            sel = st.select(k, score=torch.where(h.resid.amax(1) <= 0.05, st.energy, torch.inf))

        (``ops.grasp_select`` treats a non-finite score as infeasible).

        ``closed`` = the ``ops.CloseResult`` of ``close``: the question is asked on the contacts that exist after closing, the
        touched links' points and object normals (``closed.contacts(contacts)``, ``contacts`` = None: as many slots as the stepper
        has contacts), through ``ops.hold_contacts`` -> (E_hold, resid, force).  There are no joint torques on this route: the torque
        of a force at an arbitrary link point needs a Jacobian of that point, which the package does not have."""
        if closed is not None:
            if torque_limits is not None:
                raise ValueError("GraspStepper.hold: closed= has no joint torques, so torque_limits cannot be used with it")
            cp, onrm = closed.contacts(self.n if contacts is None else int(contacts))
            return ops.hold_contacts(cp, onrm, self.cog, loads, self.be, self.fc["friction"], self.fc["torque_weight"],
                                     self.fc["n_cone_vecs"], max_force, ops.HOLD_DEFAULTS["ridge"], iterations)
        lw = ops.hold_check(self.hand, self.n, self.fc["n_cone_vecs"], loads, max_force, ops.HOLD_DEFAULTS["ridge"], iterations,
                            self.fc["friction"], self.fc["torque_weight"], torque_limits, self.B // self.be, "GraspStepper.hold")
        lim = None if torque_limits is None else torch.as_tensor(torque_limits, dtype=torch.float32).reshape(-1).to(self.dev)
        self.flush()
        with torch.no_grad():
            Rg, LT, cp, _, _, ws = ops.fk_contacts(self.hand_pose, self.contact_idx, self.hand)
            query = ops.sdf_cloud if self.cloud else ops.sdf_meshset
            d2, sgn, nrm, _ = query(cp.reshape(-1, 3), self.objs, self.be * self.n)
            _, onrm = ops.signed_distance(d2, sgn, nrm)
            return ops._hold_terms_checked(self.hand, self.contact_idx, Rg, LT, ws, onrm.reshape(self.B, self.n, 3), cp, self.cog,
                                           lw.to(self.dev), self.B if lw.shape[0] == 1 else self.be, self.fc["friction"],
                                           self.fc["torque_weight"], self.fc["n_cone_vecs"], max_force, ops.HOLD_DEFAULTS["ridge"],
                                           iterations, lim)

    def flush(self):
        """Run the iterations that ``step`` has queued for a multi-iteration graph but not yet replayed."""
        if self._graph_pending:
            st = _C.stream_ptr()
            for _ in range(self._graph_pending):
                self._iteration(st, fused=self._can_fuse)
            self._graph_pending = 0

    def capture(self, fork=None, fused=None, iters=1):
        """Capture one iteration into a hipGraph: FK forward (column means of the squared gradient, the proposal, the
        kinematics and the object SDF of the contacts in one launch), the two stage launches that hold the force-closure
        and the penetration branch side by side (``fused``), FK backward (with the energies and the accept step as its
        tail) -- four launches, no host involvement.  ``fork`` = every role its own launch, the two branches as parallel graph
        branches: per-role occupancy instead of one register budget for both roles.  Left at None the mode follows the
        batch: one grid below 384 rows (latency: 3.14 vs 2.61 M evals/s at 256 rows, 3.07 vs 3.00 at 320), graph branches
        from 384 rows on (throughput: 3.67 vs 3.52 M at 384, 4.5 vs 4.1 M at 512, 8.0 vs 6.5 M at 2048, 8.7 vs 6.9 M at
        4096; tools/ab_fork.sh).  ``iters``
        > 1 captures that many consecutive iterations in one graph (every kernel finds its random draws through the
        device-side slot counter), which removes the graph-launch gap between iterations; ``step`` then replays once
        per ``iters`` calls and ``flush`` runs a remainder.  The state is saved and restored around the warm-up +
        capture passes, so capturing does not advance the chain."""
        keep = (self.hand_pose, self.contact_idx, self.grad, self.energy, self.ema, self.step_count, self.terms,
                self._span_acc, self._slot_ctr)
        saved = [t.clone() for t in keep]
        rng = (self.gen.get_state(), self._draw_pos)
        if fused is None:
            fused = self.B < 384 if fork is None else not fork
        if fork is None:
            fork = not fused
        fused = fused and self._can_fuse
        fork = fork and not fused
        self.graph_mode = "one grid" if fused else "graph branches" if fork else "serial"
        if fork and self._side is None:
            self._side = torch.cuda.Stream()
        s = torch.cuda.Stream()
        self.draw()  # may refill the draw buffers on the current stream: order it before the side stream's warm-up
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            self._iteration(_C.stream_ptr(), fork=fork, fused=fused)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        iters = iters if self._fuse_loop else 1
        assert 64 % iters == 0, "iters must divide the 64-slot draw buffer"
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            if self._fuse_loop:
                for _ in range(iters):
                    self._iteration(_C.stream_ptr(), fork=fork, fused=fused)
            else:
                self._evaluate(self.pose_new, self.idx_new, _C.stream_ptr(), fork=fork, fused=fused)
        torch.cuda.synchronize()
        for t, v in zip(keep, saved):
            t.copy_(v)
        self.gen.set_state(rng[0])
        self._draw_pos = rng[1]
        self._graph, self._graph_iters, self._graph_pending = g, iters, 0
        return g
