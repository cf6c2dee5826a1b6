"""HandModel with the reference's attribute/method surface (core/hand_model.py) on top of the HIP kernels.

Only the hot-path part of the reference class is mirrored: ``set_parameters``, ``fk``,
``_set_contact_idxs``, ``cal_distance``, ``self_penetration`` and the state attributes the optimizer and
``calculate_energy`` touch.  Construction goes through a :class:`HandSpec` (flat arrays) instead of
pytorch_kinematics / trimesh objects.
"""

from __future__ import annotations

import math

import torch

from .. import ops
from ..hands import get_hand_spec


class HandModel:
    def __init__(self, spec, device="cuda", grasp_type=None, n_surface_points=512):
        if not str(device).startswith("cuda"):
            raise RuntimeError("graspqp_amd.HandModel runs on the GPU only (device='cuda'); there is no CPU path")
        self.spec = spec
        self.device = torch.device(device)
        self._hand = ops.HandHandle(spec)
        self.n_dofs = spec.n_dofs
        self.n_contact_candidates = spec.n_contact_candidates
        self._actuated_joints_names = list(spec.joint_names)
        self.joints_names = list(spec.joint_names)
        # reference hand_model.py:451: the grasp_type's link subset (a spec from get_hand_spec(..., grasp_type=...) carries
        # it), None for the default type
        self._contact_links = getattr(spec, "contact_links", None)
        self.grasp_type = getattr(spec, "grasp_type", grasp_type)
        self.joints_lower = torch.tensor(spec.joints_lower, device=self.device)
        self.joints_upper = torch.tensor(spec.joints_upper, device=self.device)
        self.default_state = torch.tensor(spec.default_state, device=self.device)
        self.forward_axis = torch.tensor(spec.forward_axis, device=self.device)
        self.up_axis = torch.tensor(spec.up_axis, device=self.device)
        self.grasp_axis = torch.tensor(spec.grasp_axis, device=self.device)
        self.global_index_to_link_index = torch.tensor(spec.cand_link, dtype=torch.long, device=self.device)
        self.hand_pose = None
        self.contact_point_indices = None
        self.global_translation = None
        self.global_rotation = None
        self.current_status = None  # (B,L,3,4) link transforms in the hand frame
        self.contact_points = None
        self.contact_normals = None
        self._sphere_centers = None
        self._fk_ws = None
        self._n_surface_points = int(n_surface_points)
        self._surface = None  # (handle whose "candidates" are the hand's surface samples, link-frame points, link ids)

    # reference hand_model.py:762-766 -- returns the (B,L,3,4) link transforms (the reference returns a dict of
    # Transform3d keyed by link name; ``link_matrix(name)`` gives the same 4x4 view).
    def fk(self, joint_angles):
        B = joint_angles.shape[0]
        hp = torch.zeros(B, 9 + self.n_dofs, device=self.device)
        hp[:, 3] = 1.0
        hp[:, 7] = 1.0
        hp[:, 9:] = joint_angles.detach()
        idx = torch.zeros(B, 0, dtype=torch.long, device=self.device)
        return ops.fk_contacts(hp, idx, self._hand)[1]

    def link_matrix(self, link_name):
        l = self.spec.link_names.index(link_name)
        T = self.current_status[:, l]
        bottom = torch.tensor([0.0, 0.0, 0.0, 1.0], device=self.device).expand(T.shape[0], 1, 4)
        return torch.cat([T, bottom], dim=1)

    # reference hand_model.py:833-873
    def set_parameters(self, hand_pose, contact_point_indices=None, env_mask=None, _known_finite=False):
        """``_known_finite`` (internal, MalaStar.try_step): the pose comes straight from the proposal kernel, which zeroes every
        row that contains a NaN (optimizer.py:242-244) -- the reference's ``isnan().any()`` check (hand_model.py:862-863) cannot
        fire on it, and evaluating it would put a host-device synchronisation into every iteration."""
        if env_mask is not None:
            with torch.no_grad():
                self.hand_pose = torch.where(env_mask.unsqueeze(-1), hand_pose, self.hand_pose)
            self.hand_pose.requires_grad = True
            self.hand_pose.retain_grad()
        else:
            self.hand_pose = hand_pose.clone()
        if self.hand_pose.requires_grad:
            self.hand_pose.retain_grad()
        if not _known_finite and self.hand_pose.isnan().any():
            raise ValueError("nan in hand_pose")
        self.global_translation = self.hand_pose[:, 0:3]
        self._set_contact_idxs(contact_point_indices, env_mask=env_mask)

    # reference hand_model.py:787-831 -- only the n selected candidates are transformed (the reference
    # transforms all C and gathers n)
    def _set_contact_idxs(self, contact_point_indices, env_mask=None):
        if contact_point_indices is None:
            contact_point_indices = self.contact_point_indices
        if isinstance(contact_point_indices, str) and contact_point_indices == "all":
            contact_point_indices = (
                torch.arange(self.n_contact_candidates, dtype=torch.long, device=self.device)
                .unsqueeze(0)
                .expand(self.hand_pose.shape[0], -1)
            )
        if env_mask is None or self.contact_point_indices is None:
            self.contact_point_indices = contact_point_indices.clone()
        else:
            self.contact_point_indices = torch.where(env_mask.unsqueeze(-1), contact_point_indices, self.contact_point_indices)
        # reference hand_model.py:815-831: the contact points are gathered with the indices PASSED IN, also for the rows
        # outside env_mask (whose stored indices stay what they were) -- kept, it decides the energies of a reset iteration
        self._fk_idx = contact_point_indices.contiguous()  # the indices the kinematic state below belongs to
        Rg, LT, cp, cn, sc, ws = ops.fk_contacts(self.hand_pose, self._fk_idx, self._hand)
        self._fk_ws = ws
        self.global_rotation = Rg
        self.current_status = LT
        self.contact_points = cp
        self.contact_normals = cn
        self._sphere_centers = sc

    # reference hand_model.py:875-987
    def cal_distance(self, x, penetration_only=False):
        """x: (B,N,3) object surface points, identical for the rows of one object (object_model.py:182-184), or the
        un-expanded (n_obj,N,3).  Returns (B,N) max-over-links signed distance, inside positive."""
        penetration_only = ops.pen_mode(penetration_only)
        B = self.hand_pose.shape[0]
        if x.shape[0] == B and B > 0:
            # recover the per-object tensor: rows of an object share their points
            be = getattr(self, "_batch_each_hint", None)
            if be is None:
                raise RuntimeError("call ObjectModel.attach(hand_model) or pass the (n_obj,N,3) surface tensor")
            surf = x.view(-1, be, x.shape[1], 3)[:, 0].contiguous()
        else:
            surf = x
            be = B // x.shape[0]
        # the kinematic state (Rg, link transforms, FK workspace) is the one written by the last set_parameters
        return ops.hand_pen(self.hand_pose, surf, be, self._hand, self.contact_point_indices,
                            self.global_rotation.detach(), self.current_status.detach(), self._fk_ws,
                            self._fk_ws.numel(), penetration_only)

    # reference hand_model.py:698-760 (scripts/fit.py:462-470, --log_entropy): diversity of the grasp set as the mean
    # entropy of 32-bin histograms.  Evaluated in fp64 on the device (not a hot path), returned in the pose dtype.
    @staticmethod
    def _hist_entropy(values, lo, hi, bins=32):
        p = values.histc(bins, lo, hi)
        p = p / p.sum()
        return -(p * torch.log(torch.where(p > 0, p, torch.ones_like(p)))).sum()

    def joint_entropy(self):
        """Mean over the joints of the entropy of the joint angles' histogram over [lower, upper] -> 0-dim tensor."""
        q = self.hand_pose[:, 9:].detach().double()
        lo, hi = self.joints_lower.double().tolist(), self.joints_upper.double().tolist()
        ent = sum(self._hist_entropy(q[:, j], lo[j], hi[j]) for j in range(q.shape[1])) / q.shape[1]
        return ent.to(self.hand_pose.dtype)

    def pose_entropy(self):
        """(translation entropy, rotation entropy), each the mean of three 32-bin histogram entropies -> two 0-dim tensors.
        Translation: each axis over [-0.1, 0.1].  Rotation: the rotation vector of the hand's 6-D rotation in spherical
        coordinates (|v| over [0, pi], polar angle over [0, pi], azimuth over [-pi, pi])."""
        hp = self.hand_pose.detach().double()
        t = hp[:, 0:3]
        trans = sum(self._hist_entropy(t[:, i], -0.1, 0.1) for i in range(3)) / 3
        # Gram-Schmidt of the two 3-vectors (columns x, y, x cross y), as roma.special_gramschmidt
        x = torch.nn.functional.normalize(hp[:, 3:6], dim=-1)
        y = hp[:, 6:9]
        y = torch.nn.functional.normalize(y - (x * y).sum(-1, keepdim=True) * x, dim=-1)
        R = torch.stack([x, y, torch.linalg.cross(x, y)], -1)
        v = _rotvec(R)
        r = v.norm(dim=-1)
        theta = torch.acos(v[:, 2] / r)
        phi = torch.sign(v[:, 1]) * torch.acos(v[:, 0] / v[:, :2].norm(dim=-1))
        sph = torch.stack([r, theta, phi], -1)
        limits = [(0.0, math.pi), (0.0, math.pi), (-math.pi, math.pi)]
        rot = sum(self._hist_entropy(sph[:, i], *limits[i]) for i in range(3)) / 3
        return trans.to(self.hand_pose.dtype), rot.to(self.hand_pose.dtype)

    # reference hand_model.py:989-1040
    def self_penetration(self):
        return ops.self_pen(self._sphere_centers, self._hand)

    # reference hand_model.py:1220-1267: all C candidates (and normals) in the world frame
    def get_contact_candidates(self, with_normals=False):
        B = self.hand_pose.shape[0]
        all_idx = torch.arange(self.n_contact_candidates, dtype=torch.long, device=self.device).unsqueeze(0).expand(B, -1)
        _, _, cp, cn, _, _ = ops.fk_contacts(self.hand_pose.detach(), all_idx.contiguous(), self._hand)
        return (cp, cn) if with_normals else cp

    # reference hand_model.py:604-629 + 1042-1071: n_surface_points samples of the hand surface (per link proportional to
    # its area, 100x oversampled + farthest-point sampling, seed 42) in the world frame.  The reference draws them with
    # pytorch3d (absent: the sample SET differs, PARITY UNPINNED); here they are produced once on the host and pushed
    # through the FK kernels as extra "contact candidates", which also gives the analytic backward.
    def _surface_handle(self):
        if self._surface is None:
            import numpy as np

            from ..utils import meshes as mesh_utils

            spec = self.spec
            pts, lnk = mesh_utils.hand_surface_samples(spec, self._n_surface_points)
            import copy

            s2 = copy.copy(spec)
            s2.cand_pos, s2.cand_nrm, s2.cand_link = pts, np.tile(np.array([[0, 0, 1.0]], dtype=np.float32), (len(pts), 1)), lnk
            self._surface = (ops.HandHandle(s2), pts, lnk)
        return self._surface

    def set_surface_points(self, points, link_ids):
        """Use the given link-frame samples (Ns,3) / link ids (Ns) instead of drawing them (tests, reproducible runs)."""
        import copy

        import numpy as np

        s2 = copy.copy(self.spec)
        pts = np.ascontiguousarray(points, dtype=np.float32)
        s2.cand_pos, s2.cand_link = pts, np.ascontiguousarray(link_ids, dtype=np.int32)
        s2.cand_nrm = np.tile(np.array([[0, 0, 1.0]], dtype=np.float32), (len(pts), 1))
        self._surface = (ops.HandHandle(s2), pts, s2.cand_link)

    def set_scene(self, scene, margin=0.0):
        """The surroundings as an ``ops.SceneSDF`` (None removes it): calculate_energy(..., energy_names=[..., "E_scene"]) is then
        the sum over the surface samples of relu(margin - phi); ``margin`` >= 0 is a clearance in metres.  With an
        ``ops.SceneSDFSet`` (one grid per object) the rows are object-major and the batch must be divisible by ``n_grids``: row b
        reads grid b // (B / n_grids)."""
        if scene is not None and not isinstance(scene, (ops.SceneSDF, ops.SceneSDFSet)):
            raise ValueError("HandModel.set_scene: scene must be an ops.SceneSDF, an ops.SceneSDFSet or None")
        if not float(margin) >= 0.0:
            raise ValueError(f"HandModel.set_scene: margin = {margin!r} must be >= 0")
        self.scene, self.scene_margin = scene, float(margin)

    def set_approach(self, distance, stations, margin=None):
        """The approach corridor of calculate_energy(..., energy_names=[..., "E_approach"]): the mean over the stations
        d_k = distance k / stations, k = 1..stations <= 32, of the scene hinge with the whole hand moved back by d_k along the
        spec's grasp_axis.  Needs ``set_scene`` first; ``margin`` = None follows the scene's margin, also one set by a later
        ``set_scene``."""
        if getattr(self, "scene", None) is None:
            raise ValueError("HandModel.set_approach: call set_scene(ops.SceneSDF(...)) first")
        margin = None if margin is None else float(margin)
        if margin is not None and not margin >= 0.0:
            raise ValueError(f"HandModel.set_approach: margin = {margin!r} must be >= 0")
        if not 0.0 < float(distance) < float("inf"):
            raise ValueError(f"HandModel.set_approach: distance = {distance!r} must be finite and > 0")
        if int(stations) != stations or not 1 <= int(stations) <= 32:
            raise ValueError(f"HandModel.set_approach: stations = {stations!r} must be an integer in 1..32")
        self.approach = (float(distance), int(stations), margin)

    def set_pregrasp(self, distance, stations, opening=0.5, open_joints=None, margin=None, scene=None):
        """The pre-grasp corridor of calculate_energy(..., energy_names=[..., "E_pregrasp"]): the mean over the stations
        d_k = distance k / stations, k = 0..stations <= 32, of the scene hinge with the joints opened to
        (1 - opening) theta + opening open_joints and the whole hand moved back by d_k along the spec's grasp_axis.
        ``open_joints`` (n_dofs) = None takes the default state clamped to the joint limits; ``margin`` = None follows the scene's
        margin; ``scene`` = None takes the grid of ``set_scene`` -- this term's grid usually contains the target, which the grid
        of E_scene must not, so it can be given on its own."""
        if scene is None and getattr(self, "scene", None) is None:
            raise ValueError("HandModel.set_pregrasp: pass scene=ops.SceneSDF(...) or call set_scene(...) first")
        if scene is not None and not isinstance(scene, (ops.SceneSDF, ops.SceneSDFSet)):
            raise ValueError("HandModel.set_pregrasp: scene must be an ops.SceneSDF, an ops.SceneSDFSet or None")
        margin = None if margin is None else float(margin)
        if margin is not None and not margin >= 0.0:
            raise ValueError(f"HandModel.set_pregrasp: margin = {margin!r} must be >= 0")
        if not 0.0 < float(distance) < float("inf"):
            raise ValueError(f"HandModel.set_pregrasp: distance = {distance!r} must be finite and > 0")
        if int(stations) != stations or not 0 <= int(stations) <= 32:
            raise ValueError(f"HandModel.set_pregrasp: stations = {stations!r} must be an integer in 0..32")
        if not 0.0 <= float(opening) <= 1.0:
            raise ValueError(f"HandModel.set_pregrasp: opening = {opening!r} must be in [0, 1]")
        if open_joints is None:
            q = ops.default_open_joints(self.spec, self.device)
        else:
            q = torch.as_tensor(open_joints, dtype=torch.float32).detach().to(self.device)
        if q.shape != (self.n_dofs,):
            raise ValueError(f"HandModel.set_pregrasp: open_joints must be ({self.n_dofs},), got {tuple(q.shape)}")
        self.pregrasp = (float(distance), int(stations), float(opening), q, margin, scene)

    def set_squeeze(self, min_travel=5e-3, damping=1e-3):
        """The two parameters of calculate_energy(..., energy_names=[..., "E_squeeze"]): every contact moves along the object
        normal by max(|distance|, min_travel), and the joint velocities come from the pseudo-inverse of the contact Jacobian damped
        by ``damping``.  Both finite and > 0; the defaults make the term the reference's E_manipulativity (core/energy.py:80-87)."""
        ops.squeeze_check(None, 1, min_travel, damping, "HandModel.set_squeeze")
        self.squeeze = (float(min_travel), float(damping))

    def close_fingers(self, grid, direction, steps=32, step=None, touch=5e-4):
        """Close the fingers of the current poses (``set_parameters``) along ``direction`` (B,n_dofs) until they touch ``grid``, an
        ``ops.SceneSDF`` or ``ops.SceneSDFSet`` that contains the target -> ``ops.CloseResult``: the class-surface form of
        ``ops.close_fingers`` on the hand's surface samples.  Values only."""
        if self.hand_pose is None:
            raise ValueError("HandModel.close_fingers: call set_parameters(hand_pose, ...) first")
        _, pts, lnk = self._surface_handle()
        samples = getattr(self, "_close_samples", None)
        if samples is None or samples[0] is not pts:
            samples = self._close_samples = (pts, ops.SurfaceSamples(self.spec, pts, lnk, device=self.device))
        return ops.close_fingers(self.hand_pose.detach(), self._hand, samples[1], self.global_rotation.detach(), grid,
                                 torch.as_tensor(direction, dtype=torch.float32).to(self.device), steps, step, touch)

    def set_hold(self, loads, max_force, torque_limits=None, iterations=16):
        """The load of calculate_energy(..., energy_names=[..., "E_hold"]): ``loads`` (L,6) for every object or (n_obj,L,6) per
        object, wrenches (N, N m) on the object about its centre (``ops.hold_loads``), ``max_force`` the bound on every cone-edge
        coefficient in newtons, ``iterations`` PDIPM iterations per load.  The term takes the contact query and the cone parameters
        (friction, n_cone_vecs, torque_weight) that E_fc takes there.  ``torque_limits`` (JA) is kept for ``ops.hold_terms(...,
        return_details=True)``: the energy itself does not depend on it."""
        lw = ops.hold_check(None, None, 4, loads, max_force, ops.HOLD_DEFAULTS["ridge"], iterations, torque_limits=torque_limits,
                            who="HandModel.set_hold")
        lim = None if torque_limits is None else torch.as_tensor(torque_limits, dtype=torch.float32).reshape(-1).to(self.device)
        if lim is not None and lim.numel() != self.n_dofs:
            raise ValueError(f"HandModel.set_hold: torque_limits must be ({self.n_dofs},), got {tuple(lim.shape)}")
        self.hold = (lw, lw.to(self.device), float(max_force), lim, int(iterations))

    def set_reach(self, arm, arm_base, distance=0.10, stations=0, iterations=24, damping=1e-4, rot_scale=0.1):
        """The arm of calculate_energy(..., energy_names=[..., "E_reach"]): ``arm`` an ``ops.ArmSpec`` or ``ops.ArmHandle``,
        ``arm_base`` (3,4) or (n_obj,3,4) the arm base in the frame of each object, and the parameters of ``ops.reach_terms``
        (stations in 0..3 beyond the grasp pose over ``distance`` metres, damped-least-squares updates, damping in m^2, metres per
        radian).  Checked here, without a launch."""
        ops.reach_check(arm, distance, stations, iterations, damping, rot_scale, self.grasp_axis, "HandModel.set_reach")
        if arm is None:
            raise ValueError("HandModel.set_reach: arm must be an ops.ArmSpec or an ops.ArmHandle")
        base = torch.as_tensor(arm_base)
        # (n,3,4) float32 on the device, converted once; n = 1 serves every object
        base = ops.reach_base(base, base.shape[0] if base.dim() == 3 else 1, "HandModel.set_reach").to(self.device)
        handle = arm if isinstance(arm, ops.ArmHandle) else ops.ArmHandle(arm, self.device)
        self.reach = (handle, base, float(distance), int(stations), int(iterations), float(damping), float(rot_scale))

    def set_track(self, waypoints=8, updates=3):
        """The approach tracking of calculate_energy(..., energy_names=[..., "E_track"]): the arm of ``set_reach`` (call it first, with
        stations >= 1) follows the straight approach line over ``waypoints`` + 1 waypoints (1..64) from the retreated station to the
        grasp pose with ``updates`` (1..16) updates per waypoint (``ops.track_terms``); the distance, the damping and the rotation
        scale are the reach term's.  Checked here, without a launch."""
        if getattr(self, "reach", None) is None:
            raise ValueError("HandModel.set_track: call set_reach(arm, arm_base, ...) first")
        arm, _, dist, stations, _, damping, rot_scale = self.reach
        if stations < 1:
            raise ValueError("HandModel.set_track: set_reach needs stations >= 1: the path starts at the retreated station")
        ops.track_check(arm, dist, waypoints, updates, damping, rot_scale, self.grasp_axis, stations, False, "HandModel.set_track")
        self.track = (int(waypoints), int(updates))

    def set_arm_scene(self, scene=None, margin=None, damping=1e-6):
        """The arm clearance of calculate_energy(..., energy_names=[..., "E_arm"]): the collision spheres of the arm of
        ``set_reach`` (call it first, with an arm that has spheres) on ``scene``, an ``ops.SceneSDF`` or ``ops.SceneSDFSet`` -- None takes
        the grid of ``set_scene``; ``margin`` = None follows the scene's margin; ``damping`` is the term's own lambda_a.  The stations
        and the rotation scale are the reach term's."""
        if getattr(self, "reach", None) is None:
            raise ValueError("HandModel.set_arm_scene: call set_reach(arm, arm_base, ...) first")
        if scene is None and getattr(self, "scene", None) is None:
            raise ValueError("HandModel.set_arm_scene: pass scene=ops.SceneSDF(...) or call set_scene(...) first")
        if scene is not None and not isinstance(scene, (ops.SceneSDF, ops.SceneSDFSet)):
            raise ValueError("HandModel.set_arm_scene: scene must be an ops.SceneSDF, an ops.SceneSDFSet or None")
        margin = None if margin is None else float(margin)
        arm, _, dist, stations, _, _, rot_scale = self.reach
        ops.arm_check(arm, None, 1, 0.0 if margin is None else margin, damping, rot_scale, dist, stations, self.grasp_axis,
                      "HandModel.set_arm_scene")
        self.arm_scene = (scene, margin, float(damping))

    def set_lift(self, height, retreat, stations, direction=(0.0, 0.0, 1.0), margin=None, object_margin=0.0, object_points=None):
        """The way out of calculate_energy(..., energy_names=[..., "E_lift"]): the mean over the stations k = 1..stations <= 32 of the
        scene hinge of the hand's surface samples (``margin``; None follows the scene's margin) and of the held object's points
        (``object_margin``, finite, may be negative), both carried by (k / stations) (height u - retreat R a): u = ``direction`` in the
        object's frame (normalised here), a the spec's grasp_axis, ``height`` and ``retreat`` >= 0 in metres and not both zero.
        ``object_points`` (n_obj,M,3) in the object's frame; None takes the object model's surface points.  Needs ``set_scene``
        first, with a grid that does not contain the target."""
        if getattr(self, "scene", None) is None:
            raise ValueError("HandModel.set_lift: call set_scene(ops.SceneSDF(...)) first")
        margin = None if margin is None else float(margin)
        if object_points is not None:
            object_points = torch.as_tensor(object_points, dtype=torch.float32).detach().to(self.device).contiguous()
            if object_points.dim() != 3 or object_points.shape[2] != 3:
                raise ValueError(f"HandModel.set_lift: object_points must be (n_obj, M, 3), got {tuple(object_points.shape)}")
        u = ops.lift_direction(direction)
        ops.lift_check(None, 1, 1, 1, 1, 1, 0 if object_points is None else object_points.shape[1], height, retreat, stations,
                       self.grasp_axis, u, 0.0 if margin is None else margin, object_margin, "HandModel.set_lift")
        self.lift = (float(height), float(retreat), int(stations), torch.tensor(u, dtype=torch.float32, device=self.device), margin,
                     float(object_margin), object_points)

    def get_surface_points(self, hand_pose=None):
        """(B, n_surface_points, 3) hand surface samples in the world frame, differentiable w.r.t. hand_pose; ``hand_pose`` =
        None takes the model's own (another pose, e.g. the opened one of E_pregrasp, is a second FK at that pose)."""
        h, pts, _ = self._surface_handle()
        hp = self.hand_pose if hand_pose is None else hand_pose
        B = hp.shape[0]
        idx = torch.arange(len(pts), dtype=torch.long, device=self.device).unsqueeze(0).expand(B, -1).contiguous()
        return ops.fk_contacts(hp, idx, h)[2]

    # reference hand_model.py:1073-1077
    def get_manipulability(self, moving_directions, contact_point_indices=None, coupled=True):
        _, residuals = self.get_req_joint_velocities(moving_directions, contact_point_indices, coupled=coupled)
        if not coupled:
            residuals = residuals.mean(-1)
        return residuals

    # reference hand_model.py:772-777 (HandModel.jacobian -> Chain.jacobian of the pytorch_kinematics fork): geometric
    # Jacobian [J_v; J_w] of every mesh link, hand base frame, at the link-frame origin
    def jacobian(self, joint_angles):
        B = joint_angles.shape[0]
        hp = torch.zeros(B, 9 + self.n_dofs, device=self.device)
        hp[:, 3] = 1.0
        hp[:, 7] = 1.0
        hp[:, 9:] = joint_angles.detach()
        idx = torch.zeros(B, 0, dtype=torch.long, device=self.device)
        _, LT, _, _, _, ws = ops.fk_contacts(hp, idx, self._hand)
        return ops.link_jacobian(self._hand, LT, ws)

    # reference hand_model.py:1155-1218
    def get_req_joint_velocities(self, moving_directions, contact_point_indices=None, coupled=True, return_ee_vel=False):
        """Joint velocities that move the contact points along ``moving_directions`` (B,n,3, world frame): theta =
        pinv(J) d with the linear contact Jacobian J_v + J_w x r and the damped pseudo-inverse (lambda = 1e-3).
        -> (theta, residuals[, ee_vel]); coupled=False solves every contact on its own ((B,n,J), (B,n,3))."""
        B = self.hand_pose.shape[0]
        if contact_point_indices is None:
            contact_point_indices = (torch.arange(self.n_contact_candidates, dtype=torch.long, device=self.device)
                                     .unsqueeze(0).expand(B, -1))
        idx = contact_point_indices.contiguous()
        n = idx.shape[1]
        if coupled and not return_ee_vel and torch.is_grad_enabled() and (
                self.hand_pose.requires_grad or moving_directions.requires_grad):
            # differentiable route (E_manipulativity, core/energy.py:80-87): gradient to the joint angles through the contact
            # Jacobian, to the root rotation through R' d, and to the directions themselves
            return ops.joint_velocity_residuals(self.hand_pose, moving_directions.to(torch.float32), self._hand, idx,
                                                self.global_rotation, self.current_status, self._fk_ws)
        # link transforms / joint frames of the CURRENT pose (written by the last set_parameters)
        jc = ops.contact_jacobian(self._hand, idx, self.current_status, self._fk_ws)  # (B,n,3,J)
        R = self.global_rotation.detach()
        d = moving_directions.detach().to(torch.float32)
        if coupled:
            theta, res, ee = ops.joint_velocities(jc.reshape(B, 3 * n, self.n_dofs), d.reshape(B, 3 * n), R)
            ee = ee.view(B, n, 3)
        else:
            theta, res, ee = ops.joint_velocities(jc.reshape(B * n, 3, self.n_dofs), d.reshape(B * n, 3),
                                                  R.unsqueeze(1).expand(-1, n, -1, -1).reshape(B * n, 3, 3))
            theta, res, ee = theta.view(B, n, self.n_dofs), res.view(B, n, 3), ee.view(B, n, 3)
        if return_ee_vel:
            return theta, res, ee
        return theta, res

    @property
    def actuated_joints_names(self):
        return self._actuated_joints_names

    @property
    def n_actutated_joints(self):  # (sic) reference hand_model.py:779-781
        return self.n_dofs


def _rotvec(R):
    """Rotation vectors of rotation matrices (B,3,3): through the unit quaternion, the largest of its four components
    taken from the diagonal (numerically safe at every angle), then angle = 2 atan2(|v|, w) with w >= 0."""
    tr = R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]
    d = torch.stack([R[:, 0, 0], R[:, 1, 1], R[:, 2, 2], tr], -1)
    k = d.argmax(-1)
    q = torch.empty(R.shape[0], 4, dtype=R.dtype, device=R.device)  # (x, y, z, w)
    for i in range(3):  # the largest component is x, y or z
        j, l = (i + 1) % 3, (i + 2) % 3
        m = k == i
        qi = torch.sqrt((1 + 2 * R[:, i, i] - tr).clamp_min(0)) / 2
        s = 4 * qi
        qq = torch.empty_like(q)
        qq[:, i] = qi
        qq[:, j] = (R[:, j, i] + R[:, i, j]) / s
        qq[:, l] = (R[:, l, i] + R[:, i, l]) / s
        qq[:, 3] = (R[:, l, j] - R[:, j, l]) / s
        q = torch.where(m.unsqueeze(-1), qq, q)
    m = k == 3
    w = torch.sqrt((1 + tr).clamp_min(0)) / 2
    s = 4 * w
    qq = torch.stack([(R[:, 2, 1] - R[:, 1, 2]) / s, (R[:, 0, 2] - R[:, 2, 0]) / s, (R[:, 1, 0] - R[:, 0, 1]) / s, w], -1)
    q = torch.where(m.unsqueeze(-1), qq, q)
    q = torch.where(q[:, 3:4] < 0, -q, q)
    vn = q[:, :3].norm(dim=-1, keepdim=True)
    ang = 2 * torch.atan2(vn, q[:, 3:4])
    scale = torch.where(vn > 1e-12, ang / vn.clamp_min(1e-300), torch.full_like(vn, 2.0))
    return q[:, :3] * scale


def get_hand_model(hand_name: str, device="cuda", asset_dir=None, grasp_type=None, **kwargs) -> HandModel:
    """reference hands/__init__.py:27-28 (``grasp_type`` as in scripts/fit.py:304)"""
    return HandModel(get_hand_spec(hand_name, asset_dir, grasp_type=grasp_type), device=device, grasp_type=grasp_type, **kwargs)
