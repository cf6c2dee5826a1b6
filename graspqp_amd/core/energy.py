"""``calculate_energy`` with the reference's signature (core/energy.py:6-89), composed from the HIP-backed ops.

This is the autograd ("plugin surface") route: every term is a torch tensor whose backward runs the HIP
backward kernels, so a ``fit.py``-style loop (``new_energy.sum().backward()``) works unchanged.  The
``GraspStepper`` in ``graspqp_amd.stepper`` runs the same kernels without autograd for throughput.
"""

import os

import torch

from .. import ops


FUSED = os.environ.get("GRASPQP_FUSED_ENERGY", "1") != "0"  # False: always compose the terms from the separate ops


class _FusedTerms(torch.autograd.Function):
    """The five terms of scripts/fit.py's energy as ONE autograd node on ``hand_pose``: the forward bodies of the registered
    ops back to back (object SDF at the contacts, signed distance, E_dis, E_fc, E_joints, hand penetration, E_pen, E_spen),
    and one backward that feeds every term's derivative -- scaled by its upstream row gradient -- into a single analytic FK
    backward.  Same kernels and same numbers as the term-by-term composition below; a fit.py-shaped loop is host-bound and
    a dozen autograd nodes with Python backwards cost more host time than the kernels take."""

    @staticmethod
    def forward(ctx, hand_pose, hand_model, object_model, fc_cfg, with_normals):
        hm, om, hand = hand_model, object_model, hand_model._hand
        hp = ops._c(hand_pose.detach())
        cp, hn = ops._c(hm.contact_points.detach()), ops._c(hm.contact_normals.detach())
        Rg, LT = ops._c(hm.global_rotation.detach()), ops._c(hm.current_status.detach())
        B, n, _ = cp.shape
        body = lambda op: op._init_fn
        flat = cp.reshape(-1, 3)
        d2, sgn, nrm, cls = body(ops._sdf_meshset_op)(flat, om._meshset.hid, om.batch_size_each * n)
        dis, onrm, g_sd = body(ops._signed_distance_op)(d2, sgn, nrm)
        distance, contact_normal = dis.reshape(B, n), onrm.reshape(B, n, 3)
        e_dis, gd, gh = body(ops._energy_dis_op)(distance, contact_normal, hn, with_normals)
        c = dict(ops.FC_DEFAULTS)
        c.update(fc_cfg)
        cfg = (int(c["n_cone_vecs"]), float(c["friction"]), float(c["torque_weight"]), float(c["max_limit"]), float(c["svd_gain"]),
               float(c["values_gain"]), float(c["eps"]), int(c["max_iter"]))
        cog = ops._c(om.cog.detach())
        e_fc, xs, _nit, fc_ws = body(ops._fc_energy_op)(cp, contact_normal, cog, *cfg)
        e_j, g_pose = body(ops._energy_joints_op)(hp, hm.joints_lower, hm.joints_upper)
        surf = om.surface_points_each
        pen_dis, link, gvec = body(ops._hand_pen_op)(hp, surf, om.batch_size_each, hand.hid, Rg, LT, 1)
        e_pen = body(ops._energy_pen_op)(pen_dis)
        if hand.S > 0:
            e_spen, g_sc = body(ops._self_pen_op)(hm._sphere_centers.detach(), hand.hid)
        else:
            e_spen, g_sc = torch.zeros(B, device=cp.device), None
        ctx.save_for_backward(hp, cp, flat, cls, g_sd, gd, gh, contact_normal, cog, fc_ws, g_pose, pen_dis, link, gvec, Rg, LT,
                              hm._fk_ws, hm._fk_idx, surf, *([g_sc] if g_sc is not None else []))
        ctx.hand, ctx.cfg, ctx.be, ctx.with_normals = hand, cfg, om.batch_size_each, with_normals
        ctx.mark_non_differentiable(distance, contact_normal, xs)
        return e_dis, e_fc, e_j, e_pen, e_spen, distance, contact_normal, xs

    @staticmethod
    def backward(ctx, g_dis, g_fc, g_j, g_pen, g_spen, _g1, _g2, _g3):
        (hp, cp, flat, cls, g_sd, gd, gh, contact_normal, cog, fc_ws, g_pose, pen_dis, link, gvec, Rg, LT, fk_ws, idx, surf,
         *rest) = ctx.saved_tensors
        hand = ctx.hand
        body = lambda op: op._init_fn
        B, n, _ = cp.shape
        k, mu, tw, _ml, sg, vg, _eps, _mi = ctx.cfg
        # contacts: E_fc + E_dis (through the signed distance and the squared distance of the SDF)
        gcp = body(ops._fc_energy_bwd_op)(cp, contact_normal, cog, g_fc, fc_ws, k, mu, tw, sg, vg)
        g_d2 = (g_dis.unsqueeze(-1) * gd).reshape(-1) * g_sd
        gcp = gcp + body(ops._sdf_backward)(g_d2, flat, cls).reshape(B, n, 3)
        gcn = (g_dis.view(-1, 1, 1) * gh) if ctx.with_normals else None
        gsc = (rest[0] * g_spen.view(-1, 1, 1)) if rest else None
        # hand penetration: upstream on the penetrating surface points -> link wrenches
        g = torch.where(pen_dis > 0, g_pen.unsqueeze(-1), g_pen.new_zeros(()))
        wrench, gRt = body(ops._hand_pen_bwd_op)(hand.L, surf, ctx.be, hp, Rg, g, link, gvec)
        z = hp.new_empty(0)
        args = [gcp, gcn, gsc, wrench, gRt, None]
        ghp = body(ops._fk_bwd_op)(hand.hid, hp, idx, Rg, LT, fk_ws, *[z if a is None else a for a in args],
                                   [a is not None for a in args])
        return ghp + g_j.unsqueeze(-1) * g_pose, None, None, None, None


def _fusable(hand_model, object_model, energy_fnc, method, energy_names):
    from ..metrics.ops.registry import SpanMetricWrapper

    return (FUSED and not ops._ROUTE["dispatcher"] and not torch.compiler.is_compiling() and isinstance(energy_fnc, SpanMetricWrapper)
            and not energy_fnc.exact  # only the PDIPM overall metric has a fused form; the exact metrics are composed
            and "E_manipulativity" not in energy_names  # its directions carry a gradient to `distance`
            and method in ("gendexgrasp", "dexgraspnet") and getattr(object_model, "_meshset", None) is not None
            and object_model.surface_points_each is not None and getattr(hand_model, "_fk_ws", None) is not None)


def calculate_energy(hand_model, object_model, energy_fnc=None, energy_names=[], method="gendexgrasp", svd_gain=0.1):
    losses = {}
    if _fusable(hand_model, object_model, energy_fnc, method, energy_names):
        object_model.attach(hand_model)
        (losses["E_dis"], losses["E_fc"], losses["E_joints"], losses["E_pen"], losses["E_spen"], distance, contact_normal,
         _lambda) = _FusedTerms.apply(hand_model.hand_pose, hand_model, object_model, energy_fnc.fc_config(svd_gain=svd_gain),
                                      method == "gendexgrasp")
        return _extra_terms(losses, hand_model, energy_names, distance, contact_normal, object_model, energy_fnc, svd_gain)
    distance, contact_normal = object_model.cal_distance(hand_model.contact_points)
    # (each term below is one launch that also writes its derivative, csrc/terms.hip: the torch expressions of the
    # reference, energy.py:25-28,47-52,58-61, cost a dozen launches each, forward and backward, in a host-bound loop)
    if method == "dexgraspnet":  # sum |d|
        losses["E_dis"] = ops.energy_dis(distance, contact_normal, hand_model.contact_normals, with_normals=False)
    elif method == "gendexgrasp":  # sum exp(1 - (-n_obj . n_hand)) |d|
        losses["E_dis"] = ops.energy_dis(distance, contact_normal, hand_model.contact_normals, with_normals=True)
    else:
        raise ValueError(f"Unknown method: {method}")

    E_fc, _lambda = energy_fnc(contact_pts=hand_model.contact_points, contact_normals=contact_normal, sdf=distance,
                               cog=object_model.cog, with_solution=True, svd_gain=svd_gain)
    losses["E_fc"] = E_fc

    losses["E_joints"] = ops.energy_joints(hand_model.hand_pose, hand_model.joints_lower, hand_model.joints_upper)

    object_model.attach(hand_model)
    distances = hand_model.cal_distance(object_model.surface_points_each, penetration_only=True)  # only dis > 0 is used
    losses["E_pen"] = ops.energy_pen(distances)  # sum of where(distances <= 0, 0, distances)
    losses["E_spen"] = hand_model.self_penetration()

    return _extra_terms(losses, hand_model, energy_names, distance, contact_normal, object_model, energy_fnc, svd_gain)


def _extra_terms(losses, hand_model, energy_names, distance, contact_normal, object_model=None, energy_fnc=None, svd_gain=0.1):
    if "E_prior" in energy_names:  # energy.py:68-74: the grasp axis should point down
        forward_axis = (hand_model.global_rotation @ hand_model.grasp_axis.view(1, -1, 1)).view(-1, 3)
        axis_prior = torch.tensor([0, 0, -1], dtype=torch.float, device=forward_axis.device).view(1, 3)
        losses["E_prior"] = 1 - torch.sum(forward_axis * axis_prior, dim=-1)

    if "E_wall" in energy_names:  # energy.py:76-78: hand surface samples below the table plane z = 0
        z_height = hand_model.get_surface_points()[..., -1].clamp(max=0.0)
        losses["E_wall"] = z_height.abs().sum(-1)

    if "E_scene" in energy_names:  # hand surface samples inside the obstacles of a signed-distance grid (HandModel.set_scene)
        scene = getattr(hand_model, "scene", None)
        if scene is None:
            raise ValueError('calculate_energy: "E_scene" needs HandModel.set_scene(ops.SceneSDF(...))')
        phi = ops.scene_distance(hand_model.get_surface_points(), scene)  # +inf outside the volume: free space
        losses["E_scene"] = torch.relu(hand_model.scene_margin - phi).sum(-1)

    if "E_approach" in energy_names:  # the same hinge along the approach corridor (HandModel.set_approach): the whole hand moved
        scene, corridor = getattr(hand_model, "scene", None), getattr(hand_model, "approach", None)  # back by d_k = D k / K
        if scene is None or corridor is None:
            raise ValueError('calculate_energy: "E_approach" needs HandModel.set_scene(...) and HandModel.set_approach(...)')
        D, K, margin = corridor
        margin = hand_model.scene_margin if margin is None else margin
        x = hand_model.get_surface_points()
        back = (hand_model.global_rotation @ hand_model.grasp_axis.view(1, -1, 1)).view(-1, 3)  # R a
        e = 0
        for k in range(1, K + 1):
            e = e + torch.relu(margin - ops.scene_distance(x - (D * k / K) * back.unsqueeze(1), scene)).sum(-1)
        losses["E_approach"] = e * (1.0 / K)

    if "E_pregrasp" in energy_names:  # the hinge of the OPENED hand along the corridor, d = 0 included (HandModel.set_pregrasp):
        pregrasp = getattr(hand_model, "pregrasp", None)  # the surface points of a second FK at the opened pose, then one
        if pregrasp is None:  # scene_distance per station
            raise ValueError('calculate_energy: "E_pregrasp" needs HandModel.set_pregrasp(...)')
        D, K, opening, q_open, margin, scene = pregrasp
        scene = getattr(hand_model, "scene", None) if scene is None else scene
        if scene is None:
            raise ValueError('calculate_energy: "E_pregrasp" needs a scene: HandModel.set_pregrasp(..., scene=) or set_scene(...)')
        margin = getattr(hand_model, "scene_margin", 0.0) if margin is None else margin
        hp = hand_model.hand_pose
        opened = torch.cat([hp[:, :9], (1.0 - opening) * hp[:, 9:] + opening * q_open.unsqueeze(0)], dim=1)
        x = hand_model.get_surface_points(opened)
        back = (hand_model.global_rotation @ hand_model.grasp_axis.view(1, -1, 1)).view(-1, 3)  # R a: the root pose is shared
        e = 0
        for k in range(K + 1):
            xk = x if k == 0 else x - (D * k / K) * back.unsqueeze(1)
            e = e + torch.relu(margin - ops.scene_distance(xk, scene)).sum(-1)
        losses["E_pregrasp"] = e * (1.0 / (K + 1))

    if "E_squeeze" in energy_names:
        # contact closing feasibility as ONE launch (ops.squeeze_terms; parameters: HandModel.set_squeeze): at the defaults the value
        # and gradient of E_manipulativity below, whose composed route stays as it is.  The op takes the squared distance and the
        # closest points of the contact query, so the query runs once more here, detached.
        tau, lam = getattr(hand_model, "squeeze", (5e-3, 1e-3))
        cp = hand_model.contact_points
        B, n, _ = cp.shape
        flat = cp.detach().reshape(-1, 3)
        if getattr(object_model, "_cloudset", None) is not None:
            d2, sgn, nrm, cls = ops.sdf_cloud(flat, object_model._cloudset, object_model.batch_size_each * n)
        else:
            d2, sgn, nrm, cls = ops.sdf_meshset(flat, object_model._meshset, object_model.batch_size_each * n)
        _, onrm = ops.signed_distance(d2, sgn, nrm)
        losses["E_squeeze"] = ops.squeeze_terms(hand_model.hand_pose, hand_model._hand, hand_model._fk_idx, hand_model.global_rotation,
                                                hand_model.current_status, hand_model._fk_ws, d2.reshape(B, n), onrm.reshape(B, n, 3),
                                                cls.reshape(B, n, 3), cp, tau, lam)

    if "E_hold" in energy_names:
        # payload holding as ONE launch (ops.hold_terms; loads and force bound: HandModel.set_hold) on the contact query and the cone
        # parameters of E_fc above; the gradient reaches the pose through the contact points
        if getattr(hand_model, "hold", None) is None:
            raise ValueError('calculate_energy: "E_hold" needs HandModel.set_hold(loads, max_force, ...)')
        if not hasattr(energy_fnc, "fc_config"):
            raise ValueError('calculate_energy: "E_hold" takes the cone parameters of the friction-cone span metric (GRASPQP)')
        cfg = energy_fnc.fc_config(svd_gain=svd_gain)
        lw, lw_dev, max_force, _lim, iters = hand_model.hold
        cp = hand_model.contact_points
        B, n, _ = cp.shape
        be = object_model.batch_size_each
        ops.hold_check(hand_model._hand, n, cfg["n_cone_vecs"], lw, max_force, ops.HOLD_DEFAULTS["ridge"], iters, cfg["friction"],
                       cfg["torque_weight"], n_obj=B // be, who="calculate_energy")
        losses["E_hold"] = ops._hold_terms_checked(
            hand_model._hand, hand_model._fk_idx, hand_model.global_rotation, hand_model.current_status, hand_model._fk_ws,
            contact_normal, cp, ops._hold_cog(object_model.cog, B, be, "calculate_energy"), lw_dev, B if lw.shape[0] == 1 else be,
            cfg["friction"], cfg["torque_weight"], cfg["n_cone_vecs"], max_force, ops.HOLD_DEFAULTS["ridge"], iters, None).e

    if "E_reach" in energy_names:
        # arm reachability as ONE launch (ops.reach_terms; arm and parameters: HandModel.set_reach)
        if getattr(hand_model, "reach", None) is None:
            raise ValueError('calculate_energy: "E_reach" needs HandModel.set_reach(arm, arm_base, ...)')
        arm, base, dist, stations, iters, damping, rot_scale = hand_model.reach
        B = hand_model.hand_pose.shape[0]
        be = object_model.batch_size_each
        if base.shape[0] not in (1, B // be):
            raise ValueError(f"calculate_energy: set_reach got {base.shape[0]} arm bases, the batch has {B // be} objects")
        base_T = base if base.shape[0] == B // be else base.expand(B // be, 3, 4).contiguous()
        # return_q: the arm configurations go on to E_arm below, which then needs no reach launch of its own
        losses["E_reach"], reach_q, _ = ops.reach_terms(hand_model.hand_pose, hand_model._hand, hand_model._fk_idx,
                                                        hand_model.global_rotation, hand_model.current_status, hand_model._fk_ws, arm, base_T,
                                                        be, hand_model.grasp_axis, dist, stations, iters, damping, rot_scale, return_q=True)

    if "E_track" in energy_names:
        # approach tracking as ONE launch after the reach launch (ops.track_terms; HandModel.set_reach + set_track), from the reach
        # term's retreated station; without "E_reach" the reach launch runs here, detached, for the start configuration alone
        if getattr(hand_model, "reach", None) is None or getattr(hand_model, "track", None) is None:
            raise ValueError('calculate_energy: "E_track" needs HandModel.set_reach(arm, arm_base, ...) and HandModel.set_track(...)')
        arm, base, dist, stations, iters, damping, rot_scale = hand_model.reach
        B = hand_model.hand_pose.shape[0]
        be = object_model.batch_size_each
        if base.shape[0] not in (1, B // be):
            raise ValueError(f"calculate_energy: set_reach got {base.shape[0]} arm bases, the batch has {B // be} objects")
        base_T = base if base.shape[0] == B // be else base.expand(B // be, 3, 4).contiguous()
        state = (hand_model._hand, hand_model._fk_idx, hand_model.global_rotation, hand_model.current_status, hand_model._fk_ws)
        if "E_reach" not in energy_names:
            with torch.no_grad():
                _, reach_q, _ = ops.reach_terms(hand_model.hand_pose, *state, arm, base_T, be, hand_model.grasp_axis, dist, stations, iters,
                                                damping, rot_scale, return_q=True)
        losses["E_track"] = ops.track_terms(hand_model.hand_pose, *state, arm, base_T, be, hand_model.grasp_axis, reach_q[:, stations],
                                            dist, hand_model.track[0], hand_model.track[1], damping, rot_scale)

    if "E_arm" in energy_names:
        # arm clearance as ONE launch after the reach launch (ops.arm_terms; HandModel.set_reach + set_arm_scene) on the arm
        # configurations of E_reach above; without that name the reach launch runs here, detached, for them alone -- the term's
        # gradient goes through its own formula
        if getattr(hand_model, "reach", None) is None or getattr(hand_model, "arm_scene", None) is None:
            raise ValueError('calculate_energy: "E_arm" needs HandModel.set_reach(arm, arm_base, ...) and HandModel.set_arm_scene(...)')
        arm, base, dist, stations, iters, damping, rot_scale = hand_model.reach
        scene, margin, lam_a = hand_model.arm_scene
        scene = getattr(hand_model, "scene", None) if scene is None else scene
        if scene is None:
            raise ValueError('calculate_energy: "E_arm" needs a scene: HandModel.set_arm_scene(scene=) or set_scene(...)')
        margin = getattr(hand_model, "scene_margin", 0.0) if margin is None else margin
        B = hand_model.hand_pose.shape[0]
        be = object_model.batch_size_each
        if base.shape[0] not in (1, B // be):
            raise ValueError(f"calculate_energy: set_reach got {base.shape[0]} arm bases, the batch has {B // be} objects")
        base_T = base if base.shape[0] == B // be else base.expand(B // be, 3, 4).contiguous()
        state = (hand_model._hand, hand_model._fk_idx, hand_model.global_rotation, hand_model.current_status, hand_model._fk_ws)
        if "E_reach" not in energy_names:
            with torch.no_grad():
                _, reach_q, _ = ops.reach_terms(hand_model.hand_pose, *state, arm, base_T, be, hand_model.grasp_axis, dist, stations, iters,
                                                damping, rot_scale, return_q=True)
        losses["E_arm"] = ops.arm_terms(hand_model.hand_pose, *state, arm, base_T, be, scene, hand_model.grasp_axis, reach_q, dist,
                                        stations, margin, lam_a, rot_scale)

    if "E_lift" in energy_names:  # the scene hinge of hand AND held object on the way out (HandModel.set_lift): both carried by
        scene, lift = getattr(hand_model, "scene", None), getattr(hand_model, "lift", None)  # (k / K) (H u - D R a), k = 1..K
        if scene is None or lift is None:
            raise ValueError('calculate_energy: "E_lift" needs HandModel.set_scene(...) and HandModel.set_lift(...)')
        H, D, K, u, margin, object_margin, pts = lift
        margin = hand_model.scene_margin if margin is None else margin
        x = hand_model.get_surface_points()
        B = x.shape[0]
        if pts is None:  # the object model's surface points, one row each already
            obj = object_model.surface_points_tensor
        else:
            if B % pts.shape[0]:
                raise ValueError(f"calculate_energy: set_lift got points of {pts.shape[0]} objects, the batch has {B} rows")
            obj = pts.repeat_interleave(B // pts.shape[0], dim=0)
        back = (hand_model.global_rotation @ hand_model.grasp_axis.view(1, -1, 1)).view(-1, 3)  # R a
        e = 0
        for k in range(1, K + 1):
            c = ((k / K) * (H * u.unsqueeze(0) - D * back)).unsqueeze(1)  # (B,1,3)
            e = e + torch.relu(margin - ops.scene_distance(x + c, scene)).sum(-1)
            e = e + torch.relu(object_margin - ops.scene_distance(obj + c, scene)).sum(-1)
        losses["E_lift"] = e * (1.0 / K)

    if "E_manipulativity" in energy_names:
        # energy.py:80-87: mean squared contact velocity the joints cannot produce when the contacts move along
        # normal * max(|distance|, 5 mm); differentiable (ops.joint_velocity_residuals: analytic kinematic Hessian)
        E_jacobian = hand_model.get_manipulability(
            contact_normal * distance.unsqueeze(-1).abs().clamp(min=5e-3), hand_model.contact_point_indices)
        losses["E_manipulativity"] = E_jacobian.mean(-1)
    return losses
