"""initialize_convex_hull with the reference's signature (core/initializations.py:15-193) on the HIP kernels.

Translation / rotation from the inflated convex hull of every object (surface samples -> farthest-point sampling ->
look-at rotation -> random stand-off distance, roll, pitch, tilt), joint angles from a truncated normal around the hand's
default state, random contact indices; handed to ``HandModel.set_parameters(..., env_mask=...)`` at the end, so a call
with ``env_mask`` re-initialises just those rows (scripts/fit.py:408-422).  Everything runs on the device: no trimesh /
pytorch3d / transforms3d, no host round trip (the hull itself is set-up data of the ObjectModel).

``convex_hull_poses_screened`` is the opt-in route that avoids the obstacles of a scene (include/graspqp_hip.h, "screened hull
candidates"): every hull sample a candidate pose, every candidate scored with the stepper's own obstacle launches, the rows picked
among the collision-free candidates.  ``initialize_convex_hull`` takes it when ``args.init_avoid_scene`` is truthy.
"""

from __future__ import annotations

import ctypes
import math

import torch

from .. import _C, ops

# scripts/fit.py:59-71
DEFAULT_INIT_ARGS = dict(jitter_strength=0.1, distance_lower=0.05, distance_upper=0.1, rotate_lower=-math.pi,
                         rotate_upper=math.pi, pitch_lower=-15 * math.pi / 180, pitch_upper=15 * math.pi / 180,
                         tilt_lower=-45 * math.pi / 180, tilt_upper=45 * math.pi / 180)


def _arg(args, name):
    if args is not None and hasattr(args, name):
        return float(getattr(args, name))
    if isinstance(args, dict) and name in args:
        return float(args[name])
    return float(DEFAULT_INIT_ARGS[name])


def convex_hull_poses(hand_spec, hulls, n_obj, batch_each, args=None, generator=None, device="cuda", draws=None,
                      samples_per_object=None, return_shell=False):
    """The pose part of initialize_convex_hull for all n_obj * batch_each rows -> hand_pose (B, 9 + J) on the device.
    ``hulls`` = ObjectModel.convex_hulls(); ``draws`` = dict(u_face, u_len, u_pose, u_joint) to inject the uniforms."""
    dev = torch.device(device)
    fv, cdf, off = hulls
    J = hand_spec.n_dofs
    B = n_obj * batch_each
    M = int(samples_per_object or 100 * batch_each)  # initializations.py:57
    if draws is None:
        r = lambda *s: torch.rand(*s, device=dev, generator=generator)
        draws = {"u_face": r(n_obj, M), "u_len": r(n_obj, M, 2), "u_pose": r(B, 4), "u_joint": r(B, J)}
    d = _draws_f32(draws, dev)
    nb = ops._size_call("gq_init_workspace_bytes", ctypes.c_int64(n_obj), ctypes.c_int64(M), ctypes.c_int64(batch_each))
    ws = ops._ws(nb, dev)
    pose = torch.empty(B, 9 + J, device=dev)
    shell_p = torch.empty(B, 3, device=dev) if return_shell else None
    shell_n = torch.empty(B, 3, device=dev) if return_shell else None
    de, _keep = _init_desc(hand_spec, hulls, n_obj, batch_each, M, args, d, pose, shell_p, shell_n, ws, nb, dev)
    _C.call("gq_init_convex_hull", ctypes.byref(de), _C.stream_ptr())
    return (pose, shell_p, shell_n) if return_shell else pose


def _draws_f32(draws, dev):
    return {k: v.to(dev, torch.float32).contiguous() for k, v in draws.items()}


def _init_desc(hand_spec, hulls, n_obj, batch_each, M, args, d, pose, shell_p, shell_n, ws, nb, dev):
    """gqInitDesc of gq_init_convex_hull / gq_init_candidates -> (descriptor, tensors it points at that the caller must keep)."""
    fv, cdf, off = hulls
    J = hand_spec.n_dofs
    consts = [torch.tensor(v, dtype=torch.float32, device=dev) for v in
              (hand_spec.default_state, hand_spec.joints_lower, hand_spec.joints_upper)]
    de = _C.InitDesc()
    de.hull_face_verts, de.hull_cdf, de.hull_offsets = fv.data_ptr(), cdf.data_ptr(), off.data_ptr()
    de.n_obj, de.batch_each, de.samples_per_object, de.n_dofs, de.inflate = n_obj, batch_each, M, J, 0.01
    for i in range(3):
        setattr(de, f"forward_axis{i}", float(hand_spec.forward_axis[i]))
        setattr(de, f"up_axis{i}", float(hand_spec.up_axis[i]))
    de.default_state, de.joints_lower, de.joints_upper = (c.data_ptr() for c in consts)
    for k in DEFAULT_INIT_ARGS:
        setattr(de, k, _arg(args, k))
    de.u_face, de.u_len, de.u_pose, de.u_joint = (d[k].data_ptr() for k in ("u_face", "u_len", "u_pose", "u_joint"))
    de.hand_pose = pose.data_ptr()
    de.shell_points = shell_p.data_ptr() if shell_p is not None else None
    de.shell_dirs = shell_n.data_ptr() if shell_n is not None else None
    de.workspace, de.workspace_bytes = ws.data_ptr(), nb
    return de, consts


def hull_candidates(hand_spec, hulls, n_obj, samples_per_object, args=None, device="cuda", draws=None):
    """gq_init_candidates: every hull sample a complete pose -> (cand_pose (n_obj M, 9 + J), points (n_obj M, 3), directions
    (n_obj M, 3)).  ``draws`` = dict(u_face (n_obj,M), u_len (n_obj,M,2), u_pose (n_obj M,4), u_joint (n_obj M,J)).  Candidate m's
    pose is what ``convex_hull_poses`` gives a row that picked sample m with the draws u_pose[m], u_joint[m], bit for bit."""
    dev = torch.device(device)
    M, N = int(samples_per_object), n_obj * int(samples_per_object)
    d = _draws_f32(draws, dev)
    nb = ops._size_call("gq_init_workspace_bytes", ctypes.c_int64(n_obj), ctypes.c_int64(M), ctypes.c_int64(M))
    ws = ops._ws(nb, dev)
    pose = torch.empty(N, 9 + hand_spec.n_dofs, device=dev)
    pts, dirs = torch.empty(N, 3, device=dev), torch.empty(N, 3, device=dev)
    de, _keep = _init_desc(hand_spec, hulls, n_obj, M, M, args, d, pose, pts, dirs, ws, nb, dev)
    _C.call("gq_init_candidates", ctypes.byref(de), _C.stream_ptr())
    return pose, pts, dirs


def init_select(points, penalty, K, tol=0.0):
    """gq_init_select: points (n_obj,M,3), penalty (n_obj,M) -> (sel (n_obj,K) int32, n_feasible (n_obj) int32): farthest-point
    sampling among {penalty <= tol}, the remaining slots by ascending (penalty, index) (include/graspqp_hip.h)."""
    points, penalty = ops._c(points), ops._c(penalty)
    n_obj, M = int(penalty.shape[0]), int(penalty.shape[1])
    dev = penalty.device
    sel = torch.empty(n_obj, max(int(K), 1), dtype=torch.int32, device=dev)
    nf = torch.empty(n_obj, dtype=torch.int32, device=dev)
    nb = ops._size_call("gq_init_select_workspace_bytes", ctypes.c_int64(n_obj), ctypes.c_int64(M))
    ws = ops._ws(nb, dev)
    try:  # the host-only check first: a refused argument is a ValueError with the library's wording
        _C.call("gq_init_select_check", _C.f32(points), _C.f32(penalty), ctypes.c_int64(n_obj), ctypes.c_int64(M),
                ctypes.c_int64(int(K)), float(tol), _C.i32(sel), _C.i32(nf), _C.ptr(ws))
    except RuntimeError as e:
        raise ValueError(str(e)) from None
    _C.call("gq_init_select", _C.f32(points), _C.f32(penalty), ctypes.c_int64(n_obj), ctypes.c_int64(M), ctypes.c_int64(int(K)),
            float(tol), _C.i32(sel), _C.i32(nf), _C.ptr(ws), nb, _C.stream_ptr())
    return sel, nf


def score_candidates(hand, cand_pose, n_obj, samples, scene, scene_margin, w_scene, approach=None, chunk_rows=65536):
    """The obstacle terms of the candidate rows (n_obj M, D), object-major, with the stepper's own launches: per object g and per
    chunk of at most ``chunk_rows`` rows gq_fk_forward (one dummy contact index), then gq_scene_terms and / or gq_approach_terms on
    grid g, without wrenches.  -> (e_scene (n_obj,M) or None, e_approach (n_obj,M) or None), unweighted.  The scratch is bounded
    by the chunk, not by n_obj M."""
    dev = cand_pose.device
    N, D = cand_pose.shape
    M = N // n_obj
    do_scene = float(w_scene) > 0
    do_app = approach is not None and float(approach.get("weight", 0.0)) > 0
    if not (do_scene or do_app):
        raise ValueError("scene-aware initialisation needs a weight > 0 on E_scene or E_approach")
    if not isinstance(scene, (ops.SceneSDF, ops.SceneSDFSet)):
        raise ValueError("scene-aware initialisation needs scene=ops.SceneSDF(...) or ops.SceneSDFSet(...)")
    if isinstance(scene, ops.SceneSDFSet) and scene.n_grids != n_obj:
        raise ValueError(f"scene-aware initialisation: scene has n_grids = {scene.n_grids}, there are n_obj = {n_obj} objects")
    chunk = max(1, min(int(chunk_rows), M))
    L = hand.L
    Rg, LT = torch.empty(chunk, 9, device=dev), torch.empty(chunk, L, 12, device=dev)
    cp, cn = torch.empty(chunk, 1, 3, device=dev), torch.empty(chunk, 1, 3, device=dev)
    idx = torch.zeros(chunk, 1, dtype=torch.long, device=dev)
    fk_ws, fk_nb = hand.fk_ws(chunk, dev)
    e_scene = torch.empty(n_obj, M, device=dev) if do_scene else None
    e_app = torch.empty(n_obj, M, device=dev) if do_app else None
    if do_app:
        axis = approach.get("axis")
        axis = hand.spec.grasp_axis if axis is None else axis
        a_margin = approach.get("margin")
        a_margin = scene_margin if a_margin is None else a_margin
    st = _C.stream_ptr()
    for g in range(n_obj):
        grid = scene.scene(g).grid if isinstance(scene, ops.SceneSDFSet) else scene.grid  # the same bits (graspqp_hip.h)
        for a in range(0, M, chunk):
            b = min(a + chunk, M)
            hp = cand_pose[g * M + a:g * M + b]
            _C.call("gq_fk_forward", hand.handle, _C.f32(hp), _C.i64(idx), b - a, 1, _C.f32(Rg), _C.f32(LT), _C.f32(cp), _C.f32(cn),
                    None, 0.0, None, None, None, None, _C.ptr(fk_ws), fk_nb, st)
            if do_scene:
                ops._scene_call(grid, scene_margin, hp, samples.points, samples.link, L, Rg, LT, None, float(w_scene),
                                e_scene[g, a:b], 0, None, None, st)
            if do_app:
                ops._approach_call(grid, a_margin, approach["distance"], approach["stations"], hp, samples.points, samples.link, L,
                                   Rg, LT, axis, None, float(approach["weight"]), e_app[g, a:b], 0, None, None, st)
    return e_scene, e_app


def convex_hull_poses_screened(hand, hulls, n_obj, batch_each, samples, scene, scene_margin, w_scene, approach=None, args=None,
                               generator=None, draws=None, samples_per_object=None, chunk_rows=65536, tol=0.0, return_info=False):
    """``convex_hull_poses`` that avoids the obstacles of ``scene``: every one of the M hull samples of an object becomes a candidate
    pose (``hull_candidates``), every candidate is scored with the obstacle terms the stepper evaluates (``score_candidates``:
    ``samples`` = ops.SurfaceSamples, ``scene`` = ops.SceneSDF or ops.SceneSDFSet, ``approach`` = None or dict(distance, stations,
    margin, axis, weight)), penalty = fmaf(w_approach, e_approach, w_scene e_scene), and ``batch_each`` candidates per object are
    picked by farthest-point sampling among those with penalty <= ``tol``; when an object has fewer, the remaining rows are its
    candidates of least penalty (``init_select``).  -> hand_pose (B, 9 + J); with ``return_info`` also a dict with sel, n_feasible,
    e_scene, e_approach, penalty, cand_pose, cand_points.  Everything stays on the device; the generator order is u_face
    (n_obj,M), u_len (n_obj,M,2), u_pose (n_obj M,4), u_joint (n_obj M,J)."""
    dev = samples.points.device
    spec = hand.spec
    J = spec.n_dofs
    M = int(samples_per_object or 100 * batch_each)
    N = n_obj * M
    if draws is None:
        r = lambda *s: torch.rand(*s, device=dev, generator=generator)
        draws = {"u_face": r(n_obj, M), "u_len": r(n_obj, M, 2), "u_pose": r(N, 4), "u_joint": r(N, J)}
    cand_pose, cand_p, _ = hull_candidates(spec, hulls, n_obj, M, args, dev, draws)
    e_scene, e_app = score_candidates(hand, cand_pose, n_obj, samples, scene, scene_margin, w_scene, approach, chunk_rows)
    penalty = torch.empty(n_obj, M, device=dev)
    _C.call("gq_init_penalty", _C.f32(e_scene), float(w_scene), _C.f32(e_app), float(approach["weight"]) if e_app is not None else 0.0,
            ctypes.c_int64(N), _C.f32(penalty), _C.stream_ptr())
    sel, nf = init_select(cand_p.view(n_obj, M, 3), penalty, batch_each, tol)
    D = 9 + J
    pose = torch.gather(cand_pose.view(n_obj, M, D), 1, sel.long().unsqueeze(-1).expand(-1, -1, D)).reshape(n_obj * batch_each, D)
    if not return_info:
        return pose
    return pose, dict(sel=sel, n_feasible=nf, e_scene=e_scene, e_approach=e_app, penalty=penalty, cand_pose=cand_pose,
                      cand_points=cand_p.view(n_obj, M, 3))


def initialize_convex_hull(hand_model, object_model, args=None, env_mask=None, energy_checker=None, init_contacts=True,
                           generator=None):
    """Reference signature (initializations.py:15).  ``args`` carries the ranges of scripts/fit.py:59-71 and ``n_contact``
    (a Namespace or dict; missing entries take the reference defaults)."""
    meshes = object_model.object_mesh_list  # None: the objects are point clouds
    n_obj = len(meshes if meshes is not None else object_model.object_code_list)
    be = object_model.batch_size_each
    avoid = getattr(args, "init_avoid_scene", None) if not isinstance(args, dict) else args.get("init_avoid_scene")
    if avoid:  # screened hull candidates against what HandModel.set_scene / set_approach hold
        scene = getattr(hand_model, "scene", None)
        if scene is None:
            raise ValueError("initialize_convex_hull: args.init_avoid_scene needs HandModel.set_scene(ops.SceneSDF(...))")
        _, pts, lnk = hand_model._surface_handle()
        samples = ops.SurfaceSamples(hand_model.spec, pts, lnk, device=hand_model.device)
        corridor = getattr(hand_model, "approach", None)
        approach = None
        if corridor is not None:
            approach = dict(distance=corridor[0], stations=corridor[1], margin=corridor[2], axis=None, weight=1.0)
        pose = convex_hull_poses_screened(hand_model._hand, object_model.convex_hulls(), n_obj, be, samples, scene,
                                          hand_model.scene_margin, 1.0, approach, args, generator)
    else:
        pose = convex_hull_poses(hand_model.spec, object_model.convex_hulls(), n_obj, be, args, generator, hand_model.device)
    if not init_contacts:  # initializations.py:183-184
        return pose[:, :3], pose[:, 3:9], pose[:, 9:]
    if hasattr(args, "n_contact"):
        n_contact = int(args.n_contact)
    elif isinstance(args, dict) and "n_contact" in args:
        n_contact = int(args["n_contact"])
    else:
        n_contact = 12  # scripts/fit.py:38
    idx = torch.randint(hand_model.n_contact_candidates, (n_obj * be, n_contact), device=hand_model.device, generator=generator)
    hand_model.set_parameters(pose.requires_grad_(), idx, env_mask=env_mask)
    return pose, idx
