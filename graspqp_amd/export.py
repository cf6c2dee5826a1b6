"""export_poses -- the reference's grasp snapshot (scripts/fit.py:224-300) on the HIP kernels.

Writes one ``<object><suffix>.dexgrasp.pt`` per object with exactly the keys the reference's consumer reads
(graspqp_isaaclab/src/graspqp_isaaclab/utils/data.py:105-140): ``values`` (B,), ``parameters`` {joint name -> (B,),
"root_pose" -> (B,7) = [t, q_wxyz]}, ``grasp_velocities`` / ``full_grasp_velocities`` / ``grasp_velocities_off``
{joint name -> (B,)}, ``contact_idx`` (B,n), ``grasp_type``, ``contact_links``.  All tensors on the CPU, float32 /
int64, like the reference's.

The three velocity sets are joint velocities that close the hand along the object normals at the contacts
(``HandModel.get_req_joint_velocities``: linear contact Jacobian + damped pseudo-inverse): at the selected contacts
scaled by 5 |d|, at ALL contact candidates, and at the selected contacts scaled by 5 (|d| + 0.005).
"""

from __future__ import annotations

import os

import torch

from . import ops


def get_result_path(data_root_path, object_code, hand_name, n_contact, energy_name, grasp_type=None):
    """fit.py:203-221"""
    path = os.path.join(data_root_path, object_code, "grasp_predictions", hand_name, f"{n_contact}_contacts", energy_name,
                        "default" if grasp_type in (None, "all") else grasp_type)
    os.makedirs(path, exist_ok=True)
    return path


def grasp_snapshot(hand_model, energy, object_model):
    """The tensors of fit.py:226-252 for the whole batch (device tensors): root_pose (B,7), joint positions (B,J) and the
    three (B,J) velocity sets.  The hand model's contact indices are left as they were."""
    old_idx = hand_model.contact_point_indices.clone()
    with torch.no_grad():
        distance, normal = object_model.cal_distance(hand_model.contact_points)
        d = 5 * (normal * distance.unsqueeze(-1).abs())
        delta, _, _ = hand_model.get_req_joint_velocities(-d, hand_model.contact_point_indices, return_ee_vel=True)
        hand_model._set_contact_idxs("all")
        distance_f, normal_f = object_model.cal_distance(hand_model.contact_points)
        d_f = 5 * (normal_f * distance_f.unsqueeze(-1).abs())
        delta_full, _ = hand_model.get_req_joint_velocities(-d_f, hand_model.contact_point_indices)
        hand_model._set_contact_idxs(old_idx)
        distance, normal = object_model.cal_distance(hand_model.contact_points)
        d_o = 5 * normal * (distance.unsqueeze(-1).abs() + 0.005)
        delta_off, _, _ = hand_model.get_req_joint_velocities(-d_o, hand_model.contact_point_indices, return_ee_vel=True)
        root = ops.root_pose_wxyz(hand_model.hand_pose)
    return {"root_pose": root, "joint_positions": hand_model.hand_pose.detach()[:, 9:], "grasp_velocities": delta,
            "full_grasp_velocities": delta_full, "grasp_velocities_off": delta_off,
            "values": energy.detach(), "contact_idx": hand_model.contact_point_indices.detach()}


def snapshot_dicts(hand_model, energy, object_model, n_objects, batch_size, grasp_type=None, arm_path=None, hold=None, closed=None,
                   selection=None):
    """One dict per object in the reference's on-disk layout (CPU tensors).  ``selection`` (an ``ops.GraspSelection``, e.g. of
    ``GraspStepper.select``): each object's dict holds only its selected rows, in pick order, and two more keys,
    ``selected_rows`` (int64, the rows' indices within the object) and ``n_feasible`` (int); an object with nothing selected
    gets zero-length tensors.  The consumer reads by key, so the extra keys are harmless.  ``arm_path`` (B,T+1,N), such as
    ``GraspStepper.track_q``: the arm's joint path along the approach, waypoint 0 the retreated pose and waypoint T the grasp,
    written under the key ``arm_path`` for the rows each object's dict holds (in pick order under a ``selection``).  ``hold`` (an
    ``ops.HoldResult`` of the same rows, e.g. of ``GraspStepper.hold``): the contact forces (rows,L,n,3; newtons, object frame) and
    the joint torques (rows,L,JA) that carry its loads, under the keys ``hold_force`` and ``hold_torque``.  ``closed`` (an
    ``ops.CloseResult`` of the same rows, e.g. of ``GraspStepper.close``): the joints after finger closing under the key
    ``joint_positions_closed`` (a dict by joint name, like ``parameters``) and the number of touching links per row under
    ``n_touched_links`` (int64).  Pass all four by keyword: ``selection`` stays the last parameter."""
    if closed is not None:
        closed_theta, n_touched = closed.theta.detach().cpu(), closed.touched.detach().cpu().sum(1)
        if closed_theta.dim() != 2 or closed_theta.shape[0] != n_objects * batch_size:
            raise ValueError(f"snapshot_dicts: closed must be an ops.CloseResult of {n_objects * batch_size} rows, got theta "
                             f"{tuple(closed_theta.shape)}")
    if hold is not None:
        hold_force, hold_torque = hold.force.detach().cpu(), hold.torque.detach().cpu()
        if hold_force.dim() != 4 or hold_force.shape[0] != n_objects * batch_size or hold_torque.shape[:2] != hold_force.shape[:2]:
            raise ValueError(f"snapshot_dicts: hold must be an ops.HoldResult of {n_objects * batch_size} rows, got force "
                             f"{tuple(hold_force.shape)} and torque {tuple(hold_torque.shape)}")
    if arm_path is not None:
        arm_path = torch.as_tensor(arm_path).detach().cpu()
        if arm_path.dim() != 3 or arm_path.shape[0] != n_objects * batch_size:
            raise ValueError(f"snapshot_dicts: arm_path must be ({n_objects * batch_size}, T+1, N), got {tuple(arm_path.shape)}")
    if selection is not None:
        sel, n_sel, n_feas = selection.sel.cpu().long(), selection.n_selected.cpu(), selection.n_feasible.cpu()
        if sel.shape[0] != n_objects:
            raise ValueError(f"snapshot_dicts: the selection has {sel.shape[0]} objects, the snapshot {n_objects}")
    snap = {k: v.cpu() for k, v in grasp_snapshot(hand_model, energy, object_model).items()}
    names = list(hand_model._actuated_joints_names)
    out = []
    for a in range(n_objects):
        rows = slice(a * batch_size, (a + 1) * batch_size) if selection is None else sel[a, :int(n_sel[a])]
        params = {names[i]: snap["joint_positions"][rows, i].clone() for i in range(len(names))}
        params["root_pose"] = snap["root_pose"][rows].clone()
        data = {"values": snap["values"][rows].clone(), "parameters": params}
        for key in ("grasp_velocities", "full_grasp_velocities", "grasp_velocities_off"):
            data[key] = {names[i]: snap[key][rows, i].clone() for i in range(len(names))}
        data["contact_idx"] = snap["contact_idx"][rows].clone()
        data["grasp_type"] = grasp_type
        data["contact_links"] = hand_model._contact_links
        if arm_path is not None:
            data["arm_path"] = arm_path[rows].clone()
        if hold is not None:
            data["hold_force"], data["hold_torque"] = hold_force[rows].clone(), hold_torque[rows].clone()
        if closed is not None:
            data["joint_positions_closed"] = {names[i]: closed_theta[rows, i].clone() for i in range(len(names))}
            data["n_touched_links"] = n_touched[rows].clone()
        if selection is not None:
            data["selected_rows"] = rows - a * batch_size
            data["n_feasible"] = int(n_feas[a])
        out.append(data)
    return out


def export_poses(hand_model, energy, object_model, object_code_list, batch_size, data_root_path, hand_name, n_contact,
                 energy_name, suffix="None", grasp_type=None, arm_path=None, hold=None, closed=None, selection=None):
    """fit.py:224-300 -> list of the files written.  ``selection``, ``arm_path``, ``hold`` and ``closed``: see ``snapshot_dicts``; None
    writes every row / no arm motion / no holding forces / no closed joints (the file is then what it always was)."""
    files = []
    dicts = snapshot_dicts(hand_model, energy, object_model, len(object_code_list), batch_size, grasp_type, arm_path=arm_path,
                           hold=hold, closed=closed, selection=selection)
    for code, data in zip(object_code_list, dicts):
        path = os.path.join(get_result_path(data_root_path, code, hand_name, n_contact, energy_name, grasp_type),
                            code + f"{suffix}.dexgrasp.pt")
        torch.save(data, path)
        files.append(path)
    return files
