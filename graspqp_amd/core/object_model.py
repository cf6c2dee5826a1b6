"""ObjectModel with the reference's surface (core/object_model.py) on top of the HIP SDF kernels.

Meshes come as triangle soups (the reference loads them with trimesh from a dataset directory,
object_model.py:97-136; here ``initialize_from_meshes`` takes arrays, ``initialize`` reads OBJ files).
"""

from __future__ import annotations

import os

import numpy as np
import torch

from .. import ops
from ..hands.spec import load_obj_triangles
from ..utils import meshes as mesh_utils


def _fps_points(points: torch.Tensor, k: int) -> torch.Tensor:
    """``k`` of the (N,3) device points by farthest-point sampling from point 0 (set-up time; the arg-max of every round stays
    on the device)."""
    dist = torch.full((points.shape[0],), float("inf"), device=points.device)
    sel = torch.zeros(k, dtype=torch.long, device=points.device)
    cur = torch.zeros((), dtype=torch.long, device=points.device)
    for i in range(k):
        sel[i] = cur
        dist = torch.minimum(dist, ((points - points[cur]) ** 2).sum(-1))
        cur = torch.argmax(dist)
    return points[sel]


class ObjectModel:
    def __init__(self, data_root_path=None, batch_size_each=1, scale=1.0, num_samples=2000, device="cuda"):
        if not str(device).startswith("cuda"):
            raise RuntimeError("graspqp_amd.ObjectModel runs on the GPU only (device='cuda')")
        self.device = torch.device(device)
        self.batch_size_each = batch_size_each
        self.data_root_path = data_root_path
        self.num_samples = num_samples
        self.scale = scale
        self.object_code_list = None
        self.object_scale_tensor = None
        self.object_mesh_list = None
        self.object_face_verts_list = None
        self.surface_points_tensor = None
        self.surface_points_each = None  # (n_obj, P, 3), un-expanded
        self._meshset = None
        self._cloudset = None  # ops.PointCloudSet of an object given as oriented point clouds (initialize_from_point_clouds)
        self.cloud_points_list = None
        self._cog = None
        self._hull = None  # (face_verts (sumF,3,3), area cdf (sumF), offsets (n_obj+1)) on the device, built on demand
        self.sdf_library = "HIP"

    @property
    def cog(self):  # object_model.py:64-68
        if self._cog is None:
            self._cog = self.surface_points_tensor.mean(dim=1)
        return self._cog

    def initialize(self, object_code_list, extension=".obj", **_):
        """object_model.py:70-184 for OBJ files under ``<root>/<code>/coacd/{remeshed,decomposed}.obj`` or ``<root>/<code>/*.obj``."""
        if not isinstance(object_code_list, list):
            object_code_list = [object_code_list]
        fvs = []
        for code in object_code_list:
            cand = [os.path.join(self.data_root_path, code, "coacd", "remeshed.obj"),
                    os.path.join(self.data_root_path, code, "coacd", "decomposed.obj")]
            cand += sorted(
                os.path.join(self.data_root_path, code, f)
                for f in (os.listdir(os.path.join(self.data_root_path, code)) if os.path.isdir(os.path.join(self.data_root_path, code)) else [])
                if f.endswith(extension)
            )
            path = next((p for p in cand if os.path.exists(p)), None)
            if path is None:
                raise ValueError(f"Object {code} not found under {self.data_root_path}")
            fv = load_obj_triangles(path) * self.scale
            if len(np.unique(fv.reshape(-1, 3), axis=0)) < 100:
                raise ValueError(f"Object {code} has too few vertices, please check the data.")  # object_model.py:118
            fvs.append(fv.astype(np.float32))
        self.initialize_from_meshes(fvs, object_code_list)

    def initialize_from_meshes(self, face_verts_list, object_code_list=None, surface_points_list=None, generator=None):
        """``surface_points_list`` None: the ``num_samples`` surface points of every object are drawn ON THE DEVICE the way
        the reference does (object_model.py:163-178: 100 x num_samples area-weighted samples, farthest-point sampling
        from sample 0; ``gq_surface_fps``), then Morton-ordered; a list injects them (tests, fixed workloads)."""
        self.object_code_list = object_code_list or [f"obj{i}" for i in range(len(face_verts_list))]
        self.object_mesh_list = [np.asarray(f, dtype=np.float32) for f in face_verts_list]
        self.object_face_verts_list = [torch.tensor(f, device=self.device) for f in self.object_mesh_list]
        self._meshset = ops.MeshSet(self.object_mesh_list)
        self._cloudset, self.cloud_points_list = None, None
        n_obj = len(face_verts_list)
        self.object_scale_tensor = torch.ones(n_obj, self.batch_size_each, device=self.device)  # scale_choice = [1.0]
        if self.num_samples != 0:
            if surface_points_list is None:
                sp = ops.morton_sort_points(ops.surface_fps(self.object_mesh_list, self.num_samples, 100, generator, device=self.device))
            else:
                sp = torch.tensor(np.stack(surface_points_list), dtype=torch.float32, device=self.device)
            self.surface_points_each = sp.contiguous()
            self.surface_points_tensor = sp.repeat_interleave(self.batch_size_each, dim=0)
        self._cog = None
        self._hull = None

    def initialize_from_point_clouds(self, points_list, normals_list, object_code_list=None, radius=None, surface_points_list=None):
        """Objects as oriented point clouds (points with unit outward normals; scans, open shells, unions of parts): the
        contact query of ``cal_distance`` becomes the surfel signed distance of ``ops.sdf_cloud`` with disc radius ``radius``
        (None: per cloud 2 x the median nearest-neighbour distance).  ``surface_points_list`` None: ``num_samples`` of the
        cloud's own points by farthest-point sampling from point 0, Morton-ordered.  There is no mesh: ``object_mesh_list``
        and ``object_face_verts_list`` are None, and ``convex_hulls`` takes the cloud's points."""
        pts = [np.ascontiguousarray(np.asarray(p.detach().cpu() if torch.is_tensor(p) else p, dtype=np.float32).reshape(-1, 3))
               for p in points_list]
        if self.num_samples != 0 and surface_points_list is None:
            for i, p in enumerate(pts):
                if len(p) < self.num_samples:
                    raise ValueError(f"initialize_from_point_clouds: cloud {i} has {len(p)} points, fewer than num_samples = "
                                     f"{self.num_samples}")
        self.object_code_list = object_code_list or [f"obj{i}" for i in range(len(pts))]
        self.object_mesh_list = None
        self.object_face_verts_list = None
        self._meshset = None
        self._cloudset = ops.PointCloudSet(pts, normals_list, radius, device=self.device)
        self.cloud_points_list = pts
        self.object_scale_tensor = torch.ones(len(pts), self.batch_size_each, device=self.device)
        if self.num_samples != 0:
            if surface_points_list is None:
                sp = torch.stack([_fps_points(torch.tensor(p, device=self.device), self.num_samples) for p in pts])
                sp = ops.morton_sort_points(sp)
            else:
                sp = torch.tensor(np.stack(surface_points_list), dtype=torch.float32, device=self.device)
            self.surface_points_each = sp.contiguous()
            self.surface_points_tensor = sp.repeat_interleave(self.batch_size_each, dim=0)
        self._cog = None
        self._hull = None

    def initialize_from_tsdf(self, tsdf, min_weight=1.0, bounds=None, radius=None, object_code_list=None):
        """Objects from depth images: one object per grid of ``tsdf`` (an ``ops.SceneTSDF`` fused from frames that hold the target
        alone, ``ops.keep_label``), each in its grid's frame.  ``tsdf.extract_clouds(min_weight, bounds)`` turns the volume's
        zero level set into surfels on the device (one synchronisation, to learn their number), ``initialize_from_point_clouds``
        takes them from there: a single-view volume gives an open shell, which is what the cloud route is for."""
        clouds = tsdf.extract_clouds(min_weight, bounds)
        for g, (p, _) in enumerate(clouds):
            if len(p) == 0 or len(p) < self.num_samples:
                raise ValueError(f"initialize_from_tsdf: grid {g} yields {len(p)} surfels, num_samples = {self.num_samples} "
                                 f"(min_weight = {min_weight}, bounds = {bounds!r})")
        self.initialize_from_point_clouds([p for p, _ in clouds], [n for _, n in clouds], object_code_list, radius)

    def convex_hulls(self):
        """Convex hull of every object (scaled like initializations.py:42-46) as device arrays for
        ``initialize_convex_hull``: triangles oriented outward, per-object cumulative area table, offsets."""
        if self._hull is None:
            fvs, cdfs, off = [], [], [0]
            for i, f in enumerate(self.object_mesh_list if self._cloudset is None else self.cloud_points_list):
                h = mesh_utils.convex_hull_faces(f.reshape(-1, 3) * float(self.object_scale_tensor[i].max().item()))
                fvs.append(h)
                cdfs.append(mesh_utils.area_cdf(h))
                off.append(off[-1] + len(h))
            self._hull = (torch.tensor(np.concatenate(fvs), dtype=torch.float32, device=self.device).contiguous(),
                          torch.tensor(np.concatenate(cdfs), dtype=torch.float32, device=self.device).contiguous(),
                          torch.tensor(off, dtype=torch.int32, device=self.device))
            self.hull_face_verts_list = fvs
        return self._hull

    def attach(self, hand_model):
        hand_model._batch_each_hint = self.batch_size_each

    # object_model.py:186-255
    def cal_distance(self, x, with_closest_points=False):
        _, n_points, _ = x.shape
        if self._cloudset is not None:
            d2, sgn, nrm, cls = ops.sdf_cloud(x.reshape(-1, 3), self._cloudset, self.batch_size_each * n_points)
        else:
            d2, sgn, nrm, cls = ops.sdf_meshset(x.reshape(-1, 3), self._meshset, self.batch_size_each * n_points)
        dis, normals = ops.signed_distance(d2, sgn, nrm)  # sqrt(d2 + 1e-8) * (-sgn), nrm * sgn
        distance = dis.reshape(-1, n_points)
        normals = normals.reshape(-1, n_points, 3)
        if with_closest_points:
            return distance, normals, cls.reshape(-1, n_points, 3)
        return distance, normals
