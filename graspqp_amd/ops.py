"""Torch-facing wrappers of the HIP kernels (thin: allocate outputs, pass pointers, register autograd).

Every function here runs on the current HIP stream through the C ABI (``graspqp_amd._C``); none has a CPU path.
The ops are registered with the dispatcher as ``torch.ops.graspqp_amd.*`` (``torch.library.custom_op`` for the CUDA/HIP
device only, fake kernels for tracing, ``register_autograd`` for the backward -- itself a registered op), so they are
visible to ``torch.compile`` / the profiler like any ATen op.  Their differentiability contracts are exactly those of
the packages they replace: TorchSDF (only ``dist_sq`` w.r.t. ``points``), qpth (implicit KKT backward),
pytorch_kinematics (full FK).  Opaque device objects (mesh sets, hands) cross the dispatcher as integer ids.

Eager calls do not take the round trip through the dispatcher: a registered Python op costs ~40 us of host time per call
(schema matching, re-dispatch, the autograd wrapper of torch.library), a ``fit.py``-shaped loop on the class surface makes
about a dozen such calls per iteration, forward and backward, and is host-bound.  ``_Eager.<op>`` runs the SAME forward
body, ``setup_context`` and backward that are registered -- through a plain ``torch.autograd.Function`` where the op has a
gradient -- unless a trace / ``torch.compile`` is in progress or ``GRASPQP_DISPATCH=dispatcher`` / ``use_dispatcher(True)``
asks for the registered route (tests compare the two bit for bit).
"""

import ctypes
import os
import weakref
from typing import List, NamedTuple, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _C
from .arm import ArmSpec

_custom_op = torch.library.custom_op
_ROUTE = {"dispatcher": os.environ.get("GRASPQP_DISPATCH", "eager") == "dispatcher"}


def use_dispatcher(flag: bool) -> bool:
    """Route eager calls through the registered ``torch.ops.graspqp_amd.*`` (True) or past the dispatcher (False, the
    default; module docstring).  Returns the previous setting."""
    old, _ROUTE["dispatcher"] = _ROUTE["dispatcher"], bool(flag)
    return old


class _Eager:
    """Namespace of the eager routes, one per registered op (filled by ``_eager`` next to each registration)."""


def _eager(name, opdef, bwd=None, setup=None):
    body = opdef._init_fn  # the undecorated forward body
    if bwd is None:
        direct = body
    else:
        class _Fn(torch.autograd.Function):
            @staticmethod
            def forward(ctx, *args):
                out = body(*args)
                setup(ctx, args, out)
                return out

            @staticmethod
            def backward(ctx, *grads):
                return bwd(ctx, *grads)

        _Fn.__name__ = _Fn.__qualname__ = "graspqp_amd_" + name
        direct = _Fn.apply
    registered = getattr(torch.ops.graspqp_amd, name)

    def call(*args):
        if _ROUTE["dispatcher"] or torch.compiler.is_compiling():
            return registered(*args)
        return direct(*args)

    call.__name__ = name
    setattr(_Eager, name, staticmethod(call))
_HANDLES = weakref.WeakValueDictionary()  # id -> MeshSet / HandHandle (ops take the id: only tensors and scalars may
_next_id = [1]                            # cross the dispatcher)


def _register_handle(obj) -> int:
    i = _next_id[0]
    _next_id[0] += 1
    _HANDLES[i] = obj
    return i


def _handle(i: int):
    try:
        return _HANDLES[int(i)]
    except KeyError:
        raise RuntimeError(f"graspqp_amd: device object {i} no longer exists") from None

# ----------------------------------------------------------------------------------------------------------
# helpers
# ----------------------------------------------------------------------------------------------------------


def _ws(nbytes: int, device) -> torch.Tensor:
    return torch.empty(int(nbytes), dtype=torch.uint8, device=device)


def _size_call(name, *args) -> int:
    out = ctypes.c_size_t(0)
    _C.call(name, *args, ctypes.byref(out))
    return int(out.value)


def _c(t: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    if t.dtype != dtype:
        t = t.to(dtype)
    return t.contiguous()


# ----------------------------------------------------------------------------------------------------------
# mesh sets (device-resident triangle soups)
# ----------------------------------------------------------------------------------------------------------
class _DeviceObject:
    """An opaque object of the C ABI, created on ``device`` and destroyed once: by ``close()`` or with the wrapper."""

    def __init__(self, create, destroy, device, *args):
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self._destroy = destroy
        self.handle = None
        h = ctypes.c_void_p(0)
        with torch.cuda.device(self.device):
            _C.call(create, *args, ctypes.byref(h))
        self.handle = h

    def close(self):
        h, self.handle = getattr(self, "handle", None), None
        if h:
            getattr(_C.lib(), self._destroy)(h)
        hid = getattr(self, "hid", None)
        if hid is not None:
            _HANDLES.pop(hid, None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MeshSet(_DeviceObject):
    """n_mesh triangle soups on the device (face records precomputed once)."""

    def __init__(self, face_verts_list, device=None):
        fvs = [np.ascontiguousarray(np.asarray(f, dtype=np.float32).reshape(-1, 3, 3)) for f in face_verts_list]
        self.n_mesh = len(fvs)
        self.offsets = np.zeros(self.n_mesh + 1, dtype=np.int32)
        self.offsets[1:] = np.cumsum([len(f) for f in fvs])
        allf = np.ascontiguousarray(np.concatenate(fvs, 0))
        self.n_faces = int(self.offsets[-1])
        super().__init__("gq_meshset_create", "gq_meshset_destroy", device, allf.ctypes.data_as(ctypes.c_void_p),
                         self.offsets.ctypes.data_as(ctypes.c_void_p), self.n_mesh)
        self.hid = _register_handle(self)


class PointCloudSet(_DeviceObject):
    """n_obj oriented point clouds on the device (csrc/cloud.hip): points with outward normals and one disc radius per cloud,
    sorted into a uniform grid at set-up.  ``radius`` None: per cloud 2 x the median nearest-neighbour distance
    (``utils.meshes.cloud_radius``); a number, or one number per cloud, sets it (a cloud of one point needs it).  Normals are
    normalised in double by the library; zero / non-finite normals, non-finite points, empty clouds and radii <= 0 raise."""

    def __init__(self, points_list, normals_list, radius=None, device=None):
        pts = [np.ascontiguousarray(np.asarray(p.detach().cpu() if torch.is_tensor(p) else p, dtype=np.float32).reshape(-1, 3))
               for p in points_list]
        nrm = [np.ascontiguousarray(np.asarray(n.detach().cpu() if torch.is_tensor(n) else n, dtype=np.float32).reshape(-1, 3))
               for n in normals_list]
        if len(pts) != len(nrm) or any(len(p) != len(n) for p, n in zip(pts, nrm)):
            raise ValueError("PointCloudSet: every cloud needs as many normals as points")
        self.n_obj = len(pts)
        if radius is None:
            from .utils.meshes import cloud_radius

            radius = [cloud_radius(p) for p in pts]
        elif np.ndim(radius) == 0:
            radius = [float(radius)] * self.n_obj
        self.radius = np.ascontiguousarray(np.asarray(radius, dtype=np.float32).reshape(-1))
        if len(self.radius) != self.n_obj:
            raise ValueError(f"PointCloudSet: {len(self.radius)} radii for {self.n_obj} clouds")
        self.offsets = np.zeros(self.n_obj + 1, dtype=np.int32)
        self.offsets[1:] = np.cumsum([len(p) for p in pts])
        self.n_points = int(self.offsets[-1])
        allp = np.ascontiguousarray(np.concatenate(pts, 0)) if pts else np.zeros((0, 3), np.float32)
        alln = np.ascontiguousarray(np.concatenate(nrm, 0)) if nrm else np.zeros((0, 3), np.float32)
        as_p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        super().__init__("gq_cloudset_create", "gq_cloudset_destroy", device, as_p(allp), as_p(alln), as_p(self.offsets),
                         as_p(self.radius), self.n_obj)
        self.hid = _register_handle(self)


class Bvh(_DeviceObject):
    """Implicit 4-ary box hierarchy over one mesh (csrc/bvh.hip): the acceleration data of compute_sdf for large query
    counts."""

    def __init__(self, face_verts, device=None):
        fv = np.ascontiguousarray(np.asarray(face_verts, dtype=np.float32).reshape(-1, 3, 3))
        self.n_faces = int(fv.shape[0])
        super().__init__("gq_bvh_create", "gq_bvh_destroy", device, fv.ctypes.data_as(ctypes.c_void_p),
                         ctypes.c_int64(self.n_faces))
        self.hid = _register_handle(self)


def surface_fps(face_verts_list, n_keep: int, oversample: int = 100, generator=None, draws=None, device="cuda") -> torch.Tensor:
    """(n_obj, n_keep, 3) surface samples of every mesh, drawn on the device (reference core/object_model.py:163-178):
    ``oversample * n_keep`` area-weighted samples per mesh, farthest-point sampling from sample 0 down to ``n_keep``.
    ``draws`` = (u_face (n_obj,M), u_len (n_obj,M,2)) injects the uniforms (tests)."""
    dev = torch.device(device)
    fvs = [torch.as_tensor(f, dtype=torch.float32).reshape(-1, 3, 3).to(dev) for f in face_verts_list]
    n_obj, M = len(fvs), int(oversample) * int(n_keep)
    cdfs, off = [], [0]
    for f in fvs:
        area = 0.5 * torch.linalg.cross(f[:, 1] - f[:, 0], f[:, 2] - f[:, 0]).double().norm(dim=1)
        c = torch.cumsum(area, 0)
        cdfs.append((c / c[-1]).float())
        off.append(off[-1] + f.shape[0])
    fv, cdf = torch.cat(fvs).contiguous(), torch.cat(cdfs).contiguous()
    offs = torch.tensor(off, dtype=torch.int32, device=dev)
    if draws is None:
        draws = (torch.rand(n_obj, M, device=dev, generator=generator), torch.rand(n_obj, M, 2, device=dev, generator=generator))
    u_face, u_len = (_c(d.to(dev)) for d in draws)
    out = torch.empty(n_obj, int(n_keep), 3, device=dev)
    nb = _size_call("gq_init_workspace_bytes", ctypes.c_int64(n_obj), ctypes.c_int64(M), ctypes.c_int64(int(n_keep)))
    ws = _ws(nb, dev)
    _C.call("gq_surface_fps", _C.f32(fv), _C.f32(cdf), _C.i32(offs), ctypes.c_int64(n_obj), ctypes.c_int64(M),
            ctypes.c_int64(int(n_keep)), _C.f32(u_face), _C.f32(u_len), _C.f32(out), _C.ptr(ws), nb, _C.stream_ptr())
    return out


def morton_sort_points(points: torch.Tensor, bits: int = 10) -> torch.Tensor:
    """(n_obj,P,3) -> the same points, every object's set ordered along a 3-D Morton curve (neighbouring indices are
    spatial neighbours: the 64 points of a wavefront of the penetration query then meet the same hand links)."""
    lo, hi = points.amin(dim=1, keepdim=True), points.amax(dim=1, keepdim=True)
    q = ((points - lo) / (hi - lo).clamp_min(1e-12) * ((1 << bits) - 1)).to(torch.int64)
    code = torch.zeros(points.shape[:2], dtype=torch.int64, device=points.device)
    for b in range(bits):
        for a in range(3):
            code |= ((q[..., a] >> b) & 1) << (3 * b + a)
    order = torch.argsort(code, dim=1, stable=True)
    return torch.gather(points, 1, order.unsqueeze(-1).expand(-1, -1, 3)).contiguous()


class PointGrid(_DeviceObject):
    """Coarse uniform grid over the surface points of every object (n_obj,P,3): set-up data of the link-driven
    penetration query (gq_hand_pen_forward_cells)."""

    def __init__(self, surface_points, cells_per_axis: int = 0, device=None):
        if device is None and torch.is_tensor(surface_points) and surface_points.is_cuda:
            device = surface_points.device
        sp = np.ascontiguousarray(np.asarray(surface_points.detach().cpu() if torch.is_tensor(surface_points) else surface_points,
                                             dtype=np.float32))
        self.n_obj, self.P = int(sp.shape[0]), int(sp.shape[1])
        super().__init__("gq_pointgrid_create", "gq_pointgrid_destroy", device, sp.ctypes.data_as(ctypes.c_void_p),
                         ctypes.c_int64(self.n_obj), ctypes.c_int64(self.P), int(cells_per_axis))


# ----------------------------------------------------------------------------------------------------------
# TorchSDF-compatible ops
# ----------------------------------------------------------------------------------------------------------
def index_vertices_by_faces(verts: torch.Tensor, faces: torch.Tensor) -> torch.Tensor:
    """torchsdf.index_vertices_by_faces: verts (V,3), faces (F,3) int64 -> (F,3,3)."""
    return verts[faces.long()]


@_custom_op("graspqp_amd::sdf_backward", mutates_args=(), device_types="cuda")
def _sdf_backward(g_d2: Tensor, points: Tensor, closest: Tensor) -> Tensor:
    gp = torch.empty_like(points)
    if points.shape[0] > 0:
        _C.call("gq_sdf_backward", _C.f32(_c(g_d2)), _C.f32(points), _C.f32(closest), points.shape[0], _C.f32(gp),
                _C.stream_ptr())
    return gp


@_sdf_backward.register_fake
def _(g_d2, points, closest):
    return torch.empty_like(points)


def _sdf_outputs(pts):
    N, dev = pts.shape[0], pts.device
    return (torch.empty(N, device=dev), torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, 3, device=dev),
            torch.empty(N, 3, device=dev))


@_custom_op("graspqp_amd::compute_sdf", mutates_args=(), device_types="cuda")
def _compute_sdf_op(points: Tensor, face_verts: Tensor) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    pts, fv = _c(points), _c(face_verts)
    d2, sgn, nrm, cls = _sdf_outputs(pts)
    N, F = pts.shape[0], fv.shape[0]
    if N > 0:
        nb = _size_call("gq_sdf_workspace_bytes", ctypes.c_int64(F))
        ws = _ws(nb, pts.device)
        _C.call("gq_sdf_forward", _C.f32(pts), N, _C.f32(fv), F, _C.f32(d2), _C.i32(sgn), _C.f32(nrm), _C.f32(cls),
                _C.ptr(ws), nb, _C.stream_ptr())
    return d2, sgn, nrm, cls


@_compute_sdf_op.register_fake
def _(points, face_verts):
    return _sdf_outputs(points)


def _sdf_setup(ctx, inputs, output):
    ctx.save_for_backward(_c(inputs[0]), output[3])
    ctx.mark_non_differentiable(output[1], output[2], output[3])  # TorchSDF: only dist_sq is differentiable


def _sdf_bwd(ctx, g_d2, g_sgn, g_nrm, g_cls):
    pts, cls = ctx.saved_tensors
    return _Eager.sdf_backward(g_d2, pts, cls), None


torch.library.register_autograd("graspqp_amd::compute_sdf", _sdf_bwd, setup_context=_sdf_setup)


# Per-mesh set-up of the drop-in.  The reference hands the SAME face_verts tensor to every call (hand_model.py:351-353 keeps
# one per link, object_model.py:146-148 one per object), so the acceleration data of a mesh -- Morton-sorted face records
# + oriented 64-face cluster boxes (gq_meshset_create) -- is built on the first call with a tensor and kept while that
# tensor is alive and unmodified (weak reference + data pointer + version counter; a dead tensor drops its entry).
_MESH_CACHE = {}              # (id(face_verts), kind) -> (weakref, data_ptr, _version, MeshSet | Bvh)
_MESH_CACHE_MIN_FACES = 1024  # cluster search (one wavefront per query): meshes from this size on
_BVH_MIN_QUERIES = 32768      # box hierarchy (one query per lane): query counts from this size on
_BVH_MIN_FACES, _BVH_MAX_FACES = 32, 65536


def _cached(face_verts, kind):
    key = (id(face_verts), kind)
    ent = _MESH_CACHE.get(key)
    if ent is not None and ent[0]() is face_verts and ent[1] == face_verts.data_ptr() and ent[2] == face_verts._version:
        return ent[3]
    if torch.cuda.is_current_stream_capturing():  # the build copies to the host and synchronises
        raise RuntimeError("graspqp_amd: first call per mesh must happen outside graph capture")
    fv = face_verts.detach().to(torch.float32).cpu().numpy()  # one device->host copy, once per mesh and kind
    obj = MeshSet([fv], face_verts.device) if kind == "clusters" else Bvh(fv, face_verts.device)
    ref = weakref.ref(face_verts, lambda _r, k=key: _MESH_CACHE.pop(k, None))
    _MESH_CACHE[key] = (ref, face_verts.data_ptr(), face_verts._version, obj)
    return obj


def _cached_meshset(face_verts):
    return _cached(face_verts, "clusters")


def compute_sdf(points: torch.Tensor, face_verts: torch.Tensor):
    """torchsdf.compute_sdf drop-in -> (dist_sq, sign int32, normal, closest).

    Three device paths behind the one signature, all exact with the same winner rule (smallest ranking distance, ties to
    the smallest face index): (i) N >= 32768 queries: one query per lane through the mesh's box hierarchy (gq_sdf_forward_bvh;
    the per-link calls of HandModel.cal_distance); (ii) fewer queries against >= 1024 faces: best-first search over
    oriented 64-face cluster boxes, one wavefront per query (the contact queries of ObjectModel.cal_distance); (iii)
    otherwise the face loop of gq_sdf_forward (no set-up).  (i) and (ii) use acceleration data built on the first call
    with a ``face_verts`` tensor and kept while that tensor is alive and unmodified."""
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"compute_sdf: points must be (N,3), got {tuple(points.shape)}")
    if face_verts.dim() != 3 or tuple(face_verts.shape[1:]) != (3, 3):
        raise ValueError(f"compute_sdf: face_verts must be (F,3,3), got {tuple(face_verts.shape)}")
    if not points.is_cuda:
        raise RuntimeError("graspqp_amd ops need CUDA (ROCm) tensors; got a CPU tensor")
    if points.device.index != torch.cuda.current_device():  # launches go to the current device's stream
        with torch.cuda.device(points.device):
            return compute_sdf(points, face_verts)
    N, F = points.shape[0], face_verts.shape[0]
    if N > 0 and not face_verts.requires_grad:
        if N >= _BVH_MIN_QUERIES and _BVH_MIN_FACES <= F <= _BVH_MAX_FACES:
            return _Eager.sdf_bvh(points, _cached(face_verts, "bvh").hid)
        if F >= _MESH_CACHE_MIN_FACES:
            return _Eager.sdf_meshset(points, _cached_meshset(face_verts).hid, N)
    return _Eager.compute_sdf(points, face_verts)


@_custom_op("graspqp_amd::sdf_meshset", mutates_args=(), device_types="cuda")
def _sdf_meshset_op(points: Tensor, meshset: int, queries_per_mesh: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """compute_sdf of n_mesh groups of queries against a MeshSet (object_model.py:217-220 without the loop)."""
    pts = _c(points).reshape(-1, 3)
    d2, sgn, nrm, cls = _sdf_outputs(pts)
    _C.call("gq_sdf_forward_meshset", _handle(meshset).handle, _C.f32(pts), pts.shape[0], int(queries_per_mesh), _C.f32(d2),
            _C.i32(sgn), _C.f32(nrm), _C.f32(cls), _C.stream_ptr())
    return d2, sgn, nrm, cls


@_sdf_meshset_op.register_fake
def _(points, meshset, queries_per_mesh):
    return _sdf_outputs(points.reshape(-1, 3))


def _sdf_ms_setup(ctx, inputs, output):
    ctx.save_for_backward(_c(inputs[0]).reshape(-1, 3), output[3])
    ctx.in_shape = inputs[0].shape
    ctx.mark_non_differentiable(output[1], output[2], output[3])


def _sdf_ms_bwd(ctx, g_d2, g_sgn, g_nrm, g_cls):
    pts, cls = ctx.saved_tensors
    return _Eager.sdf_backward(g_d2, pts, cls).reshape(ctx.in_shape), None, None


torch.library.register_autograd("graspqp_amd::sdf_meshset", _sdf_ms_bwd, setup_context=_sdf_ms_setup)


@_custom_op("graspqp_amd::sdf_bvh", mutates_args=(), device_types="cuda")
def _sdf_bvh_op(points: Tensor, bvh: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """compute_sdf of many points against one mesh through its box hierarchy (one query per lane)."""
    pts = _c(points).reshape(-1, 3)
    d2, sgn, nrm, cls = _sdf_outputs(pts)
    _C.call("gq_sdf_forward_bvh", _handle(bvh).handle, _C.f32(pts), pts.shape[0], _C.f32(d2), _C.i32(sgn), _C.f32(nrm),
            _C.f32(cls), _C.stream_ptr())
    return d2, sgn, nrm, cls


@_sdf_bvh_op.register_fake
def _(points, bvh):
    return _sdf_outputs(points.reshape(-1, 3))


def _sdf_bvh_bwd(ctx, g_d2, g_sgn, g_nrm, g_cls):
    pts, cls = ctx.saved_tensors
    return _Eager.sdf_backward(g_d2, pts, cls).reshape(ctx.in_shape), None


torch.library.register_autograd("graspqp_amd::sdf_bvh", _sdf_bvh_bwd, setup_context=_sdf_ms_setup)


def sdf_meshset(points, meshset: MeshSet, queries_per_mesh: int):
    return _Eager.sdf_meshset(points, meshset.hid, int(queries_per_mesh))


@_custom_op("graspqp_amd::sdf_cloud", mutates_args=(), device_types="cuda")
def _sdf_cloud_op(points: Tensor, cloudset: int, queries_per_object: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """The contact query against a PointCloudSet (surfel signed distance, include/graspqp_hip.h): the outputs of sdf_meshset."""
    pts = _c(points).reshape(-1, 3)
    d2, sgn, nrm, cls = _sdf_outputs(pts)
    cs = _handle(cloudset)
    if cs.handle is None:
        raise RuntimeError(f"graspqp_amd: point cloud set {cloudset} has been closed")
    if pts.shape[0] > 0:
        _C.call("gq_cloud_forward", cs.handle, _C.f32(pts), pts.shape[0], int(queries_per_object), _C.f32(d2), _C.i32(sgn),
                _C.f32(nrm), _C.f32(cls), _C.stream_ptr())
    return d2, sgn, nrm, cls


@_sdf_cloud_op.register_fake
def _(points, cloudset, queries_per_object):
    return _sdf_outputs(points.reshape(-1, 3))


torch.library.register_autograd("graspqp_amd::sdf_cloud", _sdf_ms_bwd, setup_context=_sdf_ms_setup)


def sdf_cloud(points, cloudset: PointCloudSet, queries_per_object: int):
    """(dist_sq, sign int32, normal, closest) of the queries against the clouds of ``cloudset``: query q uses cloud
    q // queries_per_object.  Only dist_sq is differentiable, w.r.t. points (sdf_backward)."""
    if cloudset.handle is None:
        raise RuntimeError("graspqp_amd: this PointCloudSet has been closed")
    return _Eager.sdf_cloud(points, cloudset.hid, int(queries_per_object))


# ----------------------------------------------------------------------------------------------------------
# box QP (qpth.qp.QPFunction on G = [I; -I]) and the least-squares form used by SQPLsqSolver
# ----------------------------------------------------------------------------------------------------------
def _qp_ws(B, nz, max_iter, dev):
    nb = _size_call("gq_boxqp_workspace_bytes", ctypes.c_int64(B), int(nz), int(max_iter))
    return _ws(nb, dev), nb


@_custom_op("graspqp_amd::box_qp", mutates_args=(), device_types="cuda")
def _box_qp_op(Q: Tensor, p: Tensor, lower: Tensor, upper: Tensor, eps: float, max_iter: int,
               not_improved_lim: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    Qc, pc, lc, uc = _c(Q), _c(p), _c(lower), _c(upper)
    B, nz = pc.shape
    dev = Qc.device
    x = torch.empty(B, nz, device=dev)
    lam = torch.empty(B, 2 * nz, device=dev)
    slack = torch.empty(B, 2 * nz, device=dev)
    nit = torch.zeros(1, dtype=torch.int32, device=dev)
    ws, nb = _qp_ws(B, nz, max_iter, dev)
    _C.call("gq_boxqp_forward", _C.f32(Qc), _C.f32(pc), _C.f32(lc), _C.f32(uc), 0.0, 0.0, B, nz, float(eps),
            int(max_iter), int(not_improved_lim), _C.f32(x), _C.f32(lam), _C.f32(slack), None, _C.i32(nit),
            _C.ptr(ws), nb, _C.stream_ptr())
    return x, lam, slack, nit


@_box_qp_op.register_fake
def _(Q, p, lower, upper, eps, max_iter, not_improved_lim):
    B, nz = p.shape
    return (p.new_empty(B, nz), p.new_empty(B, 2 * nz), p.new_empty(B, 2 * nz), p.new_empty(1, dtype=torch.int32))


@_custom_op("graspqp_amd::box_qp_backward", mutates_args=(), device_types="cuda")
def _box_qp_bwd_op(Q: Tensor, lam: Tensor, slack: Tensor, gx: Tensor) -> Tuple[Tensor, Tensor]:
    B, nz = gx.shape
    dx = torch.empty(B, nz, device=gx.device)
    dlam = torch.empty(B, 2 * nz, device=gx.device)
    _C.call("gq_boxqp_backward", _C.f32(_c(Q)), _C.f32(lam), _C.f32(slack), _C.f32(_c(gx)), B, nz, _C.f32(dx), _C.f32(dlam),
            _C.stream_ptr())
    return dx, dlam


@_box_qp_bwd_op.register_fake
def _(Q, lam, slack, gx):
    return torch.empty_like(gx), torch.empty_like(lam)


def _box_qp_setup(ctx, inputs, output):
    ctx.save_for_backward(_c(inputs[0]), output[0], output[1], output[2])
    ctx.mark_non_differentiable(output[1], output[2], output[3])


def _box_qp_bwd(ctx, gx, g_lam, g_slack, g_nit):
    Qc, x, lam, slack = ctx.saved_tensors
    nz = x.shape[1]
    dx, dlam = _Eager.box_qp_backward(Qc, lam, slack, gx)
    gQ = 0.5 * (dx.unsqueeze(2) * x.unsqueeze(1) + x.unsqueeze(2) * dx.unsqueeze(1))
    # h = [upper; -lower]; grad_h = -dlam
    return gQ, dx, dlam[:, nz:], -dlam[:, :nz], None, None, None


torch.library.register_autograd("graspqp_amd::box_qp", _box_qp_bwd, setup_context=_box_qp_setup)


def box_qp(Q, p, lower, upper, eps=5e-2, max_iter=12, not_improved_lim=3):
    """argmin 1/2 x'Qx + p'x, lower <= x <= upper -> (x, lam, slack); differentiable (qpth semantics)."""
    if Q.is_cuda and Q.device.index != torch.cuda.current_device():  # launches go to the current device's stream
        with torch.cuda.device(Q.device):
            return box_qp(Q, p, lower, upper, eps, max_iter, not_improved_lim)
    x, lam, slack, _ = _Eager.box_qp(Q, p, lower, upper, float(eps), int(max_iter), int(not_improved_lim))
    return x, lam, slack


@_custom_op("graspqp_amd::lsq_box_qp", mutates_args=(), device_types="cuda")
def _lsq_box_qp_op(A: Tensor, b: Tensor, lower_s: float, upper_s: float, ridge: float, eps: float,
                   max_iter: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """x = argmin 1/2 x'(A'A + ridge I)x - (A'b)'x in the box (qp_solver.py:101-126) -> (x, lam, slack, n_iter)."""
    Ac, bc = _c(A), _c(b)
    B, m, nz = Ac.shape
    dev = Ac.device
    x = torch.empty(B, nz, device=dev)
    lam = torch.empty(B, 2 * nz, device=dev)
    slack = torch.empty(B, 2 * nz, device=dev)
    nit = torch.zeros(1, dtype=torch.int32, device=dev)
    ws, nb = _qp_ws(B, nz, max_iter, dev)
    _C.call("gq_lsq_boxqp_forward", _C.f32(Ac), _C.f32(bc), None, None, float(lower_s), float(upper_s), B, m, nz,
            float(ridge), float(eps), int(max_iter), 3, _C.f32(x), _C.f32(lam), _C.f32(slack), None, _C.i32(nit),
            _C.ptr(ws), nb, _C.stream_ptr())
    return x, lam, slack, nit


@_lsq_box_qp_op.register_fake
def _(A, b, lower_s, upper_s, ridge, eps, max_iter):
    B, m, nz = A.shape
    return (A.new_empty(B, nz), A.new_empty(B, 2 * nz), A.new_empty(B, 2 * nz), A.new_empty(1, dtype=torch.int32))


@_custom_op("graspqp_amd::lsq_box_qp_backward", mutates_args=(), device_types="cuda")
def _lsq_box_qp_bwd_op(A: Tensor, lam: Tensor, slack: Tensor, gx: Tensor, ridge: float) -> Tuple[Tensor, Tensor]:
    B, m, nz = A.shape
    dx = torch.empty(B, nz, device=A.device)
    dlam = torch.empty(B, 2 * nz, device=A.device)
    _C.call("gq_lsq_boxqp_backward", _C.f32(_c(A)), _C.f32(lam), _C.f32(slack), _C.f32(_c(gx)), B, m, nz, float(ridge),
            _C.f32(dx), _C.f32(dlam), _C.stream_ptr())
    return dx, dlam


@_lsq_box_qp_bwd_op.register_fake
def _(A, lam, slack, gx, ridge):
    return torch.empty_like(gx), torch.empty_like(lam)


def _lsq_setup(ctx, inputs, output):
    ctx.save_for_backward(_c(inputs[0]), _c(inputs[1]), output[0], output[1], output[2])
    ctx.ridge = inputs[4]
    ctx.mark_non_differentiable(output[1], output[2], output[3])


def _lsq_bwd(ctx, gx, g_lam, g_slack, g_nit):
    Ac, bc, x, lam, slack = ctx.saved_tensors
    dx, _ = _Eager.lsq_box_qp_backward(Ac, lam, slack, gx, ctx.ridge)
    # Q = A'A + ridge I -> grad_A = A (dx x' + x dx');  p = -A'b -> grad_A += -b dx', grad_b = -A dx
    Adx = (Ac @ dx.unsqueeze(-1)).squeeze(-1)
    Ax = (Ac @ x.unsqueeze(-1)).squeeze(-1)
    gA = Adx.unsqueeze(2) * x.unsqueeze(1) + Ax.unsqueeze(2) * dx.unsqueeze(1) - bc.unsqueeze(2) * dx.unsqueeze(1)
    return gA, -Adx, None, None, None, None, None


torch.library.register_autograd("graspqp_amd::lsq_box_qp", _lsq_bwd, setup_context=_lsq_setup)


def lsq_box_qp(A, b, lower, upper, ridge=1e-4, eps=5e-2, max_iter=12, return_n_iter=False):
    """x (B,nz); with ``return_n_iter`` also the (1,) int32 iteration count of qpth's batch-global stop rule."""
    if b is None:
        b = torch.zeros(A.shape[0], A.shape[1], device=A.device, dtype=A.dtype)
    x, _, _, nit = _Eager.lsq_box_qp(A, b, float(lower), float(upper), float(ridge), float(eps), int(max_iter))
    return (x, nit) if return_n_iter else x


# ----------------------------------------------------------------------------------------------------------
# fused force-closure energy
# ----------------------------------------------------------------------------------------------------------
@_custom_op("graspqp_amd::fc_energy", mutates_args=(), device_types="cuda")
def _fc_energy_op(contact_pts: Tensor, contact_normals: Tensor, cog: Tensor, n_cone_vecs: int, friction: float,
                  torque_weight: float, max_limit: float, svd_gain: float, values_gain: float, eps: float,
                  max_iter: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """-> (E_fc (B), force sums (B,n), n_iter (1) int32, workspace kept for the backward)."""
    cp, cn, cg = _c(contact_pts), _c(contact_normals), _c(cog)
    B, n, _ = cp.shape
    dev = cp.device
    e = torch.empty(B, device=dev)
    xs = torch.empty(B, n, device=dev)
    nit = torch.zeros(1, dtype=torch.int32, device=dev)
    nb = _size_call("gq_fc_workspace_bytes", ctypes.c_int64(B), n, int(n_cone_vecs), int(max_iter))
    ws = _ws(nb, dev)
    _C.call("gq_fc_forward", _C.f32(cp), _C.f32(cn), _C.f32(cg), B, n, int(n_cone_vecs), float(friction),
            float(torque_weight), float(max_limit), float(svd_gain), float(values_gain), float(eps), int(max_iter),
            _C.f32(e), _C.f32(xs), _C.i32(nit), _C.ptr(ws), nb, _C.stream_ptr())
    return e, xs, nit, ws


@_fc_energy_op.register_fake
def _(contact_pts, contact_normals, cog, n_cone_vecs, friction, torque_weight, max_limit, svd_gain, values_gain, eps, max_iter):
    B, n, _ = contact_pts.shape
    nb = _size_call("gq_fc_workspace_bytes", ctypes.c_int64(B), n, int(n_cone_vecs), int(max_iter))  # host-only helper
    return (contact_pts.new_empty(B), contact_pts.new_empty(B, n), contact_pts.new_empty(1, dtype=torch.int32),
            contact_pts.new_empty(nb, dtype=torch.uint8))


@_custom_op("graspqp_amd::fc_energy_backward", mutates_args=("ws",), device_types="cuda")  # scratch inside the workspace
def _fc_energy_bwd_op(contact_pts: Tensor, contact_normals: Tensor, cog: Tensor, ge: Tensor, ws: Tensor, n_cone_vecs: int,
                      friction: float, torque_weight: float, svd_gain: float, values_gain: float) -> Tensor:
    gp = torch.empty_like(contact_pts)
    B, n, _ = contact_pts.shape
    _C.call("gq_fc_backward", _C.f32(contact_pts), _C.f32(contact_normals), _C.f32(cog), _C.f32(_c(ge)), B, n,
            int(n_cone_vecs), float(friction), float(torque_weight), float(svd_gain), float(values_gain), 0, _C.f32(gp),
            _C.ptr(ws), ws.numel(), _C.stream_ptr())
    return gp


@_fc_energy_bwd_op.register_fake
def _(contact_pts, contact_normals, cog, ge, ws, n_cone_vecs, friction, torque_weight, svd_gain, values_gain):
    return torch.empty_like(contact_pts)


def _fc_setup(ctx, inputs, output):
    ctx.save_for_backward(_c(inputs[0]), _c(inputs[1]), _c(inputs[2]), output[3])
    ctx.cfg = inputs[3:]
    ctx.mark_non_differentiable(output[1], output[2], output[3])


def _fc_bwd(ctx, ge, g_xs, g_nit, g_ws):
    cp, cn, cg, ws = ctx.saved_tensors
    k, mu, tw, _ml, sg, vg, _eps, _mi = ctx.cfg
    gp = _Eager.fc_energy_backward(cp, cn, cg, ge, ws, k, mu, tw, sg, vg)
    return (gp,) + (None,) * 10


torch.library.register_autograd("graspqp_amd::fc_energy", _fc_bwd, setup_context=_fc_setup)


FC_DEFAULTS = dict(friction=0.2, n_cone_vecs=4, torque_weight=5.0, max_limit=20.0, svd_gain=0.1, values_gain=2.0,
                   eps=5e-2, max_iter=12)


def fc_energy(contact_pts, contact_normals, cog, return_n_iter=False, **cfg):
    """E_fc (B,) and per-contact force sums (B,n); gradient flows to contact_pts only (normals are SDF constants)."""
    c = dict(FC_DEFAULTS)
    c.update(cfg)
    e, xs, nit, _ = _Eager.fc_energy(
        contact_pts, contact_normals.detach(), cog.detach(), int(c["n_cone_vecs"]), float(c["friction"]),
        float(c["torque_weight"]), float(c["max_limit"]), float(c["svd_gain"]), float(c["values_gain"]), float(c["eps"]),
        int(c["max_iter"]))
    return (e, xs, nit) if return_n_iter else (e, xs)


# ----------------------------------------------------------------------------------------------------------
# exact grasp-quality metrics: bounded least squares to optimality (csrc/exact.hip).  No autograd: the outputs are
# values of a finished grasp set, as the reference's numpy-solved ones are.
# ----------------------------------------------------------------------------------------------------------
LSQ_EXACT_MAX_ITER = 512  # free-set solves per problem (scipy's BVLS needed <= 39 at nz = 96 on span problems)


@_custom_op("graspqp_amd::lsq_box_exact", mutates_args=(), device_types="cuda")
def _lsq_box_exact_op(A: Tensor, b: Tensor, lower: float, upper: float, max_iter: int) -> Tuple[Tensor, Tensor, Tensor]:
    """argmin 1/2 |A x - b|^2, lower <= x <= upper, exactly (scipy_solver.py:61-131) -> (x (B,nz), cost (B), status (B))."""
    dt = A.dtype if A.dtype in (torch.float32, torch.float64) else torch.float32
    Ac, bc = _c(A, dt), _c(b, dt)
    B, m, nz = Ac.shape
    x = torch.empty(B, nz, device=Ac.device, dtype=dt)
    cost = torch.empty(B, device=Ac.device, dtype=dt)
    status = torch.empty(B, device=Ac.device, dtype=torch.int32)
    _C.call("gq_lsq_exact_forward", _C.ptr(Ac), _C.ptr(bc), int(dt == torch.float64), ctypes.c_int64(B), m, nz,
            float(lower), float(upper), int(max_iter), _C.ptr(x), _C.ptr(cost), _C.i32(status), _C.stream_ptr())
    return x, cost, status


@_lsq_box_exact_op.register_fake
def _(A, b, lower, upper, max_iter):
    B, m, nz = A.shape
    dt = A.dtype if A.dtype in (torch.float32, torch.float64) else torch.float32
    return A.new_empty(B, nz, dtype=dt), A.new_empty(B, dtype=dt), A.new_empty(B, dtype=torch.int32)


def lsq_box_exact(A, b, lower, upper, max_iter=LSQ_EXACT_MAX_ITER):
    """Batched exact bounded least squares: A (B,m,nz) with m <= 8, nz <= 128, b (B,m), scalar bounds; fp32 or fp64 in,
    fp64 arithmetic, outputs in the input dtype.  status >= 0: solves used, -1: iteration cap, -2: non-finite input."""
    return _Eager.lsq_box_exact(A.detach(), b.detach(), float(lower), float(upper), int(max_iter))


@_custom_op("graspqp_amd::span_exact", mutates_args=(), device_types="cuda")
def _span_exact_op(contact_pts: Tensor, contact_normals: Tensor, cog: Tensor, n_cone_vecs: int, friction: float,
                   torque_weight: float, n_basis: int, lower: float, upper: float,
                   max_iter: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """Span metric solved exactly, F built once per row on the device -> (value (B,nb), x_sum (B,nb,n), svd (B),
    status (B,nb)); n_basis 1: overall (span.py:313-415), 12: Euclidean (span.py:94-231)."""
    cp, cn, cg = _c(contact_pts), _c(contact_normals), _c(cog)
    B, n, _ = cp.shape
    dev = cp.device
    value = torch.empty(B, n_basis, device=dev)
    x_sum = torch.empty(B, n_basis, n, device=dev)
    svd = torch.empty(B, device=dev)
    status = torch.empty(B, n_basis, device=dev, dtype=torch.int32)
    _C.call("gq_span_exact_forward", _C.f32(cp), _C.f32(cn), _C.f32(cg), ctypes.c_int64(B), n, int(n_cone_vecs),
            float(friction), float(torque_weight), int(n_basis), float(lower), float(upper), int(max_iter), _C.f32(value),
            _C.f32(x_sum), _C.f32(svd), _C.i32(status), _C.stream_ptr())
    return value, x_sum, svd, status


@_span_exact_op.register_fake
def _(contact_pts, contact_normals, cog, n_cone_vecs, friction, torque_weight, n_basis, lower, upper, max_iter):
    B, n, _ = contact_pts.shape
    f = dict(dtype=torch.float32)
    return (contact_pts.new_empty(B, n_basis, **f), contact_pts.new_empty(B, n_basis, n, **f), contact_pts.new_empty(B, **f),
            contact_pts.new_empty(B, n_basis, dtype=torch.int32))


def span_exact(contact_pts, contact_normals, cog, n_cone_vecs=4, friction=0.2, torque_weight=5.0, n_basis=1, lower=1.0,
               upper=51.0, max_iter=LSQ_EXACT_MAX_ITER):
    """-> (value, x_sum, svd, status); non-differentiable."""
    return _Eager.span_exact(contact_pts.detach(), contact_normals.detach(), cog.detach(), int(n_cone_vecs),
                             float(friction), float(torque_weight), int(n_basis), float(lower), float(upper),
                             int(max_iter))


# ----------------------------------------------------------------------------------------------------------
# the reference's other force-closure energies: dexgrasp (||G'n||^2) and TDG (grasp-wrench-space directions)
# ----------------------------------------------------------------------------------------------------------
@_custom_op("graspqp_amd::dexgrasp_energy", mutates_args=(), device_types="cuda")
def _dexgrasp_op(contact_pts: Tensor, contact_normals: Tensor, cog: Tensor, torque_weight: float) -> Tuple[Tensor, Tensor]:
    """-> (E (B), dE/d contact_pts (B,n,3)); metrics/ops/dexgrasp.py:4-34."""
    cp, cn, cg = _c(contact_pts), _c(contact_normals), _c(cog)
    B, n, _ = cp.shape
    e = torch.empty(B, device=cp.device)
    g = torch.empty_like(cp)
    _C.call("gq_dexgrasp_energy", _C.f32(cp), _C.f32(cn), _C.f32(cg), ctypes.c_int64(B), n, float(torque_weight), None, 1.0, 0,
            _C.f32(e), _C.f32(g), _C.stream_ptr())
    return e, g


@_dexgrasp_op.register_fake
def _(contact_pts, contact_normals, cog, torque_weight):
    return contact_pts.new_empty(contact_pts.shape[0]), torch.empty_like(contact_pts)


@_custom_op("graspqp_amd::tdg_energy", mutates_args=(), device_types="cuda")
def _tdg_op(contact_pts: Tensor, contact_normals: Tensor, cog: Tensor, directions: Tensor, friction: float, obb_length: float,
            enable_density: bool, scale: float) -> Tuple[Tensor, Tensor]:
    """-> (E (B), dE/d contact_pts (B,n,3)); metrics/ops/tdg.py:147-239."""
    cp, cn, cg, dr = _c(contact_pts), _c(contact_normals), _c(cog), _c(directions)
    B, n, _ = cp.shape
    e = torch.empty(B, device=cp.device)
    g = torch.empty_like(cp)
    _C.call("gq_tdg_energy", _C.f32(cp), _C.f32(cn), _C.f32(cg), _C.f32(dr), dr.shape[0], ctypes.c_int64(B), n, float(friction),
            float(obb_length), int(bool(enable_density)), float(scale), None, 1.0, 0, _C.f32(e), _C.f32(g), _C.stream_ptr())
    return e, g


@_tdg_op.register_fake
def _(contact_pts, contact_normals, cog, directions, friction, obb_length, enable_density, scale):
    return contact_pts.new_empty(contact_pts.shape[0]), torch.empty_like(contact_pts)


def _alt_setup(ctx, inputs, output):
    ctx.save_for_backward(output[1])
    ctx.n_in = len(inputs)
    ctx.mark_non_differentiable(output[1])


def _alt_bwd(ctx, ge, gg):
    (g,) = ctx.saved_tensors
    return (g * ge.view(-1, 1, 1),) + (None,) * (ctx.n_in - 1)


torch.library.register_autograd("graspqp_amd::dexgrasp_energy", _alt_bwd, setup_context=_alt_setup)
torch.library.register_autograd("graspqp_amd::tdg_energy", _alt_bwd, setup_context=_alt_setup)


def dexgrasp_energy(contact_pts, contact_normals, cog, torque_weight=0.0):
    """(B,) DexGraspNet force-closure term; gradient to contact_pts (the normals are SDF constants)."""
    return _Eager.dexgrasp_energy(contact_pts, contact_normals.detach(), cog.detach(), float(torque_weight))[0]


def tdg_energy(contact_pts, contact_normals, cog, directions, friction=0.2, obb_length=0.2, enable_density=True, scale=100.0):
    return _Eager.tdg_energy(contact_pts, contact_normals.detach(), cog.detach(), directions, float(friction),
                                            float(obb_length), bool(enable_density), float(scale))[0]


def fc_peek(ws, B, n, k):
    """(F, x, val, svd) views of the last fc_energy forward on workspace ``ws`` (tests)."""
    outs = [ctypes.c_void_p(0) for _ in range(4)]
    _C.call("gq_fc_peek", _C.ptr(ws), ws.numel(), B, n, k, *[ctypes.byref(o) for o in outs])
    return outs


# ----------------------------------------------------------------------------------------------------------
# hand handle + kinematics
# ----------------------------------------------------------------------------------------------------------
class HandHandle(_DeviceObject):
    """Device copy of a HandSpec's reduced kinematic tree + its link meshes."""

    def __init__(self, spec, device=None):
        if isinstance(spec, str):
            from .hands import get_hand_spec

            spec = get_hand_spec(spec)
        self.spec = spec
        keep = []

        def arr(a, dt):
            a = np.ascontiguousarray(np.asarray(a, dtype=dt))
            keep.append(a)
            return a.ctypes.data_as(ctypes.c_void_p)

        d = _C.HandDesc()
        d.n_dofs, d.n_links = spec.n_nodes, spec.n_links  # tree joints; the pose carries spec.n_dofs actuated ones
        d.n_cand, d.n_spheres = spec.n_contact_candidates, spec.n_spheres
        d.node_parent = arr(spec.node_parent, np.int32)
        d.node_type = arr(spec.node_type, np.int32)
        d.node_pre = arr(spec.node_pre[:, :3, :], np.float32)
        d.node_axis = arr(spec.node_axis, np.float32)
        d.link_node = arr(spec.link_node, np.int32)
        d.link_offset = arr(spec.link_offset[:, :3, :], np.float32)
        d.cand_pos = arr(spec.cand_pos, np.float32)
        d.cand_nrm = arr(spec.cand_nrm, np.float32)
        d.cand_link = arr(spec.cand_link, np.int32)
        d.sphere = arr(spec.sphere, np.float32)
        d.sphere_link = arr(spec.sphere_link, np.int32)
        d.joints_lower = arr(spec.joints_lower, np.float32)
        d.joints_upper = arr(spec.joints_upper, np.float32)
        if spec.is_coupled:  # theta_tree = coupling theta_actuated + offset (ability_hand, panda)
            d.n_actuated = spec.n_dofs
            d.coupling = arr(spec.coupling, np.float32)
            d.coupling_offset = arr(spec.coupling_offset, np.float32)
        super().__init__("gq_hand_create", "gq_hand_destroy", device, ctypes.byref(d))
        self.links = MeshSet([spec.link_faces(l) for l in range(spec.n_links)], self.device)
        with torch.cuda.device(self.device):
            _C.call("gq_meshset_build_occupancy", self.links.handle)
        self.J, self.L, self.S = spec.n_dofs, spec.n_links, spec.n_spheres
        self.hid = _register_handle(self)

    def fk_ws(self, B, dev):
        nb = _size_call("gq_fk_workspace_bytes", self.handle, ctypes.c_int64(B))
        return _ws(nb, dev), nb

    def close(self):
        links = getattr(self, "links", None)
        if links is not None:
            links.close()
        super().close()


@_custom_op("graspqp_amd::fk_contacts", mutates_args=(), device_types="cuda")
def _fk_op(hand_pose: Tensor, idx: Tensor, hand: int) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """hand_pose, contact idx -> (Rg (B,3,3), link_T (B,L,3,4), contact_points, contact_normals, sphere_centers,
    FK workspace holding the per-joint frames for the backward)."""
    h = _handle(hand)
    hp = _c(hand_pose)
    ix = _c(idx, torch.int64)
    B, n = ix.shape
    dev = hp.device
    Rg = torch.empty(B, 3, 3, device=dev)
    LT = torch.empty(B, h.L, 3, 4, device=dev)
    cp = torch.empty(B, n, 3, device=dev)
    cn = torch.empty(B, n, 3, device=dev)
    sc = torch.empty(B, max(h.S, 1), 3, device=dev)
    ws, nb = h.fk_ws(B, dev)
    _C.call("gq_fk_forward", h.handle, _C.f32(hp), _C.i64(ix), B, n, _C.f32(Rg), _C.f32(LT), _C.f32(cp),
            _C.f32(cn), _C.f32(sc) if h.S > 0 else None, 0.0, None, None, None, None, _C.ptr(ws), nb, _C.stream_ptr())
    return Rg, LT, cp, cn, sc[:, : h.S].contiguous(), ws


@_fk_op.register_fake
def _(hand_pose, idx, hand):
    h = _handle(hand)
    B, n = idx.shape
    e = hand_pose.new_empty
    nb = _size_call("gq_fk_workspace_bytes", h.handle, ctypes.c_int64(B))
    return (e(B, 3, 3), e(B, h.L, 3, 4), e(B, n, 3), e(B, n, 3), e(B, h.S, 3), e(nb, dtype=torch.uint8))


@_custom_op("graspqp_amd::fk_backward", mutates_args=(), device_types="cuda")
def _fk_bwd_op(hand: int, hand_pose: Tensor, idx: Tensor, Rg: Tensor, LT: Tensor, ws: Tensor, gcp: Tensor, gcn: Tensor,
               gsc: Tensor, wrench: Tensor, gRt: Tensor, gR: Tensor, has: List[bool]) -> Tensor:
    """Analytic FK backward (replaces autograd through pytorch_kinematics).  ``has`` flags which of the six gradient
    inputs (contact points, contact normals, sphere centres, link wrench, g_Rt, g_R) are present; absent ones are
    passed as empty tensors (only tensors may cross the dispatcher)."""
    h = _handle(hand)
    B, n = idx.shape
    gp = torch.empty_like(hand_pose)
    opt = lambda t, on: _C.f32(_c(t)) if on else None
    _C.call("gq_fk_backward", h.handle, _C.f32(hand_pose), _C.i64(idx), B, n, _C.f32(_c(Rg)), _C.f32(_c(LT)),
            opt(gcp, has[0]), opt(gcn, has[1]), opt(gsc, has[2] and h.S > 0), opt(wrench, has[3]), opt(gRt, has[4]), None,
            opt(gR, has[5]), _C.f32(gp), None, None, _C.ptr(ws), ws.numel(), _C.stream_ptr())
    return gp


@_fk_bwd_op.register_fake
def _(hand, hand_pose, idx, Rg, LT, ws, gcp, gcn, gsc, wrench, gRt, gR, has):
    return torch.empty_like(hand_pose)


def _fk_backward(hand, hp, ix, Rg, LT, ws, gcp=None, gcn=None, gsc=None, wrench=None, gRt=None, gR=None):
    z = hp.new_empty(0)
    args = [gcp, gcn, gsc, wrench, gRt, gR]
    return _Eager.fk_backward(hand.hid, hp, ix, Rg, LT, ws, *[z if a is None else a for a in args],
                                             [a is not None for a in args])


def _fk_setup(ctx, inputs, output):
    ctx.save_for_backward(_c(inputs[0]), _c(inputs[1], torch.int64), output[0], output[1], output[5])
    ctx.hand = inputs[2]
    ctx.mark_non_differentiable(output[5])


def _fk_bwd(ctx, gRg, gLT, gcp, gcn, gsc, gws):
    hp, ix, Rg, LT, ws = ctx.saved_tensors
    # d / d link_T is routed through hand_pen's link wrenches, never through link_T itself: autograd hands a zero (or
    # no) gradient here, which is ignored
    return _fk_backward(_handle(ctx.hand), hp, ix, Rg, LT, ws, gcp, gcn, gsc, None, None, gRg), None, None


torch.library.register_autograd("graspqp_amd::fk_contacts", _fk_bwd, setup_context=_fk_setup)


def fk_contacts(hand_pose, idx, hand: HandHandle):
    """-> (Rg (B,3,3), link_T (B,L,3,4), contact_points, contact_normals, sphere_centers, fk workspace)."""
    if not hand_pose.is_cuda:
        raise RuntimeError("graspqp_amd ops need CUDA (ROCm) tensors; got a CPU tensor")
    return _Eager.fk_contacts(hand_pose, idx, hand.hid)


# ----------------------------------------------------------------------------------------------------------
# export-time kinematics (scripts/fit.py:224-300): explicit Jacobians, damped pseudo-inverse, root pose
# ----------------------------------------------------------------------------------------------------------
def link_jacobian(hand: HandHandle, link_T, fk_workspace):
    """(B,L,6,J) geometric Jacobian [J_v; J_w] of every mesh link in the hand frame (HandModel.jacobian)."""
    LT = _c(link_T.detach())
    B = LT.shape[0]
    out = torch.empty(B, hand.L, 6, hand.J, device=LT.device)
    _C.call("gq_link_jacobian", hand.handle, ctypes.c_int64(B), _C.f32(LT), _C.f32(out), _C.ptr(fk_workspace),
            fk_workspace.numel(), _C.stream_ptr())
    return out


def contact_jacobian(hand: HandHandle, contact_idx, link_T, fk_workspace):
    """(B,n,3,J) linear contact Jacobian J_v + J_w x r (hand_model.py:1176-1196), hand frame."""
    LT = _c(link_T.detach())
    ix = _c(contact_idx, torch.int64)
    B, n = ix.shape
    out = torch.empty(B, n, 3, hand.J, device=LT.device)
    _C.call("gq_contact_jacobian", hand.handle, _C.i64(ix), ctypes.c_int64(B), n, _C.f32(LT), _C.f32(out),
            _C.ptr(fk_workspace), fk_workspace.numel(), _C.stream_ptr())
    return out


def joint_velocities(jac, directions, Rg=None, damping=1e-3):
    """theta = pinv_damped(J) d (hand_model.py:46-54,1198-1218).  jac (B,m,J), directions (B,m) -- world frame when
    Rg (B,3,3) is given.  -> (theta (B,J), residual (B,m), ee_vel (B,m))."""
    Jc = _c(jac.detach())
    d = _c(directions.detach())
    B, m, J = Jc.shape
    theta = torch.empty(B, J, device=Jc.device)
    res = torch.empty(B, m, device=Jc.device)
    ee = torch.empty(B, m, device=Jc.device)
    R = None if Rg is None else _c(Rg.detach()).reshape(B, 9)
    _C.call("gq_joint_velocities", _C.f32(Jc), _C.f32(d), _C.f32(R), ctypes.c_int64(B), m, J, float(damping),
            _C.f32(theta), _C.f32(res), _C.f32(ee), _C.stream_ptr())
    return theta, res, ee


class _JointVelocityResiduals(torch.autograd.Function):
    """residuals (B,3n) = (J theta - d_h)^2 with theta = pinv_damped(J) d_h, d_h = R' d (hand_model.py:1155-1218, coupled form),
    differentiable w.r.t. hand_pose (joint angles through the contact Jacobian -- analytic kinematic Hessian,
    gq_contact_jacobian_backward -- and the root rotation through d_h) and w.r.t. the moving directions d: what autograd
    through pytorch_kinematics gives the reference for E_manipulativity (core/energy.py:80-87).  The kinematic state
    (link transforms, FK workspace, root rotation) is the one of ``hand_pose``, passed in detached."""

    @staticmethod
    def forward(ctx, hand_pose, directions, hand, idx, Rg, LT, ws, damping):
        hp, d, R = _c(hand_pose.detach()), _c(directions.detach()), _c(Rg.detach())
        ix = _c(idx, torch.int64)
        B, n = ix.shape
        jc = contact_jacobian(hand, ix, LT, ws).reshape(B, 3 * n, hand.J)
        theta, res, _ = joint_velocities(jc, d.reshape(B, 3 * n), R, damping)
        d_h = (R.transpose(1, 2).unsqueeze(1) @ d.unsqueeze(-1)).squeeze(-1).reshape(B, 3 * n)
        r = (jc @ theta.unsqueeze(-1)).squeeze(-1) - d_h  # signed residual, hand frame
        ctx.save_for_backward(hp, d, R, ix, _c(LT.detach()), ws, jc, theta, r)
        ctx.hand, ctx.damping = hand, damping
        ctx.mark_non_differentiable(theta)
        return theta, res

    @staticmethod
    def backward(ctx, _g_theta, g_res):
        hp, d, R, ix, LT, ws, jc, theta, r = ctx.saved_tensors
        hand = ctx.hand
        B, n = ix.shape
        g = 2.0 * g_res * r                                           # d E / d r
        u, _, _ = joint_velocities(jc, g, None, ctx.damping)          # (J'J + lambda I)^-1 J' g
        w = g - (jc @ u.unsqueeze(-1)).squeeze(-1)                    # (I - J M^-1 J') g
        GJ = (w.unsqueeze(-1) * theta.unsqueeze(1) - r.unsqueeze(-1) * u.unsqueeze(1)).contiguous()  # d E / d J  (B,3n,J)
        g_dh = (-w).reshape(B, n, 3)                                  # d E / d d_h
        g_d = (R.unsqueeze(1) @ g_dh.unsqueeze(-1)).squeeze(-1)       # d_h = R' d
        gR = (d.unsqueeze(-1) * g_dh.unsqueeze(-2)).sum(1).contiguous()  # (B,3,3): dE/dR[a,c] = sum_i d[i,a] g_dh[i,c]
        g_th = torch.empty(B, hand.J, device=hp.device)
        _C.call("gq_contact_jacobian_backward", hand.handle, _C.i64(ix), ctypes.c_int64(B), n, _C.f32(LT), _C.f32(GJ),
                _C.f32(g_th), _C.ptr(ws), ws.numel(), _C.stream_ptr())
        ghp = _fk_backward(hand, hp, ix, R, LT, ws, None, None, None, None, None, gR).clone()
        ghp[:, hp.shape[1] - hand.J:] += g_th
        return ghp, g_d, None, None, None, None, None, None


def joint_velocity_residuals(hand_pose, directions, hand: HandHandle, idx, Rg, LT, ws, damping=1e-3):
    """-> (theta (B,J), residuals (B,3n)); see _JointVelocityResiduals."""
    return _JointVelocityResiduals.apply(hand_pose, directions, hand, idx, Rg, LT, ws, float(damping))


def root_pose_wxyz(hand_pose):
    """(B,7) = [translation, unit quaternion (w,x,y,z)] of hand_pose[:, :9] (fit.py:260-263)."""
    hp = _c(hand_pose.detach())
    out = torch.empty(hp.shape[0], 7, device=hp.device)
    _C.call("gq_root_pose_wxyz", _C.f32(hp), ctypes.c_int64(hp.shape[0]), hp.shape[1], _C.f32(out), _C.stream_ptr())
    return out


@_custom_op("graspqp_amd::hand_pen", mutates_args=(), device_types="cuda")
def _hand_pen_op(hand_pose: Tensor, surface_points: Tensor, batch_each: int, hand: int, Rg: Tensor, LT: Tensor,
                 penetration_only: int) -> Tuple[Tensor, Tensor, Tensor]:
    """max-over-links signed distance (inside positive) of object surface points -> (dis (B,P), argmax link, d dis / d x_h).

    The kinematic state (Rg, link_T) is passed in detached; the gradient is routed to ``hand_pose`` directly through the
    analytic FK backward (link wrenches), which is what autograd through pytorch_kinematics computes in the reference
    (hand_model.py:875-987)."""
    h = _handle(hand)
    hp = _c(hand_pose)
    sp = _c(surface_points)
    n_obj, P, _ = sp.shape
    B = hp.shape[0]
    dev = hp.device
    dis = torch.empty(B, P, device=dev)
    link = torch.zeros(B, P, dtype=torch.int32, device=dev)  # mode 1 writes link / gvec only where dis > 0
    gvec = torch.zeros(B, P, 3, device=dev)
    _C.call("gq_hand_pen_forward", h.links.handle, _C.f32(sp), n_obj, P, int(batch_each), _C.f32(hp), hp.shape[1],
            _C.f32(_c(Rg)), _C.f32(_c(LT)), int(penetration_only), _C.f32(dis), _C.i32(link), _C.f32(gvec), None, 0,
            None, None, None, _C.stream_ptr())
    return dis, link, gvec


@_hand_pen_op.register_fake
def _(hand_pose, surface_points, batch_each, hand, Rg, LT, penetration_only):
    B, P = hand_pose.shape[0], surface_points.shape[1]
    return (hand_pose.new_empty(B, P), hand_pose.new_empty(B, P, dtype=torch.int32), hand_pose.new_empty(B, P, 3))


@_custom_op("graspqp_amd::hand_pen_backward", mutates_args=(), device_types="cuda")
def _hand_pen_bwd_op(n_links: int, surface_points: Tensor, batch_each: int, hand_pose: Tensor, Rg: Tensor, g: Tensor,
                     link: Tensor, gvec: Tensor) -> Tuple[Tensor, Tensor]:
    sp = _c(surface_points)
    n_obj, P, _ = sp.shape
    B = hand_pose.shape[0]
    wrench = torch.empty(B, n_links, 6, device=g.device)
    gRt = torch.empty(B, 12, device=g.device)
    _C.call("gq_hand_pen_backward", int(n_links), _C.f32(sp), n_obj, P, int(batch_each), _C.f32(hand_pose), hand_pose.shape[1],
            _C.f32(_c(Rg)), _C.f32(_c(g)), _C.i32(link), _C.f32(gvec), _C.f32(wrench), _C.f32(gRt), None, 0.0, None, None, None,
            _C.stream_ptr())
    return wrench, gRt


@_hand_pen_bwd_op.register_fake
def _(n_links, surface_points, batch_each, hand_pose, Rg, g, link, gvec):
    B = hand_pose.shape[0]
    return hand_pose.new_empty(B, n_links, 6), hand_pose.new_empty(B, 12)


def pen_mode(penetration_only) -> int:
    """0 (False: the exact query) or 1 (True: exact only where dis > 0, which is all E_pen reads); anything else raises."""
    if penetration_only not in (0, 1):  # bools included
        raise ValueError(f"penetration_only={penetration_only!r}: accepted values are False / 0 (exact query) and "
                         "True / 1 (penetration-only query)")
    return int(penetration_only)


def hand_pen(hand_pose, surface_points, batch_each, hand, idx, Rg, LT, ws, nb=None, penetration_only=False):
    """(B,P) max-over-links signed distance, differentiable w.r.t. hand_pose (see the op's docstring)."""
    return _HandPen.apply(hand_pose, surface_points, int(batch_each), hand, idx, Rg.detach(), LT.detach(), ws,
                          pen_mode(penetration_only))


class _HandPen(torch.autograd.Function):
    """Glue between two registered ops (hand_pen + fk_backward): the backward needs the hand's FK workspace and contact
    indices, which are not inputs of the distance query itself."""

    @staticmethod
    def forward(ctx, hand_pose, surface_points, batch_each, hand, idx, Rg, LT, ws, penetration_only):
        hp = _c(hand_pose.detach())
        sp = _c(surface_points)
        dis, link, gvec = _Eager.hand_pen(hp, sp, batch_each, hand.hid, Rg, LT, penetration_only)
        ctx.save_for_backward(hp, sp, idx, Rg, LT, ws, link, gvec)
        ctx.hand, ctx.batch_each = hand, batch_each
        return dis

    @staticmethod
    def backward(ctx, g):
        hp, sp, idx, Rg, LT, ws, link, gvec = ctx.saved_tensors
        hand = ctx.hand
        wrench, gRt = _Eager.hand_pen_backward(hand.L, sp, ctx.batch_each, hp, Rg, g, link, gvec)
        gp = _fk_backward(hand, hp, idx, Rg, LT, ws, None, None, None, wrench, gRt, None)
        return gp, None, None, None, None, None, None, None, None


# ----------------------------------------------------------------------------------------------------------
# tabletop terms (core/energy.py:68-78): E_prior and E_wall on the hand's surface samples, one launch (csrc/tabletop.hip)
# ----------------------------------------------------------------------------------------------------------
class SurfaceSamples:
    """Samples of a hand's surface on the device: ``points`` (Ns,3) float32 in the link frames, ``link`` (Ns) int32.  They
    are RE-ORDERED by link (stable sort), which keeps the 64-sample chunks of the kernel on few links: ``points`` / ``link``
    hold the same set as the arrays passed in, but not in the caller's order unless that was already by link -- read the
    samples back from here when they must match (HandModel.set_surface_points, the oracle).  The terms depend on the order
    only in their last bits.  ``spec_or_hand``: the HandSpec or HandHandle the link ids refer to."""

    def __init__(self, spec_or_hand, points, link_ids, device="cuda"):
        spec = getattr(spec_or_hand, "spec", spec_or_hand)
        pts = np.ascontiguousarray(np.asarray(points.detach().cpu() if torch.is_tensor(points) else points, dtype=np.float32))
        lnk = np.ascontiguousarray(np.asarray(link_ids.detach().cpu() if torch.is_tensor(link_ids) else link_ids, dtype=np.int32))
        if pts.ndim != 2 or pts.shape[1] != 3 or lnk.shape != (pts.shape[0],):
            raise ValueError(f"SurfaceSamples: points must be (Ns,3) and link_ids (Ns), got {pts.shape} / {lnk.shape}")
        self.n_links, self.Ns = int(spec.n_links), int(pts.shape[0])
        _C.call("gq_tabletop_check", ctypes.c_int64(1), self.n_links, ctypes.c_int64(self.Ns))
        if lnk.min() < 0 or lnk.max() >= self.n_links:
            raise ValueError(f"SurfaceSamples: link ids must lie in [0, {self.n_links})")
        order = np.argsort(lnk, kind="stable")
        self.points = torch.from_numpy(pts[order]).to(device).contiguous()
        self.link = torch.from_numpy(lnk[order]).to(device).contiguous()
        self._host = (pts[order], lnk[order])
        self._moments = None

    @property
    def link_moments(self) -> Tensor:
        """(n_links,10) float32 on the device, built at the first use from the host copy of the samples: per link the number of
        samples n, their centroid c (3) and the centred second moment sum (p - c)(p - c)' as Cxx Cxy Cxz Cyy Cyz Czz, summed in
        fp64.  A link without samples has a row of zeros.  ``grasp_distances`` / ``grasp_select`` read the hand surface through
        these 10 numbers per link."""
        if self._moments is None:
            pts, lnk = self._host
            m = np.zeros((self.n_links, 10), np.float64)
            for l in np.unique(lnk):
                p = pts[lnk == l].astype(np.float64)
                c = p.mean(0)
                C = (p - c).T @ (p - c)
                m[l] = [len(p), *c, C[0, 0], C[0, 1], C[0, 2], C[1, 1], C[1, 2], C[2, 2]]
            self._moments = torch.from_numpy(m.astype(np.float32)).to(self.points.device)
        return self._moments


def _axis3(grasp_axis) -> List[float]:
    a = grasp_axis.detach().cpu().tolist() if torch.is_tensor(grasp_axis) else [float(x) for x in grasp_axis]
    if len(a) != 3:
        raise ValueError(f"grasp_axis must have 3 entries, got {len(a)}")
    return [float(x) for x in a]


def _axis_c(axis):
    """The float[3] a launch reads its axis from: a ready ctypes array as it is (the stepper builds its own once), else one
    made of the sequence."""
    return axis if isinstance(axis, ctypes.Array) else (ctypes.c_float * 3)(*(float(a) for a in axis))


def _dev(t, dtype=torch.float32):
    """A launch's device pointer: of a tensor, checked at every call (``_C.ptr``); or the pointer a caller made with ``_C.f32`` /
    ``_C.i32`` of a buffer that stays where it is (the stepper converts its own buffers once), passed on as it is; None is NULL."""
    return t if t is None or type(t) is ctypes.c_void_p else _C.ptr(t, dtype)


def _tabletop_call(hp, points, link, n_links, Rg, LT, axis, table_z, up_wall, w_wall, up_prior, w_prior, e_wall, e_prior,
                   accumulate, wrench, gRt, gR, st=None):
    p, (B, D) = _dev, hp.shape  # sizes as plain ints, the axis as its array: the prototypes convert them
    _C.call("gq_tabletop_terms", _C.f32(points), p(link, torch.int32), points.shape[0], int(n_links), _C.f32(hp), D, p(Rg), p(LT),
            B, _axis_c(axis), float(table_z), p(up_wall), float(w_wall), p(up_prior), float(w_prior), p(e_wall), p(e_prior),
            int(accumulate), p(wrench), p(gRt), p(gR), _C.stream_ptr() if st is None else st)


@_custom_op("graspqp_amd::tabletop_terms", mutates_args=(), device_types="cuda")
def _tabletop_op(hand_pose: Tensor, points: Tensor, link: Tensor, n_links: int, Rg: Tensor, LT: Tensor, grasp_axis: List[float],
                 table_z: float) -> Tuple[Tensor, Tensor]:
    """-> (E_prior (B), E_wall (B)), unweighted (core/energy.py:68-78 with the plane z = table_z).  The kinematic state
    (Rg, link_T) is the one of ``hand_pose``, passed in detached, as for hand_pen."""
    hp = _c(hand_pose)
    B = hp.shape[0]
    e_prior, e_wall = torch.empty(B, device=hp.device), torch.empty(B, device=hp.device)
    _tabletop_call(hp, _c(points), _c(link, torch.int32), n_links, _c(Rg), _c(LT), grasp_axis, table_z, None, 0.0, None, 0.0,
                   e_wall, e_prior, 0, None, None, None)
    return e_prior, e_wall


@_tabletop_op.register_fake
def _(hand_pose, points, link, n_links, Rg, LT, grasp_axis, table_z):
    B = hand_pose.shape[0]
    return hand_pose.new_empty(B), hand_pose.new_empty(B)


@_custom_op("graspqp_amd::tabletop_terms_backward", mutates_args=(), device_types="cuda")
def _tabletop_bwd_op(hand_pose: Tensor, points: Tensor, link: Tensor, n_links: int, Rg: Tensor, LT: Tensor,
                     grasp_axis: List[float], table_z: float, g_prior: Tensor, g_wall: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """Upstream row gradients (B) on (E_prior, E_wall) -> (link wrench (B,L,6), gRt (B,12), g_R (B,9)) for fk_backward."""
    hp = _c(hand_pose)
    B, dev = hp.shape[0], hp.device
    wrench, gRt, gR = torch.empty(B, n_links, 6, device=dev), torch.empty(B, 12, device=dev), torch.empty(B, 9, device=dev)
    _tabletop_call(hp, _c(points), _c(link, torch.int32), n_links, _c(Rg), _c(LT), grasp_axis, table_z, _c(g_wall), 0.0,
                   _c(g_prior), 0.0, None, None, 0, wrench, gRt, gR)
    return wrench, gRt, gR


@_tabletop_bwd_op.register_fake
def _(hand_pose, points, link, n_links, Rg, LT, grasp_axis, table_z, g_prior, g_wall):
    B = hand_pose.shape[0]
    return hand_pose.new_empty(B, n_links, 6), hand_pose.new_empty(B, 12), hand_pose.new_empty(B, 9)


class _TabletopTerms(torch.autograd.Function):
    """Glue between two registered ops (tabletop_terms + fk_backward), as _HandPen: the terms hand link wrenches and the
    global-pose gradients to the analytic FK backward, which needs the hand's FK workspace and contact indices."""

    @staticmethod
    def forward(ctx, hand_pose, hand, samples, idx, Rg, LT, ws, axis, table_z):
        hp = _c(hand_pose.detach())
        e_prior, e_wall = _Eager.tabletop_terms(hp, samples.points, samples.link, hand.L, Rg, LT, axis, table_z)
        ctx.save_for_backward(hp, idx, Rg, LT, ws, samples.points, samples.link)
        ctx.hand, ctx.axis, ctx.table_z = hand, axis, table_z
        return e_prior, e_wall

    @staticmethod
    def backward(ctx, g_prior, g_wall):
        hp, idx, Rg, LT, ws, points, link = ctx.saved_tensors
        hand = ctx.hand
        wrench, gRt, gR = _Eager.tabletop_terms_backward(hp, points, link, hand.L, Rg, LT, ctx.axis, ctx.table_z, g_prior, g_wall)
        gp = _fk_backward(hand, hp, idx, Rg, LT, ws, None, None, None, wrench, gRt, gR)
        return gp, None, None, None, None, None, None, None, None


def tabletop_terms(hand_pose, hand: HandHandle, samples: SurfaceSamples, idx, Rg, LT, ws, grasp_axis, table_z=0.0):
    """-> (E_prior (B), E_wall (B)) of core/energy.py:68-78 on ``samples``, unweighted, differentiable w.r.t. ``hand_pose``.
    ``idx``, ``Rg``, ``LT``, ``ws`` are the kinematic state of ``hand_pose`` (fk_contacts); ``table_z`` is the height of the
    table plane (0 in the reference)."""
    if not hand_pose.is_cuda:
        raise RuntimeError("graspqp_amd ops need CUDA (ROCm) tensors; got a CPU tensor")
    if samples.n_links != hand.L:
        raise ValueError(f"tabletop_terms: the samples refer to {samples.n_links} links, the hand has {hand.L}")
    return _TabletopTerms.apply(hand_pose, hand, samples, _c(idx, torch.int64), Rg.detach(), LT.detach(), ws,
                                _axis3(grasp_axis), float(table_z))


# ----------------------------------------------------------------------------------------------------------
# scene obstacles: E_scene on a signed-distance grid of the surroundings (csrc/scene.hip, include/graspqp_hip.h)
# ----------------------------------------------------------------------------------------------------------
_SCENE_CHUNK = 1 << 20  # nodes per set-up query of from_meshes / from_point_clouds


def _grid_struct(struct, values, origin, voxel):
    """gqSceneGrid of a (nx,ny,nz) tensor, or gqClutterGrids of a (G,nx,ny,nz) one: the same fields behind a leading n_grids."""
    g = struct()
    g.values = values.data_ptr()
    if struct is _C.ClutterGrids:
        g.n_grids, g.nx, g.ny, g.nz = (int(s) for s in values.shape)
    else:
        g.nx, g.ny, g.nz = (int(s) for s in values.shape)
    g.origin = (ctypes.c_float * 3)(*(float(o) for o in origin))
    g.voxel = float(voxel)
    return g


def _scene_grid(values, origin, voxel) -> "_C.SceneGrid":
    return _grid_struct(_C.SceneGrid, values, origin, voxel)


def _clutter_grids(values, origin, voxel) -> "_C.ClutterGrids":
    return _grid_struct(_C.ClutterGrids, values, origin, voxel)


def _grid_fields(stack, values, origin, device):
    """For SceneSDF and, with ``stack``, SceneSDFSet: ``values`` as the device tensor the grid struct points at (a CUDA float32
    contiguous tensor as it is, anything else converted once) and ``origin`` as 3 floats."""
    who, dims = ("SceneSDFSet", "(G,nx,ny,nz)") if stack else ("SceneSDF", "(nx,ny,nz)")
    v = values if torch.is_tensor(values) else torch.as_tensor(np.asarray(values, dtype=np.float32))
    if v.dim() != 3 + stack:
        raise ValueError(f"{who}: values must be {dims}, got {tuple(v.shape)}")
    origin = [float(o) for o in (origin.detach().cpu().tolist() if torch.is_tensor(origin) else origin)]
    if len(origin) != 3:
        raise ValueError(f"{who}: origin must have 3 entries, got {len(origin)}")
    if not (v.is_cuda and v.dtype == torch.float32 and v.is_contiguous()):
        v = v.detach().to(device, torch.float32).contiguous()
    return v, tuple(origin)


class SceneSDF:
    """A signed-distance grid of the hand's surroundings (an ESDF / TSDF volume): ``values`` (nx,ny,nz) float32 on the
    device, phi at the nodes in metres, POSITIVE OUTSIDE the obstacles; ``origin`` = world position of node (0,0,0);
    ``voxel`` = the node spacing of all axes.  A CUDA float32 contiguous tensor is used without a copy (anything else is
    converted once), so overwriting ``values`` in place moves the obstacles, also under a captured graph.  Between the nodes
    phi is the trilinear interpolant; outside the volume is free space (include/graspqp_hip.h)."""

    def __init__(self, values, origin, voxel, device="cuda"):
        v, origin = _grid_fields(False, values, origin, device)
        self.values, self.origin, self.voxel = v, origin, float(voxel)
        self.shape = tuple(int(s) for s in v.shape)
        self.grid = _scene_grid(v, self.origin, self.voxel)
        self.check()

    def check(self, batch=1, n_links=1, n_samples=1):
        """gq_scene_check (host only) of the grid and of a launch's shapes; raises ValueError with the library's message."""
        try:
            _C.call("gq_scene_check", ctypes.byref(self.grid), ctypes.c_int64(int(batch)), int(n_links), ctypes.c_int64(int(n_samples)))
        except RuntimeError as e:
            raise ValueError(f"SceneSDF: {e}") from None

    @staticmethod
    def _nodes(origin, shape, voxel, device):
        ax = [float(o) + float(voxel) * torch.arange(int(n), dtype=torch.float64, device=device) for o, n in zip(origin, shape)]
        return torch.stack(torch.meshgrid(*ax, indexing="ij"), -1).to(torch.float32)

    def node_positions(self):
        """World positions of the nodes, (nx,ny,nz,3) float32 on the device of ``values``."""
        return self._nodes(self.origin, self.shape, self.voxel, self.values.device)

    @classmethod
    def _filled(cls, query, n_obj, origin, shape, voxel, device):
        """phi = min over the objects of sign * sqrt(dist_sq) at the nodes, in chunks of at most 2^20 nodes."""
        pts = cls._nodes(origin, shape, voxel, device).reshape(-1, 3)
        phi = torch.full((pts.shape[0],), float("inf"), device=device)
        with torch.no_grad():
            for k in range(n_obj):
                for a in range(0, pts.shape[0], _SCENE_CHUNK):
                    d2, sgn = query(k, pts[a:a + _SCENE_CHUNK])
                    phi[a:a + _SCENE_CHUNK] = torch.minimum(phi[a:a + _SCENE_CHUNK], sgn.to(torch.float32) * d2.sqrt())
        return cls(phi.reshape(tuple(int(n) for n in shape)), origin, voxel, device)

    @classmethod
    def from_meshes(cls, face_verts_list, origin, shape, voxel, device="cuda"):
        """The grid of the union of triangle meshes (each (F,3,3)): phi = min over the meshes of sign * sqrt(dist_sq) of
        ``compute_sdf`` at the node positions.  Set-up code.  A mesh must be CLOSED for its sign to mean anything: the sign is
        that of the nearest face's side, which for an open sheet flips across the sheet's plane far from it."""
        fvs = [torch.as_tensor(np.asarray(f.detach().cpu() if torch.is_tensor(f) else f, dtype=np.float32).reshape(-1, 3, 3)).to(device)
               for f in face_verts_list]
        return cls._filled(lambda k, p: compute_sdf(p, fvs[k])[:2], len(fvs), origin, shape, voxel, device)

    @classmethod
    def from_point_clouds(cls, points_list, normals_list, origin, shape, voxel, radius=None, device="cuda"):
        """The same from oriented point clouds (``PointCloudSet`` / ``sdf_cloud``, the surfel signed distance of DESIGN 13);
        a cloud must sample a CLOSED surface with outward normals for its sign to mean anything."""
        n = len(points_list)
        rad = [None] * n if radius is None else [float(radius)] * n if np.ndim(radius) == 0 else [float(r) for r in radius]
        if len(rad) != n or len(normals_list) != n:
            raise ValueError(f"SceneSDF.from_point_clouds: {n} clouds, {len(normals_list)} normal sets, {len(rad)} radii")
        sets = [PointCloudSet([p], [nr], r, device) for p, nr, r in zip(points_list, normals_list, rad)]
        return cls._filled(lambda k, p: sdf_cloud(p, sets[k], p.shape[0])[:2], len(sets), origin, shape, voxel, device)


class SceneSDFSet:
    """A stack of scene grids, one per object (include/graspqp_hip.h, "clutter scenes"): ``values`` (G,nx,ny,nz) float32 on the
    device, grid g in the frame of object g; ``origin`` and ``voxel`` are shared by all grids.  A CUDA float32 contiguous
    tensor is used without a copy, so ``scene_compose`` or an in-place write moves the obstacles, also under a captured graph.
    Rows are object-major: of B rows, row b reads grid b // (B / G)."""

    def __init__(self, values, origin, voxel, device="cuda"):
        v, origin = _grid_fields(True, values, origin, device)
        self.values, self.origin, self.voxel = v, origin, float(voxel)
        self.n_grids, self.shape = int(v.shape[0]), tuple(int(s) for s in v.shape[1:])
        self.grid_set = _clutter_grids(v, self.origin, self.voxel)
        self.check(self.n_grids, 1)

    @classmethod
    def empty(cls, n_grids, origin, shape, voxel, device="cuda"):
        """An uninitialised stack for ``scene_compose`` to fill."""
        return cls(torch.empty((int(n_grids),) + tuple(int(n) for n in shape), dtype=torch.float32, device=device), origin, voxel, device)

    def check(self, batch, rows_per_grid, n_links=1, n_samples=1):
        """gq_clutter_check (host only) of the stack and of a launch's shapes; raises ValueError with the library's message."""
        try:
            _C.call("gq_clutter_check", ctypes.byref(self.grid_set), ctypes.c_int64(int(batch)), int(rows_per_grid), int(n_links),
                    ctypes.c_int64(int(n_samples)))
        except RuntimeError as e:
            raise ValueError(f"SceneSDFSet: {e}") from None

    def rows_per_grid(self, batch, what="batch"):
        if batch % self.n_grids:
            raise ValueError(f"SceneSDFSet: {what} = {batch} is not divisible by n_grids = {self.n_grids}")
        return batch // self.n_grids

    def scene(self, g) -> "SceneSDF":
        """Grid ``g`` as an ``ops.SceneSDF`` that shares the stack's memory."""
        return SceneSDF(self.values[int(g)], self.origin, self.voxel)


def scene_compose(out: SceneSDFSet, target_T, parts, part_T, exclude=None, base=None, far=1.0):
    """Fills ``out`` in place on the device (gq_clutter_compose) and returns it: node (g,i,j,k) = min(``far``, ``base`` at the
    node's world position, every part but ``exclude[g]`` at its part-frame position), the node being placed in the world by
    ``target_T[g]``.  ``parts``: a sequence of ``SceneSDF``, each in its own part frame; ``target_T`` (G,3,4) or (G,12) and
    ``part_T`` (n_parts,3,4) or (n_parts,12): world_from_frame [R|t], float32 CUDA (contiguous float32 CUDA tensors are read
    in place at launch, so the call can be captured in a graph and replayed after a pose update); ``exclude`` (G) int32 or
    None; ``base``: a ``SceneSDF`` in the world frame or None.  No allocation, no synchronisation."""
    parts = list(parts)
    dev = out.values.device

    def poses(T, n, name):
        if T is None:
            T = torch.zeros(0, 12)
        T = T if torch.is_tensor(T) else torch.as_tensor(np.asarray(T, dtype=np.float32))
        T = _c(T.to(dev)).reshape(-1, 12) if T.numel() else T.to(dev, torch.float32).reshape(0, 12)
        if T.shape[0] != n:
            raise ValueError(f"scene_compose: {name} must hold {n} poses of 12 floats, got {tuple(T.shape)}")
        return T

    tT, pT = poses(target_T, out.n_grids, "target_T"), poses(part_T, len(parts), "part_T")
    ex = None
    if exclude is not None:
        ex = _c(exclude.to(dev), torch.int32)
        if ex.shape != (out.n_grids,):
            raise ValueError(f"scene_compose: exclude must be ({out.n_grids},), got {tuple(ex.shape)}")
    arr = (_C.SceneGrid * max(len(parts), 1))(*(p.grid for p in parts))
    try:
        _C.call("gq_clutter_compose_check", ctypes.byref(out.grid_set), ctypes.cast(arr, ctypes.c_void_p), len(parts),
                ctypes.byref(base.grid) if base is not None else None, float(far))
    except RuntimeError as e:
        raise ValueError(f"scene_compose: {e}") from None
    _Eager.scene_compose(out.values, list(out.origin), out.voxel, tT, [p.values for p in parts],
                         [float(o) for p in parts for o in p.origin], [p.voxel for p in parts], pT, ex,
                         None if base is None else base.values, [0.0, 0.0, 0.0] if base is None else list(base.origin),
                         0.0 if base is None else base.voxel, float(far))
    return out


def _depth_views(depth, labels, cam_T, intrinsics, depth_range) -> "_C.DepthViews":
    v = _C.DepthViews()
    v.depth, v.labels, v.cam_T = depth.data_ptr(), (labels.data_ptr() if labels is not None else None), cam_T.data_ptr()
    v.n_views, v.height, v.width = (int(s) for s in depth.shape)
    v.fx, v.fy, v.cx, v.cy = (float(x) for x in intrinsics)
    v.depth_min, v.depth_max = (float(x) for x in depth_range)
    return v


class SceneTSDF:
    """A scene volume fused from depth images on the device (include/graspqp_hip.h, "scenes from depth images").

    ``.scene`` is an ``ops.SceneSDF`` (``n_grids`` None: one grid in the world frame) or an ``ops.SceneSDFSet`` (``n_grids``
    grids, grid g in the frame of object g) over ``shape`` nodes at ``voxel`` spacing from ``origin``; it goes wherever a scene
    goes (``GraspStepper(scene=...)``, ``HandModel.set_scene``, the ``base`` of ``scene_compose``) and shares ``.values``, the
    running truncated signed distance in metres, positive in seen free space, clamped to +-``trunc``.  ``.weight`` is the number
    of views that updated each node, capped at ``max_weight``.  ``integrate`` writes both in place with one launch per batch of
    frames, so a stepper's captured graph reads the new volume at its next replay.

    ``unknown`` is the value of a node no view has updated.  The default ``-trunc`` makes unobserved space OCCUPIED: the
    conservative choice for a hand that must stay in seen free space (occluded regions, the space behind surfaces and outside
    every frustum push the hand out).  ``+trunc`` makes unobserved space FREE instead: only surfaces that were actually seen are
    obstacles, and the hand may enter space no camera has looked at.

    The distance is truncated: ``E_scene`` / ``E_approach`` are hinges at ``scene_margin``, and a margin at or above ``trunc``
    would be active everywhere in free space -- keep ``scene_margin`` below ``trunc``, or run the stepper on ``esdf(max_distance)``,
    the Euclidean distance field of the volume, which also has a gradient deep inside obstacles.  With a skipped label (``skip``), every
    ray through the target's pixels is taken as free in that grid, so a table hidden under the target is carved away with it:
    keep the table by ``E_wall`` or by a second view that sees it beside the target."""

    def __init__(self, origin, shape, voxel, trunc, n_grids=None, unknown=None, max_weight=64.0, device="cuda"):
        self.trunc, self.max_weight = float(trunc), float(max_weight)
        self.unknown = -self.trunc if unknown is None else float(unknown)
        fin = lambda v: abs(v) < float("inf")  # False for a NaN
        if not (fin(self.trunc) and self.trunc > 0.0):
            raise ValueError(f"SceneTSDF: trunc must be finite and > 0, got {trunc!r}")
        if not (fin(self.max_weight) and self.max_weight >= 1.0):
            raise ValueError(f"SceneTSDF: max_weight must be finite and >= 1, got {max_weight!r}")
        if not fin(self.unknown):
            raise ValueError(f"SceneTSDF: unknown must be finite, got {unknown!r}")
        G = 1 if n_grids is None else int(n_grids)
        self._stack = torch.empty((G,) + tuple(int(n) for n in shape), dtype=torch.float32, device=device)
        self.weight = torch.empty_like(self._stack) if n_grids is not None else torch.empty_like(self._stack)[0]
        self.scene = SceneSDFSet(self._stack, origin, voxel, device) if n_grids is not None else SceneSDF(self._stack[0], origin, voxel, device)
        self.values, self.origin, self.voxel = self.scene.values, self.scene.origin, self.scene.voxel
        self.n_grids, self.shape = G, tuple(self._stack.shape[1:])
        self._weight = self.weight.view(self._stack.shape)
        self._grids = _clutter_grids(self._stack, self.origin, self.voxel)
        self.reset()

    def reset(self):
        """A fresh volume: ``values = unknown``, ``weight = 0`` (two fills, no synchronisation)."""
        self._stack.fill_(self.unknown)
        self._weight.zero_()
        return self

    def integrate(self, depth, intrinsics, cam_T, labels=None, target_T=None, skip=None, depth_range=(0.05, 5.0)):
        """Fuses depth frames into the volume in place (gq_tsdf_integrate, one launch) and returns ``self``.  ``depth`` (H,W) or
        (V,H,W): metres along the optical axis; ``intrinsics`` = (fx, fy, cx, cy) of the pinhole, pixel centres at integer
        (col,row); ``cam_T`` (V,12) or (V,3,4): world_from_camera [R|t]; ``labels`` like ``depth``, int32: a segmentation id per
        pixel; ``target_T`` (G,12) or (G,3,4): world_from_frame of every grid, None = the grids' frame is the world; ``skip`` (G)
        int32: the label grid g takes as free space (its own target), negative = none; ``depth_range`` = (depth_min, depth_max),
        a pixel outside it is no measurement.  Contiguous float32 / int32 CUDA tensors are read in place at launch, so the call
        can be captured in a graph and replayed after the images, poses or ``skip`` were overwritten.  No allocation, no
        synchronisation.  Views are fused in ascending order; V views in one call give the bits of V calls."""
        dev = self._stack.device

        def tensor(t, dtype):
            t = t if torch.is_tensor(t) else torch.as_tensor(np.asarray(t))
            return _c(t.to(dev), dtype)

        d = tensor(depth, torch.float32)
        d = d[None] if d.dim() == 2 else d
        if d.dim() != 3:
            raise ValueError(f"SceneTSDF.integrate: depth must be (H,W) or (V,H,W), got {tuple(d.shape)}")
        V = int(d.shape[0])
        lab = None
        if labels is not None:
            lab = tensor(labels, torch.int32)
            lab = lab[None] if lab.dim() == 2 else lab
            if lab.shape != d.shape:
                raise ValueError(f"SceneTSDF.integrate: labels must have depth's shape {tuple(d.shape)}, got {tuple(lab.shape)}")

        def poses(T, n, name):
            T = tensor(T, torch.float32)
            if T.numel() != 12 * n:
                raise ValueError(f"SceneTSDF.integrate: {name} must hold {n} poses of 12 floats, got {tuple(T.shape)}")
            return T.reshape(n, 12)

        cT = poses(cam_T, V, "cam_T")
        tT = None if target_T is None else poses(target_T, self.n_grids, "target_T")
        sk = None
        if skip is not None:
            sk = tensor(skip, torch.int32)
            if sk.shape != (self.n_grids,):
                raise ValueError(f"SceneTSDF.integrate: skip must be ({self.n_grids},), got {tuple(sk.shape)}")
        intrinsics, depth_range = [float(x) for x in intrinsics], [float(x) for x in depth_range]
        if len(intrinsics) != 4 or len(depth_range) != 2:
            raise ValueError("SceneTSDF.integrate: intrinsics must be (fx, fy, cx, cy) and depth_range (depth_min, depth_max)")
        views = _depth_views(d, lab, cT, intrinsics, depth_range)
        try:
            _C.call("gq_tsdf_check", ctypes.byref(self._grids), ctypes.byref(views), self.trunc, self.max_weight, self.unknown)
        except RuntimeError as e:
            raise ValueError(f"SceneTSDF.integrate: {e}") from None
        _Eager.tsdf_integrate(self._stack, self._weight, list(self.origin), self.voxel, d, lab, cT, intrinsics, depth_range, tT, sk,
                              self.trunc, self.max_weight)
        return self

    def _region(self, bounds):
        """The half-open node region [i0,i1,j0,j1,k0,k1] of the nodes inside ``bounds`` = (lo, hi), two points of the grid frame."""
        if bounds is None:
            return []
        lo, hi = (np.asarray(b, dtype=np.float64).reshape(3) for b in bounds)
        region = []
        for a in range(3):
            u0, u1 = (lo[a] - self.origin[a]) / self.voxel, (hi[a] - self.origin[a]) / self.voxel
            if not (abs(u0) < float("inf") and abs(u1) < float("inf")):
                raise ValueError(f"SceneTSDF.surfels: bounds must be finite, got {bounds!r}")
            i0, i1 = max(int(np.ceil(u0 - 1e-6)), 0), min(int(np.floor(u1 + 1e-6)) + 1, self.shape[a])
            if i0 >= i1:
                raise ValueError(f"SceneTSDF.surfels: bounds {bounds!r} hold no node of the grid on axis {a}")
            region += [i0, i1]
        return region

    def surfels(self, capacity, min_weight=1.0, bounds=None, out=None):
        """The zero level set of every grid as an oriented point cloud (gq_tsdf_surfels, three launches): -> ``(points
        (G,capacity,3), normals (G,capacity,3), count (G,2) int32)`` on the device, in the grid's frame.  A surfel sits where D
        changes sign along a grid edge whose two nodes carry ``weight >= min_weight`` and |D| < ``trunc``; its normal is the
        normalised smoothed gradient of D (outward: D is positive in free space).  ``count[g] = (found, written)`` with
        ``written = min(found, capacity)``; rows at and beyond ``written`` are not touched.  ``bounds`` = (lo, hi), two points of
        the grid frame: only edges between nodes inside that box.  ``out`` = an earlier result, whose buffers are written again.
        No synchronisation, and with ``out`` no allocation: the call can be captured in a graph behind ``integrate``.  The order
        of the surfels is fixed (tile, node, axis), so two calls agree bit for bit.  With ``min_weight=2`` only surfaces two views
        agree on remain, which trims the silhouette tails of a projective TSDF: on the sphere check of DESIGN 18 the radial error
        falls from median 0.41 mm / max 0.67 voxel to 0.28 mm / 0.63 voxel."""
        capacity = int(capacity)
        region = self._region(bounds)
        self._surfels_check(region, min_weight, True, capacity)
        dev, G = self._stack.device, self.n_grids
        if out is None:
            out = (torch.empty(G, capacity, 3, device=dev), torch.empty(G, capacity, 3, device=dev),
                   torch.empty(G, 2, dtype=torch.int32, device=dev))
        P, N, count = out
        if not (tuple(P.shape) == tuple(N.shape) == (G, capacity, 3) and tuple(count.shape) == (G, 2)):
            raise ValueError(f"SceneTSDF.surfels: out must be ((G,capacity,3), (G,capacity,3), (G,2)) with G = {G}, capacity = {capacity}")
        _Eager.tsdf_surfels(self._stack, self._weight, list(self.origin), self.voxel, region, float(min_weight), self.trunc, P, N, count,
                            self._surfel_workspace())
        return P, N, count

    def _surfels_check(self, region, min_weight, has_outputs, capacity):
        reg = (ctypes.c_int32 * 6)(*region) if region else None
        try:
            _C.call("gq_tsdf_surfels_check", ctypes.byref(self._grids), reg, float(min_weight), self.trunc, int(has_outputs),
                    ctypes.c_int64(capacity))
        except RuntimeError as e:
            raise ValueError(f"SceneTSDF.surfels: {e}") from None

    def _surfel_workspace(self):
        if getattr(self, "_surfel_ws", None) is None:
            self._surfel_ws = _ws(_size_call("gq_tsdf_surfels_workspace_bytes", ctypes.byref(self._grids)), self._stack.device)
        return self._surfel_ws

    def extract_clouds(self, min_weight=1.0, bounds=None):
        """-> a list of G ``(points (n_g,3), normals (n_g,3))`` pairs on the device, every grid's surfels trimmed to their number: a
        counting call, ONE read of ``count`` on the host (the only synchronisation), then a call of exactly the largest size."""
        region = self._region(bounds)
        self._surfels_check(region, min_weight, False, 0)
        count = torch.empty(self.n_grids, 2, dtype=torch.int32, device=self._stack.device)
        _Eager.tsdf_surfels(self._stack, self._weight, list(self.origin), self.voxel, region, float(min_weight), self.trunc, None, None,
                            count, self._surfel_workspace())
        found = count[:, 0].cpu().tolist()
        P, N, _ = self.surfels(max(max(found), 1), min_weight, bounds)
        return [(P[g, :n], N[g, :n]) for g, n in enumerate(found)]

    def esdf(self, max_distance, out=None):
        """The Euclidean distance field of the volume (gq_esdf, eight launches): -> a scene of the kind of ``.scene``
        with the same geometry, which goes wherever a scene goes.  Outside the band it holds the signed distance to the zero
        crossings of the volume, up to +-``max_distance``: it has a gradient deep inside obstacles and unobserved space, where
        the fused value is flat, and ``scene_margin`` / ``approach_margin`` may now go up to ``max_distance`` instead of staying
        below ``trunc``.  Inside the band (|D| < ``trunc``) the values remain the fused ones, bit for bit, and so remain
        projective.  A grid knows only its own crossings: near the grid's border the distance to a surface outside it is
        overestimated.  The volume is not written.  The output scene and the workspace are made at the first call, owned by the
        volume and returned on every call (``out``: a scene of the same kind and geometry to write instead); after that no
        allocation and no synchronisation, so the call can be captured in a graph behind ``integrate`` and a stepper built on
        the returned scene reads the new field at its next replay."""
        if out is None:
            if getattr(self, "_esdf_scene", None) is None:
                v = torch.empty_like(self._stack)
                self._esdf_scene = (SceneSDFSet(v, self.origin, self.voxel, v.device) if isinstance(self.scene, SceneSDFSet)
                                    else SceneSDF(v[0], self.origin, self.voxel, v.device))
            out = self._esdf_scene
        try:
            return scene_esdf(self.scene, self.trunc, max_distance, out)
        except ValueError as e:
            raise ValueError(f"SceneTSDF.esdf: {e}") from None


def scene_esdf(src, trunc, max_distance, out=None):
    """The Euclidean distance field of a TSDF (gq_esdf, eight launches; include/graspqp_hip.h): ``src`` is an
    ``ops.SceneSDF`` or an ``ops.SceneSDFSet`` whose values are a truncated signed distance, positive in free space, clamped to
    +-``trunc`` (a ``SceneTSDF``'s ``.scene``, or the TSDF of a perception stack); -> a scene of the same kind and geometry.  A
    node with |D| < ``trunc`` keeps D bit for bit, a non-finite node too; every other node gets the signed distance to the
    nearest zero crossing of its grid along the grid edges' crossing points, held to [``trunc``, ``max_distance``], with the
    sign of D.  ``src`` is not written.  ``out``: a scene of the same kind and geometry to write (not ``src``); it keeps the
    workspace of its first call, so a further call with ``out`` allocates nothing and does not synchronise."""
    if not isinstance(src, (SceneSDF, SceneSDFSet)):
        raise ValueError(f"scene_esdf: src must be an ops.SceneSDF or an ops.SceneSDFSet, got {type(src).__name__}")
    single = isinstance(src, SceneSDF)
    stack = lambda s: s.values[None] if single else s.values
    sg = _clutter_grids(stack(src), src.origin, src.voxel)
    try:
        need = _size_call("gq_esdf_workspace_bytes", ctypes.byref(sg))
    except RuntimeError as e:
        raise ValueError(f"scene_esdf: {e}") from None
    if out is None:
        v = torch.empty_like(src.values)
        out = SceneSDF(v, src.origin, src.voxel, v.device) if single else SceneSDFSet(v, src.origin, src.voxel, v.device)
    if type(out) is not type(src):
        raise ValueError(f"scene_esdf: out must be an ops.{type(src).__name__} like src, got {type(out).__name__}")
    ws = getattr(out, "_esdf_ws", None)
    if ws is None or ws.numel() < need or ws.device != out.values.device:
        ws = out._esdf_ws = _ws(need, out.values.device)
    dg = _clutter_grids(stack(out), out.origin, out.voxel)
    try:
        _C.call("gq_esdf_check", ctypes.byref(sg), ctypes.byref(dg), float(trunc), float(max_distance), ctypes.c_void_p(ws.data_ptr()))
    except RuntimeError as e:
        raise ValueError(f"scene_esdf: {e}") from None
    _Eager.scene_esdf(stack(src), list(src.origin), src.voxel, float(trunc), float(max_distance), stack(out), ws)
    return out


def keep_label(depth, labels, label):
    """``depth`` with 0 (no measurement) wherever the pixel's label differs from ``label``: frames masked this way fuse into a
    volume that holds the labelled object alone (``SceneTSDF.integrate`` ignores a pixel outside ``depth_range``)."""
    depth = depth if torch.is_tensor(depth) else torch.as_tensor(np.asarray(depth))
    labels = labels if torch.is_tensor(labels) else torch.as_tensor(np.asarray(labels))
    if depth.shape != labels.shape:
        raise ValueError(f"keep_label: labels must have depth's shape {tuple(depth.shape)}, got {tuple(labels.shape)}")
    return torch.where(labels.to(depth.device) == int(label), depth, torch.zeros((), dtype=depth.dtype, device=depth.device))


def _scene_call(grid, margin, hp, points, link, n_links, Rg, LT, up_scene, w_scene, e_scene, accumulate, wrench, gRt, st=None):
    p, (B, D) = _dev, hp.shape
    entry, rows = "gq_scene_terms", ()
    if isinstance(grid, _C.ClutterGrids):  # a stack: rows_per_grid follows the struct, row b reads grid b // (B / G)
        entry, rows = "gq_clutter_terms", (B // max(grid.n_grids, 1),)
    _C.call(entry, ctypes.byref(grid), *rows, float(margin), _C.f32(points), p(link, torch.int32), points.shape[0], int(n_links),
            _C.f32(hp), D, p(Rg), p(LT), B, p(up_scene), float(w_scene), p(e_scene), int(accumulate), p(wrench), p(gRt),
            _C.stream_ptr() if st is None else st)


def _scene_query_call(grid, flat, phi, grad, inside):
    N = flat.shape[0]
    if isinstance(grid, _C.ClutterGrids):  # a stack: point i reads grid i // (N / G)
        _C.call("gq_clutter_query", ctypes.byref(grid), _C.f32(flat), ctypes.c_int64(N), ctypes.c_int64(N // max(grid.n_grids, 1)),
                _C.f32(phi), _C.f32(grad), _C.u8(inside), _C.stream_ptr())
        return
    _C.call("gq_scene_query", ctypes.byref(grid), _C.f32(flat), ctypes.c_int64(N), _C.f32(phi), _C.f32(grad), _C.u8(inside),
            _C.stream_ptr())


def _scene_distance_setup(ctx, inputs, output):
    ctx.save_for_backward(output[1])
    ctx.mark_non_differentiable(output[1], output[2])


def _scene_distance_bwd(ctx, g_phi, g_grad, g_inside):
    (grad,) = ctx.saved_tensors
    return grad * g_phi.unsqueeze(-1), None, None, None


def scene_distance(points, scene: SceneSDF):
    """phi (...) of the scene's grid at world points (...,3): the trilinear interpolant, +inf outside the volume (free
    space).  Differentiable w.r.t. ``points``: the backward is grad phi * upstream, zero outside the volume."""
    if not points.is_cuda:
        raise RuntimeError("graspqp_amd ops need CUDA (ROCm) tensors; got a CPU tensor")
    if points.dim() < 1 or points.shape[-1] != 3:
        raise ValueError(f"scene_distance: points must be (...,3), got {tuple(points.shape)}")
    if isinstance(scene, SceneSDFSet):  # points (B,...,3), B divisible by G: row b reads grid b // (B / G)
        if points.dim() < 2:
            raise ValueError(f"scene_distance: with a SceneSDFSet points must be (B,...,3), got {tuple(points.shape)}")
        scene.rows_per_grid(points.shape[0], "the points' leading dimension")
        return _Eager.scene_distance_set(points, scene.values, list(scene.origin), scene.voxel)[0]
    return _Eager.scene_distance(points, scene.values, list(scene.origin), scene.voxel)[0]


class _SceneTerms(torch.autograd.Function):
    """Glue between two registered ops (scene_terms + fk_backward), as _TabletopTerms."""

    @staticmethod
    def forward(ctx, hand_pose, hand, samples, idx, Rg, LT, ws, scene, margin):
        hp = _c(hand_pose.detach())
        ctx.is_set = isinstance(scene, SceneSDFSet)
        fwd = _Eager.scene_terms_set if ctx.is_set else _Eager.scene_terms
        e = fwd(hp, samples.points, samples.link, hand.L, Rg, LT, scene.values, list(scene.origin), scene.voxel, margin)
        ctx.save_for_backward(hp, idx, Rg, LT, ws, samples.points, samples.link, scene.values)
        ctx.hand, ctx.origin, ctx.voxel, ctx.margin = hand, list(scene.origin), scene.voxel, margin
        return e

    @staticmethod
    def backward(ctx, g_scene):
        hp, idx, Rg, LT, ws, points, link, values = ctx.saved_tensors
        hand = ctx.hand
        bwd = _Eager.scene_terms_set_backward if ctx.is_set else _Eager.scene_terms_backward
        wrench, gRt = bwd(hp, points, link, hand.L, Rg, LT, values, ctx.origin, ctx.voxel, ctx.margin, g_scene)
        gp = _fk_backward(hand, hp, idx, Rg, LT, ws, None, None, None, wrench, gRt, None)
        return gp, None, None, None, None, None, None, None, None


def scene_terms(hand_pose, hand: HandHandle, samples: SurfaceSamples, idx, Rg, LT, ws, scene: SceneSDF, margin=0.0):
    """-> E_scene (B) = sum over ``samples`` of max(margin - phi(x_w), 0) on the scene's grid, unweighted, differentiable
    w.r.t. ``hand_pose``.  ``idx``, ``Rg``, ``LT``, ``ws`` are the kinematic state of ``hand_pose`` (fk_contacts); ``margin``
    >= 0 is a clearance in metres."""
    if not hand_pose.is_cuda:
        raise RuntimeError("graspqp_amd ops need CUDA (ROCm) tensors; got a CPU tensor")
    if samples.n_links != hand.L:
        raise ValueError(f"scene_terms: the samples refer to {samples.n_links} links, the hand has {hand.L}")
    if not float(margin) >= 0.0:
        raise ValueError(f"scene_terms: margin = {margin!r} must be >= 0")
    if isinstance(scene, SceneSDFSet):
        scene.check(hand_pose.shape[0], scene.rows_per_grid(hand_pose.shape[0]), hand.L, samples.Ns)
    return _SceneTerms.apply(hand_pose, hand, samples, _c(idx, torch.int64), Rg.detach(), LT.detach(), ws, scene, float(margin))


# ----------------------------------------------------------------------------------------------------------
# approach clearance: E_approach, the scene grid along the hand's approach corridor (csrc/approach.hip)
# ----------------------------------------------------------------------------------------------------------
def approach_check(scene: SceneSDF, batch, n_links, n_samples, distance, stations, grasp_axis):
    """gq_approach_check (host only) of the grid, a launch's shapes and the corridor; raises ValueError with the library's
    message."""
    ax = _axis_c(grasp_axis)
    if isinstance(scene, SceneSDFSet):  # the stack's own check, then the corridor's on one of its grids
        scene.check(batch, scene.rows_per_grid(int(batch)), n_links, n_samples)
        scene = scene.scene(0)
    try:
        _C.call("gq_approach_check", ctypes.byref(scene.grid), ctypes.c_int64(int(batch)), int(n_links),
                ctypes.c_int64(int(n_samples)), float(distance), int(stations), ctypes.cast(ax, ctypes.c_void_p))
    except RuntimeError as e:
        raise ValueError(f"approach: {e}") from None


def _approach_call(grid, margin, distance, stations, hp, points, link, n_links, Rg, LT, axis, up_approach, w_approach, e_approach,
                   accumulate, wrench, gRt, st=None):
    p, (B, D) = _dev, hp.shape
    entry, rows = "gq_approach_terms", ()
    if isinstance(grid, _C.ClutterGrids):  # a stack: rows_per_grid follows the struct, row b reads grid b // (B / G)
        entry, rows = "gq_clutter_corridor_terms", (B // max(grid.n_grids, 1),)
    _C.call(entry, ctypes.byref(grid), *rows, float(margin), float(distance), int(stations), _C.f32(points), p(link, torch.int32),
            points.shape[0], int(n_links), _C.f32(hp), D, p(Rg), p(LT), B, _axis_c(axis), p(up_approach), float(w_approach),
            p(e_approach), int(accumulate), p(wrench), p(gRt), _C.stream_ptr() if st is None else st)


def _grid_ops(sfx, mk_grid):
    """The registered ops that read a signed-distance grid, for one kind of grid: ``mk_grid`` = _scene_grid and ``sfx`` = "" for a
    single grid, ``values`` (nx,ny,nz); _clutter_grids and "_set" for a stack of G grids, one per object (csrc/clutter.hip): the
    stack crosses the dispatcher as ``values`` (G,nx,ny,nz), and row b of B reads grid b // (B / G).  The two kinds share the
    schemas, the bodies and the fakes; the launches are picked by the grid struct (_scene_query_call, _scene_call,
    _approach_call).  -> the five op definitions."""

    @_custom_op(f"graspqp_amd::scene_distance{sfx}", mutates_args=(), device_types="cuda")
    def distance_op(points: Tensor, values: Tensor, origin: List[float], voxel: float) -> Tuple[Tensor, Tensor, Tensor]:
        """-> (phi (...), grad phi (...,3), inside (...) uint8) of the grid at world points (...,3); outside the volume
        phi = +inf, grad = 0, inside = 0.  A stack takes points (B,...,3), B divisible by G."""
        pts, v = _c(points), _c(values)
        flat = pts.reshape(-1, 3)
        N, dev = flat.shape[0], pts.device
        phi, grad, inside = torch.empty(N, device=dev), torch.empty(N, 3, device=dev), torch.empty(N, dtype=torch.uint8, device=dev)
        _scene_query_call(mk_grid(v, origin, voxel), flat, phi, grad, inside)
        return phi.reshape(pts.shape[:-1]), grad.reshape(pts.shape), inside.reshape(pts.shape[:-1])

    @distance_op.register_fake
    def _(points, values, origin, voxel):
        return (points.new_empty(points.shape[:-1]), points.new_empty(points.shape),
                points.new_empty(points.shape[:-1], dtype=torch.uint8))

    torch.library.register_autograd(f"graspqp_amd::scene_distance{sfx}", _scene_distance_bwd, setup_context=_scene_distance_setup)

    @_custom_op(f"graspqp_amd::scene_terms{sfx}", mutates_args=(), device_types="cuda")
    def scene_op(hand_pose: Tensor, points: Tensor, link: Tensor, n_links: int, Rg: Tensor, LT: Tensor, values: Tensor,
                 origin: List[float], voxel: float, margin: float) -> Tensor:
        """-> E_scene (B), unweighted: sum over the hand's surface samples of max(margin - phi, 0).  The kinematic state (Rg,
        link_T) is the one of ``hand_pose``, passed in detached, as for hand_pen."""
        hp, v = _c(hand_pose), _c(values)
        e = torch.empty(hp.shape[0], device=hp.device)
        _scene_call(mk_grid(v, origin, voxel), margin, hp, _c(points), _c(link, torch.int32), n_links, _c(Rg), _c(LT), None, 0.0,
                    e, 0, None, None)
        return e

    @scene_op.register_fake
    def _(hand_pose, points, link, n_links, Rg, LT, values, origin, voxel, margin):
        return hand_pose.new_empty(hand_pose.shape[0])

    @_custom_op(f"graspqp_amd::scene_terms{sfx}_backward", mutates_args=(), device_types="cuda")
    def scene_bwd_op(hand_pose: Tensor, points: Tensor, link: Tensor, n_links: int, Rg: Tensor, LT: Tensor, values: Tensor,
                     origin: List[float], voxel: float, margin: float, g_scene: Tensor) -> Tuple[Tensor, Tensor]:
        """Upstream row gradients (B) on E_scene -> (link wrench (B,L,6), gRt (B,12)) for fk_backward."""
        hp, v = _c(hand_pose), _c(values)
        B, dev = hp.shape[0], hp.device
        wrench, gRt = torch.empty(B, n_links, 6, device=dev), torch.empty(B, 12, device=dev)
        _scene_call(mk_grid(v, origin, voxel), margin, hp, _c(points), _c(link, torch.int32), n_links, _c(Rg), _c(LT),
                    _c(g_scene), 0.0, None, 0, wrench, gRt)
        return wrench, gRt

    @scene_bwd_op.register_fake
    def _(hand_pose, points, link, n_links, Rg, LT, values, origin, voxel, margin, g_scene):
        B = hand_pose.shape[0]
        return hand_pose.new_empty(B, n_links, 6), hand_pose.new_empty(B, 12)

    @_custom_op(f"graspqp_amd::approach_terms{sfx}", mutates_args=(), device_types="cuda")
    def approach_op(hand_pose: Tensor, points: Tensor, link: Tensor, n_links: int, Rg: Tensor, LT: Tensor, values: Tensor,
                    origin: List[float], voxel: float, grasp_axis: List[float], distance: float, stations: int,
                    margin: float) -> Tensor:
        """-> E_approach (B), unweighted: the mean over the stations d_k = distance k / stations of the hinge sum of the hand's
        surface samples moved back by d_k along grasp_axis.  The kinematic state (Rg, link_T) is the one of ``hand_pose``."""
        hp, v = _c(hand_pose), _c(values)
        e = torch.empty(hp.shape[0], device=hp.device)
        _approach_call(mk_grid(v, origin, voxel), margin, distance, stations, hp, _c(points), _c(link, torch.int32), n_links,
                       _c(Rg), _c(LT), grasp_axis, None, 0.0, e, 0, None, None)
        return e

    @approach_op.register_fake
    def _(hand_pose, points, link, n_links, Rg, LT, values, origin, voxel, grasp_axis, distance, stations, margin):
        return hand_pose.new_empty(hand_pose.shape[0])

    @_custom_op(f"graspqp_amd::approach_terms{sfx}_backward", mutates_args=(), device_types="cuda")
    def approach_bwd_op(hand_pose: Tensor, points: Tensor, link: Tensor, n_links: int, Rg: Tensor, LT: Tensor, values: Tensor,
                        origin: List[float], voxel: float, grasp_axis: List[float], distance: float, stations: int, margin: float,
                        g_approach: Tensor) -> Tuple[Tensor, Tensor]:
        """Upstream row gradients (B) on E_approach -> (link wrench (B,L,6), gRt (B,12)) for fk_backward."""
        hp, v = _c(hand_pose), _c(values)
        B, dev = hp.shape[0], hp.device
        wrench, gRt = torch.empty(B, n_links, 6, device=dev), torch.empty(B, 12, device=dev)
        _approach_call(mk_grid(v, origin, voxel), margin, distance, stations, hp, _c(points), _c(link, torch.int32), n_links,
                       _c(Rg), _c(LT), grasp_axis, _c(g_approach), 0.0, None, 0, wrench, gRt)
        return wrench, gRt

    @approach_bwd_op.register_fake
    def _(hand_pose, points, link, n_links, Rg, LT, values, origin, voxel, grasp_axis, distance, stations, margin, g_approach):
        B = hand_pose.shape[0]
        return hand_pose.new_empty(B, n_links, 6), hand_pose.new_empty(B, 12)

    return distance_op, scene_op, scene_bwd_op, approach_op, approach_bwd_op


_scene_distance_op, _scene_op, _scene_bwd_op, _approach_op, _approach_bwd_op = _grid_ops("", _scene_grid)
_scene_distance_set_op, _scene_set_op, _scene_set_bwd_op, _approach_set_op, _approach_set_bwd_op = _grid_ops("_set", _clutter_grids)


class _ApproachTerms(torch.autograd.Function):
    """Glue between two registered ops (approach_terms + fk_backward), as _SceneTerms."""

    @staticmethod
    def forward(ctx, hand_pose, hand, samples, idx, Rg, LT, ws, scene, axis, distance, stations, margin):
        hp = _c(hand_pose.detach())
        ctx.is_set = isinstance(scene, SceneSDFSet)
        fwd = _Eager.approach_terms_set if ctx.is_set else _Eager.approach_terms
        e = fwd(hp, samples.points, samples.link, hand.L, Rg, LT, scene.values, list(scene.origin), scene.voxel, axis, distance,
                stations, margin)
        ctx.save_for_backward(hp, idx, Rg, LT, ws, samples.points, samples.link, scene.values)
        ctx.hand, ctx.origin, ctx.voxel = hand, list(scene.origin), scene.voxel
        ctx.corridor = (axis, distance, stations, margin)
        return e

    @staticmethod
    def backward(ctx, g_approach):
        hp, idx, Rg, LT, ws, points, link, values = ctx.saved_tensors
        hand = ctx.hand
        bwd = _Eager.approach_terms_set_backward if ctx.is_set else _Eager.approach_terms_backward
        wrench, gRt = bwd(hp, points, link, hand.L, Rg, LT, values, ctx.origin, ctx.voxel, *ctx.corridor, g_approach)
        gp = _fk_backward(hand, hp, idx, Rg, LT, ws, None, None, None, wrench, gRt, None)
        return (gp,) + (None,) * 11


def approach_terms(hand_pose, hand: HandHandle, samples: SurfaceSamples, idx, Rg, LT, ws, scene: SceneSDF, grasp_axis, distance,
                   stations, margin=0.0):
    """-> E_approach (B) = (1/K) sum over the stations k = 1..K and over ``samples`` of max(margin - phi(x_w^k), 0) on the
    scene's grid, x_w^k the sample with the whole hand moved back by ``distance`` k / K along ``grasp_axis`` (hand frame);
    unweighted, differentiable w.r.t. ``hand_pose``.  ``idx``, ``Rg``, ``LT``, ``ws`` are the kinematic state of ``hand_pose``
    (fk_contacts); K = ``stations`` in 1..32, ``distance`` > 0 and ``margin`` >= 0 in metres."""
    if not hand_pose.is_cuda:
        raise RuntimeError("graspqp_amd ops need CUDA (ROCm) tensors; got a CPU tensor")
    if samples.n_links != hand.L:
        raise ValueError(f"approach_terms: the samples refer to {samples.n_links} links, the hand has {hand.L}")
    if not float(margin) >= 0.0:
        raise ValueError(f"approach_terms: margin = {margin!r} must be >= 0")
    axis = [float(a) for a in _axis3(grasp_axis)]
    approach_check(scene, hand_pose.shape[0], hand.L, samples.Ns, distance, stations, axis)
    return _ApproachTerms.apply(hand_pose, hand, samples, _c(idx, torch.int64), Rg.detach(), LT.detach(), ws, scene, axis,
                                float(distance), int(stations), float(margin))


# ----------------------------------------------------------------------------------------------------------
# pre-grasp clearance: E_pregrasp, the OPENED hand along the approach corridor (csrc/pregrasp.hip).  One launch does the opened
# kinematics, the stations and the joint gradient; a single grid crosses as the stack of one
# ----------------------------------------------------------------------------------------------------------
def _pregrasp_grids(values, origin, voxel) -> "_C.ClutterGrids":
    """gqClutterGrids of a (G,nx,ny,nz) stack, or of a single (nx,ny,nz) grid as the stack of one (a view: no copy)."""
    return _clutter_grids(values if values.dim() == 4 else values.unsqueeze(0), origin, voxel)


def pregrasp_check(scene, batch, n_links, n_samples, distance, stations, grasp_axis, opening):
    """gq_pregrasp_check (host only) of the grid or stack, a launch's shapes, the corridor and the opening; raises ValueError
    with the library's message."""
    if not isinstance(scene, (SceneSDF, SceneSDFSet)):
        raise ValueError("pregrasp: scene must be an ops.SceneSDF or an ops.SceneSDFSet")
    ax = _axis_c(grasp_axis)
    G = scene.n_grids if isinstance(scene, SceneSDFSet) else 1
    if int(batch) % G:
        raise ValueError(f"pregrasp: batch = {batch} is not divisible by n_grids = {G}")
    try:
        _C.call("gq_pregrasp_check", ctypes.byref(_pregrasp_grids(scene.values, scene.origin, scene.voxel)),
                ctypes.c_int64(int(batch)), ctypes.c_int64(int(batch) // G), int(n_links), ctypes.c_int64(int(n_samples)),
                float(distance), int(stations), ctypes.cast(ax, ctypes.c_void_p), float(opening))
    except RuntimeError as e:
        raise ValueError(f"pregrasp: {e}") from None


def default_open_joints(spec, device="cuda") -> Tensor:
    """The joints the term opens the hand towards unless told otherwise: ``spec.default_state`` clamped to the joint limits,
    the mean ``initialize_convex_hull`` opens the hand to; (JA) float32 on ``device``."""
    q = np.clip(np.asarray(spec.default_state, dtype=np.float32), np.asarray(spec.joints_lower, dtype=np.float32),
                np.asarray(spec.joints_upper, dtype=np.float32))
    return torch.from_numpy(np.ascontiguousarray(q)).to(device)


def _pregrasp_call(hand, grids, margin, distance, stations, opening, open_joints, hp, points, link, Rg, axis, up_pregrasp,
                   w_pregrasp, e_pregrasp, accumulate, g_theta, gRt, st=None):
    p, (B, D) = _dev, hp.shape
    _C.call("gq_pregrasp_terms", hand.handle, ctypes.byref(grids), B // max(grids.n_grids, 1), float(margin), float(distance),
            int(stations), float(opening), p(open_joints), _C.f32(points), p(link, torch.int32), points.shape[0], _C.f32(hp), D,
            p(Rg), B, _axis_c(axis), p(up_pregrasp), float(w_pregrasp), p(e_pregrasp), int(accumulate), p(g_theta), p(gRt),
            _C.stream_ptr() if st is None else st)


@_custom_op("graspqp_amd::pregrasp_terms", mutates_args=(), device_types="cuda")
def _pregrasp_op(hand_pose: Tensor, points: Tensor, link: Tensor, hand: int, Rg: Tensor, values: Tensor, origin: List[float],
                 voxel: float, grasp_axis: List[float], distance: float, stations: int, opening: float, open_joints: Tensor,
                 margin: float) -> Tensor:
    """-> E_pregrasp (B), unweighted: the mean over the stations d_k = distance k / stations, k = 0..stations, of the hinge sum of
    the hand's surface samples with the joints opened by ``opening`` towards ``open_joints`` and the hand moved back by d_k along
    grasp_axis.  ``values`` is one grid (nx,ny,nz) or a stack (G,nx,ny,nz); Rg is the rotation of ``hand_pose``."""
    h = _handle(hand)
    hp, v = _c(hand_pose), _c(values)
    e = torch.empty(hp.shape[0], device=hp.device)
    _pregrasp_call(h, _pregrasp_grids(v, origin, voxel), margin, distance, stations, opening, _c(open_joints), hp, _c(points),
                   _c(link, torch.int32), _c(Rg), grasp_axis, None, 0.0, e, 0, None, None)
    return e


@_pregrasp_op.register_fake
def _(hand_pose, points, link, hand, Rg, values, origin, voxel, grasp_axis, distance, stations, opening, open_joints, margin):
    return hand_pose.new_empty(hand_pose.shape[0])


@_custom_op("graspqp_amd::pregrasp_terms_backward", mutates_args=(), device_types="cuda")
def _pregrasp_bwd_op(hand_pose: Tensor, points: Tensor, link: Tensor, hand: int, Rg: Tensor, values: Tensor, origin: List[float],
                     voxel: float, grasp_axis: List[float], distance: float, stations: int, opening: float, open_joints: Tensor,
                     margin: float, g_pregrasp: Tensor) -> Tuple[Tensor, Tensor]:
    """Upstream row gradients (B) on E_pregrasp -> (g_theta (B,JA), gRt (B,12)): the direct joint gradient, and the global-pose
    part in the form fk_backward takes."""
    h = _handle(hand)
    hp, v = _c(hand_pose), _c(values)
    B, dev = hp.shape[0], hp.device
    g_theta, gRt = torch.empty(B, hp.shape[1] - 9, device=dev), torch.empty(B, 12, device=dev)
    _pregrasp_call(h, _pregrasp_grids(v, origin, voxel), margin, distance, stations, opening, _c(open_joints), hp, _c(points),
                   _c(link, torch.int32), _c(Rg), grasp_axis, _c(g_pregrasp), 0.0, None, 0, g_theta, gRt)
    return g_theta, gRt


@_pregrasp_bwd_op.register_fake
def _(hand_pose, points, link, hand, Rg, values, origin, voxel, grasp_axis, distance, stations, opening, open_joints, margin,
      g_pregrasp):
    B = hand_pose.shape[0]
    return hand_pose.new_empty(B, hand_pose.shape[1] - 9), hand_pose.new_empty(B, 12)


class _PregraspTerms(torch.autograd.Function):
    """Glue between registered ops (pregrasp_terms + fk_backward), as _ApproachTerms: the backward launch overwrites gRt and
    g_theta with the per-row upstream; the FK backward of the CLOSED hand turns gRt into the root-pose gradient (the opened hand
    shares the root pose), and g_theta is the joint part as it stands."""

    @staticmethod
    def forward(ctx, hand_pose, hand, samples, idx, Rg, LT, ws, scene, axis, distance, stations, opening, open_joints, margin):
        hp = _c(hand_pose.detach())
        e = _Eager.pregrasp_terms(hp, samples.points, samples.link, hand.hid, Rg, scene.values, list(scene.origin), scene.voxel,
                                  axis, distance, stations, opening, open_joints, margin)
        ctx.save_for_backward(hp, idx, Rg, LT, ws, samples.points, samples.link, scene.values, open_joints)
        ctx.hand, ctx.origin, ctx.voxel = hand, list(scene.origin), scene.voxel
        ctx.corridor = (axis, distance, stations, opening)
        ctx.margin = margin
        return e

    @staticmethod
    def backward(ctx, g_pregrasp):
        hp, idx, Rg, LT, ws, points, link, values, open_joints = ctx.saved_tensors
        hand = ctx.hand
        g_theta, gRt = _Eager.pregrasp_terms_backward(hp, points, link, hand.hid, Rg, values, ctx.origin, ctx.voxel, *ctx.corridor,
                                                      open_joints, ctx.margin, g_pregrasp)
        gp = _fk_backward(hand, hp, idx, Rg, LT, ws, None, None, None, None, gRt, None)
        gp[:, 9:] += g_theta
        return (gp,) + (None,) * 13


def pregrasp_terms(hand_pose, hand: HandHandle, samples: SurfaceSamples, idx, Rg, LT, ws, scene, grasp_axis, distance, stations,
                   opening, open_joints=None, margin=0.0):
    """-> E_pregrasp (B) = 1/(K+1) sum over the stations k = 0..K and over ``samples`` of max(margin - phi(x_w^k), 0) on the
    scene's grid, with the joints opened to (1 - opening) theta + opening ``open_joints`` and the whole hand moved back by
    ``distance`` k / K along ``grasp_axis`` (hand frame); unweighted, differentiable w.r.t. ``hand_pose``.  ``scene`` is an
    ``ops.SceneSDF`` or an ``ops.SceneSDFSet`` (row b reads grid b // (B / G)); it may contain the target, since station 0 is the
    opened hand at the grasp pose.  ``idx``, ``Rg``, ``LT``, ``ws`` are the kinematic state of ``hand_pose`` (fk_contacts);
    K = ``stations`` in 0..32, ``distance`` > 0, ``opening`` in [0,1], ``margin`` >= 0.  ``open_joints`` (JA) = None takes
    ``default_open_joints(spec)``: the default state clamped to the joint limits."""
    if not hand_pose.is_cuda:
        raise RuntimeError("graspqp_amd ops need CUDA (ROCm) tensors; got a CPU tensor")
    if samples.n_links != hand.L:
        raise ValueError(f"pregrasp_terms: the samples refer to {samples.n_links} links, the hand has {hand.L}")
    if not float(margin) >= 0.0:
        raise ValueError(f"pregrasp_terms: margin = {margin!r} must be >= 0")
    if hand_pose.shape[1] != 9 + hand.J:
        raise ValueError(f"pregrasp_terms: hand_pose must be (B, {9 + hand.J}), got {tuple(hand_pose.shape)}")
    axis = [float(a) for a in _axis3(grasp_axis)]
    pregrasp_check(scene, hand_pose.shape[0], hand.L, samples.Ns, distance, stations, axis, opening)
    dev = hand_pose.device
    if open_joints is None:
        open_joints = default_open_joints(hand.spec, dev)
    else:
        open_joints = _c(torch.as_tensor(open_joints, dtype=torch.float32).detach().to(dev))
    if open_joints.shape != (hand.J,):
        raise ValueError(f"pregrasp_terms: open_joints must be ({hand.J},), got {tuple(open_joints.shape)}")
    return _PregraspTerms.apply(hand_pose, hand, samples, _c(idx, torch.int64), Rg.detach(), LT.detach(), ws, scene, axis,
                                float(distance), int(stations), float(opening), open_joints, float(margin))


# ----------------------------------------------------------------------------------------------------------
# contact closing feasibility: E_squeeze (csrc/squeeze.hip), the reference's E_manipulativity (core/energy.py:80-87) as ONE launch:
# contact Jacobian, damped normal equations in fp64, both solves, residual, and the three gradient parts
# ----------------------------------------------------------------------------------------------------------
def squeeze_check(hand, n_contact, min_travel, damping, who="squeeze_terms"):
    """The parameters of the squeeze term (no GPU): finite min_travel > 0 and damping > 0 (J'J alone is singular for 3n < JA), at
    most 64 joints and 64 contacts; raises ValueError."""
    if not 0.0 < float(min_travel) < float("inf"):
        raise ValueError(f"{who}: squeeze_min_travel = {min_travel!r} must be finite and > 0")
    if not 0.0 < float(damping) < float("inf"):
        raise ValueError(f"{who}: squeeze_damping = {damping!r} must be finite and > 0")
    if hand is not None and not (1 <= int(n_contact) <= 64 and hand.spec.n_nodes <= 64 and hand.J <= 64):
        raise ValueError(f"{who}: the squeeze term takes at most 64 joints and 64 contacts, got {hand.spec.n_nodes} joints, "
                         f"n_contact = {n_contact}")


def _squeeze_call(hand, idx, Rg, LT, ws, d2, onrm, closest, cpts, min_travel, damping, up, w, e, theta, accumulate, g_theta, g_R,
                  g_R_base, g_cpts, st=None):
    p, (B, n) = _dev, idx.shape
    _C.call("gq_squeeze_terms", hand.handle, _C.i64(idx), ctypes.c_int64(B), n, p(d2), p(onrm), p(closest), p(cpts), p(Rg), p(LT),
            _C.ptr(ws), ws.numel(), float(min_travel), float(damping), p(up), float(w), p(e), p(theta), int(accumulate), p(g_theta),
            p(g_R), p(g_R_base), p(g_cpts), _C.stream_ptr() if st is None else st)


@_custom_op("graspqp_amd::squeeze_terms", mutates_args=(), device_types="cuda")
def _squeeze_op(hand: int, idx: Tensor, Rg: Tensor, LT: Tensor, ws: Tensor, dist_sq: Tensor, obj_normal: Tensor, min_travel: float,
                damping: float) -> Tuple[Tensor, Tensor]:
    """-> (E_squeeze (B), unweighted; theta (B,JA), the squeeze joint velocities) of the kinematic state (idx, Rg, LT, ws) and the
    contact query (dist_sq (B,n), outward obj_normal (B,n,3))."""
    h = _handle(hand)
    ix = _c(idx, torch.int64)
    B, dev = ix.shape[0], ix.device
    e, theta = torch.empty(B, device=dev), torch.empty(B, h.J, device=dev)
    _squeeze_call(h, ix, _c(Rg), _c(LT), ws, _c(dist_sq), _c(obj_normal), None, None, min_travel, damping, None, 0.0, e, theta, 0,
                  None, None, None, None)
    return e, theta


@_squeeze_op.register_fake
def _(hand, idx, Rg, LT, ws, dist_sq, obj_normal, min_travel, damping):
    B = idx.shape[0]
    return dist_sq.new_empty(B), dist_sq.new_empty(B, _handle(hand).J)


@_custom_op("graspqp_amd::squeeze_terms_backward", mutates_args=(), device_types="cuda")
def _squeeze_bwd_op(hand: int, idx: Tensor, Rg: Tensor, LT: Tensor, ws: Tensor, dist_sq: Tensor, obj_normal: Tensor, closest: Tensor,
                    contact_pts: Tensor, min_travel: float, damping: float, g_squeeze: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """Upstream row gradients (B) on E_squeeze -> (g_theta (B,JA), g_R (B,3,3), g_contact_pts (B,n,3)): the direct joint gradient,
    dE/dR in the form fk_backward takes, and the gradient to the contact points.  One launch."""
    h = _handle(hand)
    ix = _c(idx, torch.int64)
    (B, n), dev = ix.shape, ix.device
    g_theta, g_R, g_cp = torch.empty(B, h.J, device=dev), torch.empty(B, 3, 3, device=dev), torch.empty(B, n, 3, device=dev)
    _squeeze_call(h, ix, _c(Rg), _c(LT), ws, _c(dist_sq), _c(obj_normal), _c(closest), _c(contact_pts), min_travel, damping,
                  _c(g_squeeze), 1.0, None, None, 0, g_theta, g_R, None, g_cp)
    return g_theta, g_R, g_cp


@_squeeze_bwd_op.register_fake
def _(hand, idx, Rg, LT, ws, dist_sq, obj_normal, closest, contact_pts, min_travel, damping, g_squeeze):
    B, n = idx.shape
    e = dist_sq.new_empty
    return e(B, _handle(hand).J), e(B, 3, 3), e(B, n, 3)


class _SqueezeTerms(torch.autograd.Function):
    """Glue between registered ops (squeeze_terms + fk_backward), as _PregraspTerms: the backward launch writes g_theta, g_R and
    the contact-point gradient with the per-row upstream; the FK backward turns g_R into the root-rotation gradient, and g_theta is
    the joint part as it stands.  The contact-point gradient goes back to ``contact_pts`` (whose own graph carries it on)."""

    @staticmethod
    def forward(ctx, hand_pose, contact_pts, hand, idx, Rg, LT, ws, dist_sq, obj_normal, closest, min_travel, damping):
        hp = _c(hand_pose.detach())
        e, theta = _Eager.squeeze_terms(hand.hid, idx, Rg, LT, ws, dist_sq, obj_normal, min_travel, damping)
        ctx.save_for_backward(hp, idx, Rg, LT, ws, dist_sq, obj_normal, closest, _c(contact_pts.detach()))
        ctx.hand, ctx.par = hand, (min_travel, damping)
        ctx.mark_non_differentiable(theta)
        return e, theta

    @staticmethod
    def backward(ctx, g_squeeze, _g_theta):
        hp, idx, Rg, LT, ws, dist_sq, obj_normal, closest, cpts = ctx.saved_tensors
        hand = ctx.hand
        g_theta, g_R, g_cp = _Eager.squeeze_terms_backward(hand.hid, idx, Rg, LT, ws, dist_sq, obj_normal, closest, cpts, *ctx.par,
                                                           _c(g_squeeze))
        gp = _fk_backward(hand, hp, idx, Rg, LT, ws, None, None, None, None, None, g_R)
        gp[:, 9:] += g_theta
        return (gp, g_cp) + (None,) * 10


def squeeze_terms(hand_pose, hand: HandHandle, idx, Rg, LT, ws, dist_sq, obj_normal, closest, contact_pts, min_travel=5e-3,
                  damping=1e-3, return_theta=False):
    """-> E_squeeze (B) = 1/(3n) sum r^2, r = J theta - R' d, theta = (J'J + damping I)^-1 J' R' d, d_i = obj_normal_i
    max(sqrt(dist_sq_i + 1e-8), min_travel): the mean squared part of the contacts' closing motion that the joints cannot produce.
    At the defaults it is the reference's E_manipulativity (core/energy.py:80-87) in value and gradient.  Unweighted; differentiable
    w.r.t. ``hand_pose`` (joints through the contact Jacobian, root rotation through R' d) and ``contact_pts`` (through the travel
    of the contacts above ``min_travel``; the normals are constants, as in the reference).  ``idx``, ``Rg``, ``LT``, ``ws`` are the
    kinematic state of ``hand_pose`` (fk_contacts); ``dist_sq`` (B,n), ``obj_normal`` (B,n,3, outward), ``closest`` (B,n,3) the object
    query of ``contact_pts`` (B,n,3).  ``return_theta``: also the squeeze joint velocities theta (B,JA)."""
    if not hand_pose.is_cuda:
        raise RuntimeError("graspqp_amd ops need CUDA (ROCm) tensors; got a CPU tensor")
    if hand_pose.shape[1] != 9 + hand.J:
        raise ValueError(f"squeeze_terms: hand_pose must be (B, {9 + hand.J}), got {tuple(hand_pose.shape)}")
    B, n = idx.shape
    squeeze_check(hand, n, min_travel, damping)
    if tuple(dist_sq.shape) != (B, n) or tuple(obj_normal.shape) != (B, n, 3) or tuple(closest.shape) != (B, n, 3) or \
            tuple(contact_pts.shape) != (B, n, 3):
        raise ValueError(f"squeeze_terms: dist_sq must be ({B}, {n}) and obj_normal / closest / contact_pts ({B}, {n}, 3)")
    e, theta = _SqueezeTerms.apply(hand_pose, contact_pts, hand, _c(idx, torch.int64), _c(Rg.detach()), _c(LT.detach()), ws,
                                   _c(dist_sq.detach()), _c(obj_normal.detach()), _c(closest.detach()), float(min_travel),
                                   float(damping))
    return (e, theta) if return_theta else e


# ----------------------------------------------------------------------------------------------------------
# payload holding: E_hold (csrc/hold.hip), the load wrenches a grasp can carry as ONE launch: the E_fc step's cone matrix on the
# inward normals, one box QP per load wrench side by side (low-rank PDIPM, a fixed number of iterations, row-local best iterate),
# the unheld share of the load, the contact forces and the joint torques they ask of the hand
# ----------------------------------------------------------------------------------------------------------
HOLD_DEFAULTS = {"ridge": 1e-4, "iterations": 16}


class HoldResult(NamedTuple):
    """What ``hold_terms(..., return_details=True)`` and ``GraspStepper.hold`` return; every field unweighted."""
    e: Tensor       # (B) E_hold = mean over the loads of V_l / |w_l|^2, the unheld share of the load
    resid: Tensor   # (B,L) |F x_l + w_l| / |w_l| without the ridge part: what one gates on
    x: Tensor       # (B,L,nz) cone-edge coefficients in [0, max_force]; normal force of contact c: sqrt(1 - mu^2) / k * sum_e x
    force: Tensor   # (B,L,n,3) force of finger c on the object, world frame, newtons
    torque: Tensor  # (B,L,JA) actuated joint torques J_act' R' force; values only, no gradient
    effort: Optional[Tensor]  # (B) max |torque| / torque_limits, or None without limits; values only


def hold_loads(mass, up=(0.0, 0.0, 1.0), accelerations=((0.0, 0.0, 0.0),), com_offset=None, g=9.81):
    """-> the load wrenches of ``hold_terms`` as a CPU float32 tensor: (L,6) for a scalar ``mass`` in kg, (n_obj,L,6) for a
    sequence of masses.  Load l is what the hand has to hold the object against while it accelerates with ``accelerations[l]``
    (m/s^2, object frame) under gravity along -``up`` (normalised here): force -m (g up + a), torque ``com_offset`` x force about
    the centre the contacts' ``cog`` stands for (``com_offset`` (3,) or (n_obj,3): where the true centre of mass lies relative
    to it; None: no offset).  The default is the object's weight alone."""
    m = torch.as_tensor(mass, dtype=torch.float64)
    per_object = m.dim() > 0
    m = m.reshape(-1)
    upv = torch.as_tensor(up, dtype=torch.float64).reshape(-1)
    acc = torch.as_tensor(accelerations, dtype=torch.float64)
    if not (m.numel() >= 1 and bool(torch.isfinite(m).all()) and bool((m > 0).all())):
        raise ValueError(f"hold_loads: mass = {mass!r} must be finite and > 0")
    if upv.shape != (3,) or not bool(torch.isfinite(upv).all()) or float(upv.norm()) == 0.0:
        raise ValueError(f"hold_loads: up = {up!r} must be a finite non-zero 3-vector")
    if acc.dim() != 2 or acc.shape[1] != 3 or not 1 <= acc.shape[0] <= 8 or not bool(torch.isfinite(acc).all()):
        raise ValueError(f"hold_loads: accelerations must be (L,3) with 1 <= L <= 8 and finite, got {tuple(acc.shape)}")
    if not 0.0 < float(g) < float("inf"):
        raise ValueError(f"hold_loads: g = {g!r} must be finite and > 0")
    force = -m.view(-1, 1, 1) * (float(g) * (upv / upv.norm()).view(1, 1, 3) + acc.unsqueeze(0))  # (n_obj,L,3)
    if com_offset is None:
        torque = torch.zeros_like(force)
    else:
        off = torch.as_tensor(com_offset, dtype=torch.float64)
        if off.shape not in ((3,), (m.numel(), 3)) or not bool(torch.isfinite(off).all()):
            raise ValueError(f"hold_loads: com_offset must be (3,) or ({m.numel()},3) and finite, got {tuple(off.shape)}")
        torque = torch.cross(off.reshape(-1, 1, 3).expand_as(force), force, dim=-1)
    w = torch.cat([force, torque], -1).float()
    return w if per_object else w[0]


def hold_check(hand, n_contact, n_cone_vecs, loads, max_force, ridge=1e-4, iterations=16, friction=0.2, torque_weight=5.0,
               torque_limits=None, n_obj=None, who="hold_terms"):
    """The parameter checks of the payload-holding term (no GPU; raises ValueError): at most 64 contacts and joints, n_cone_vecs >=
    3 and n_contact * n_cone_vecs <= 128 columns, ``loads`` (L,6) or (n_obj,L,6) with 1 <= L <= 8, every load finite with a
    non-zero wrench once its torque is multiplied by ``torque_weight``, max_force and ridge finite and > 0, 1 <= iterations <= 64,
    friction in (0, 1], ``torque_limits`` (JA) finite and > 0.  -> the loads as a CPU float32 tensor (n_sets,L,6)."""
    lw = torch.as_tensor(loads).detach().to("cpu", torch.float32)
    if lw.dim() == 2:
        lw = lw.unsqueeze(0)
    if lw.dim() != 3 or lw.shape[2] != 6 or not 1 <= lw.shape[1] <= 8 or lw.shape[0] < 1:
        raise ValueError(f"{who}: loads must be (L,6) or (n_obj,L,6) with 1 <= L <= 8, got {tuple(torch.as_tensor(loads).shape)}")
    if n_obj is not None and lw.shape[0] not in (1, int(n_obj)):
        raise ValueError(f"{who}: loads are given for {lw.shape[0]} objects, the batch has {int(n_obj)}")
    if not 0.0 <= float(torque_weight) < float("inf"):
        raise ValueError(f"{who}: torque_weight = {torque_weight!r} must be finite and >= 0")
    scaled = torch.cat([lw[..., :3], float(torque_weight) * lw[..., 3:]], -1)
    if not bool(torch.isfinite(scaled).all()) or not bool((scaled.norm(dim=-1) > 0).all()):
        raise ValueError(f"{who}: every load must be finite with a non-zero wrench (torque rows times torque_weight)")
    if not 0.0 < float(max_force) < float("inf"):
        raise ValueError(f"{who}: hold_max_force = {max_force!r} must be finite and > 0")
    if not 0.0 < float(ridge) < float("inf"):
        raise ValueError(f"{who}: ridge = {ridge!r} must be finite and > 0")
    if not 1 <= int(iterations) <= 64:
        raise ValueError(f"{who}: hold_iterations = {iterations!r} must be in 1..64")
    if not 0.0 < float(friction) <= 1.0:
        raise ValueError(f"{who}: friction = {friction!r} must be in (0, 1]")
    if n_contact is not None and not (1 <= int(n_contact) <= 64 and int(n_cone_vecs) >= 3 and int(n_contact) * int(n_cone_vecs) <= 128):
        raise ValueError(f"{who}: 1..64 contacts, n_cone_vecs >= 3 and at most 128 columns are supported, got n_contact = {n_contact}, "
                         f"n_cone_vecs = {n_cone_vecs}")
    if hand is not None and not (hand.spec.n_nodes <= 64 and hand.J <= 64):
        raise ValueError(f"{who}: the hold term takes at most 64 joints, got {hand.spec.n_nodes}")
    if torque_limits is not None:
        tl = torch.as_tensor(torque_limits).detach().to("cpu", torch.float32).reshape(-1)
        if (hand is not None and tl.numel() != hand.J) or not bool(torch.isfinite(tl).all()) or not bool((tl > 0).all()):
            raise ValueError(f"{who}: torque_limits must be ({hand.J if hand is not None else 'JA'},) finite and > 0")
    return lw.contiguous()


def _hold_call(hand, idx, Rg, LT, ws, onrm, cpts, cog, loads, loads_each, k, mu, tw, max_force, ridge, iters, limits, up, w, e, resid, x,
               force, torque, effort, accumulate, g_cpts, st=None):
    """gq_hold_terms on loads the caller has checked (hold_check): the host copy is not passed."""
    p, (B, n) = _dev, cpts.shape[:2]
    kin = torque is not None or effort is not None
    _C.call("gq_hold_terms", hand.handle if kin else None, _C.i64(idx) if kin else None, ctypes.c_int64(B), n, int(k), p(onrm), p(cpts),
            p(cog), p(Rg) if kin else None, p(LT) if kin else None, _C.ptr(ws) if kin else None, ws.numel() if kin else 0, p(loads), None,
            ctypes.c_int64(loads.shape[0]), int(loads.shape[1]), ctypes.c_int64(loads_each), float(mu), float(tw), float(max_force),
            float(ridge), int(iters), p(limits), p(up), float(w), p(e), p(resid), p(x), p(force), p(torque), p(effort), int(accumulate),
            p(g_cpts), _C.stream_ptr() if st is None else st)


@_custom_op("graspqp_amd::hold_terms", mutates_args=(), device_types="cuda")
def _hold_op(hand: int, idx: Tensor, Rg: Tensor, LT: Tensor, ws: Tensor, obj_normal: Tensor, contact_pts: Tensor, cog: Tensor,
             loads: Tensor, loads_each: int, friction: float, torque_weight: float, n_cone_vecs: int, max_force: float, ridge: float,
             iterations: int, torque_limits: Optional[Tensor]) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """-> (E_hold (B), resid (B,L), x (B,L,nz), force (B,L,n,3), torque (B,L,JA), effort (B), or (0) without limits) of the contact
    query (outward obj_normal, contact_pts, cog (B,3)) and the kinematic state (idx, Rg, LT, ws); loads (n_sets,L,6) on the device,
    checked by the caller (hold_check)."""
    h = _handle(hand)
    ix = _c(idx, torch.int64)
    (B, n), dev, L = ix.shape, ix.device, loads.shape[1]
    f = lambda *s: torch.empty(*s, device=dev)
    e, resid, x, force, torque = f(B), f(B, L), f(B, L, n * n_cone_vecs), f(B, L, n, 3), f(B, L, h.J)
    effort = f(B) if torque_limits is not None else f(0)
    _hold_call(h, ix, _c(Rg), _c(LT), ws, _c(obj_normal), _c(contact_pts), _c(cog), _c(loads), loads_each, n_cone_vecs, friction,
               torque_weight, max_force, ridge, iterations, None if torque_limits is None else _c(torque_limits), None, 0.0, e, resid, x,
               force, torque, effort if torque_limits is not None else None, 0, None)
    return e, resid, x, force, torque, effort


@_hold_op.register_fake
def _(hand, idx, Rg, LT, ws, obj_normal, contact_pts, cog, loads, loads_each, friction, torque_weight, n_cone_vecs, max_force, ridge,
      iterations, torque_limits):
    (B, n), L, f = idx.shape, loads.shape[1], contact_pts.new_empty
    return f(B), f(B, L), f(B, L, n * n_cone_vecs), f(B, L, n, 3), f(B, L, _handle(hand).J), f(B if torque_limits is not None else 0)


@_custom_op("graspqp_amd::hold_terms_backward", mutates_args=(), device_types="cuda")
def _hold_bwd_op(obj_normal: Tensor, contact_pts: Tensor, cog: Tensor, loads: Tensor, loads_each: int, friction: float,
                 torque_weight: float, n_cone_vecs: int, max_force: float, ridge: float, iterations: int, g_hold: Tensor) -> Tensor:
    """Upstream row gradients (B) on E_hold -> g_contact_pts (B,n,3), the envelope gradient through the torque rows of F (the
    normals are constants).  One launch: the loads are solved again, nothing is kept from the forward."""
    cp = _c(contact_pts)
    g_cp = torch.empty_like(cp)
    _hold_call(None, None, None, None, None, _c(obj_normal), cp, _c(cog), _c(loads), loads_each, n_cone_vecs, friction, torque_weight,
               max_force, ridge, iterations, None, _c(g_hold), 1.0, None, None, None, None, None, None, 0, g_cp)
    return g_cp


@_hold_bwd_op.register_fake
def _(obj_normal, contact_pts, cog, loads, loads_each, friction, torque_weight, n_cone_vecs, max_force, ridge, iterations, g_hold):
    return torch.empty_like(contact_pts)


def _hold_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[5], inputs[6], inputs[7], inputs[8])
    ctx.par = tuple(inputs[9:16])
    ctx.mark_non_differentiable(*output[1:])


def _hold_bwd(ctx, g_e, *_):
    onrm, cp, cog, loads = ctx.saved_tensors
    g_cp = _Eager.hold_terms_backward(onrm, cp, cog, loads, *ctx.par, _c(g_e))
    return (None,) * 6 + (g_cp,) + (None,) * 10


torch.library.register_autograd("graspqp_amd::hold_terms", _hold_bwd, setup_context=_hold_setup)


def _hold_cog(cog, B, batch_each, who):
    cog = _c(cog.detach())
    if cog.shape == (B, 3):
        return cog
    if cog.dim() == 2 and cog.shape[1] == 3 and cog.shape[0] * int(batch_each) == B:
        return cog.repeat_interleave(int(batch_each), dim=0).contiguous()
    raise ValueError(f"{who}: cog must be ({B}, 3) or (n_obj, 3) with n_obj * batch_each = {B}, got {tuple(cog.shape)}")


def hold_terms(hand_pose, hand: HandHandle, idx, Rg, LT, ws, obj_normal, contact_pts, cog, loads, batch_each, friction, torque_weight,
               n_cone_vecs, max_force, ridge=1e-4, iterations=16, torque_limits=None, return_details=False):
    """-> E_hold (B) = (1/L) sum_l V_l(x_l) / |w_l|^2 with x_l = argmin_{0 <= x <= max_force} V_l(x) = |F x + w_l|^2 + ridge |x|^2:
    the share of the load wrenches ``loads`` that the contacts cannot carry (1: nothing, down to a floor set by the ridge).  F is
    the E_fc step's cone matrix of (``contact_pts``, ``obj_normal``, ``cog``, ``friction``, ``torque_weight``, ``n_cone_vecs``) on the
    INWARD normals; ``loads`` (L,6) for every object or (n_obj,L,6) per object (``hold_loads``; row b belongs to object
    b // batch_each) are wrenches (N, N m) on the object about ``cog``; ``max_force`` bounds every edge coefficient in newtons (the
    normal force of a contact is sqrt(1 - mu^2) / k * sum_e x).  Exactly ``iterations`` PDIPM iterations per load, the iterate with
    the load's own smallest residual: a row's result depends on that row alone.  Differentiable w.r.t. ``contact_pts`` ONLY (the
    envelope gradient through the torque rows of F; the normals are constants as in E_fc): exact at the optimum, at the default
    16 iterations within 7e-4 of it.  ``idx``, ``Rg``, ``LT``, ``ws``: the kinematic state of ``hand_pose`` (fk_contacts), read for
    the joint torques.  ``return_details``: a ``HoldResult``; its torque and effort are values only.  Pass ``loads`` as a CPU tensor
    (a CUDA one is fetched for the checks, which synchronises)."""
    if not contact_pts.is_cuda:
        raise RuntimeError("graspqp_amd ops need CUDA (ROCm) tensors; got a CPU tensor")
    if hand_pose.shape[1] != 9 + hand.J:
        raise ValueError(f"hold_terms: hand_pose must be (B, {9 + hand.J}), got {tuple(hand_pose.shape)}")
    B, n = idx.shape
    if int(batch_each) < 1 or B % int(batch_each):
        raise ValueError(f"hold_terms: batch_each = {batch_each!r} must divide the batch {B}")
    lw = hold_check(hand, n, n_cone_vecs, loads, max_force, ridge, iterations, friction, torque_weight, torque_limits,
                    B // int(batch_each))
    if tuple(obj_normal.shape) != (B, n, 3) or tuple(contact_pts.shape) != (B, n, 3):
        raise ValueError(f"hold_terms: obj_normal and contact_pts must be ({B}, {n}, 3)")
    dev = contact_pts.device
    lim = None if torque_limits is None else torch.as_tensor(torque_limits, dtype=torch.float32).reshape(-1).to(dev)
    out = _hold_terms_checked(hand, idx, Rg, LT, ws, obj_normal, contact_pts, _hold_cog(cog, B, batch_each, "hold_terms"), lw.to(dev),
                              B if lw.shape[0] == 1 else int(batch_each), friction, torque_weight, n_cone_vecs, max_force, ridge,
                              iterations, lim)
    return out if return_details else out.e


def _hold_terms_checked(hand, idx, Rg, LT, ws, obj_normal, contact_pts, cog, loads_dev, loads_each, friction, torque_weight, n_cone_vecs,
                        max_force, ridge, iterations, limits):
    e, resid, x, force, torque, effort = _Eager.hold_terms(
        hand.hid, _c(idx, torch.int64), _c(Rg.detach()), _c(LT.detach()), ws, _c(obj_normal.detach()), contact_pts, cog, loads_dev,
        int(loads_each), float(friction), float(torque_weight), int(n_cone_vecs), float(max_force), float(ridge), int(iterations), limits)
    return HoldResult(e, resid, x, force, torque, effort if limits is not None else None)


def hold_contacts(contact_pts, obj_normal, cog, loads, batch_each, friction, torque_weight, n_cone_vecs, max_force, ridge=1e-4,
                  iterations=16):
    """-> (E_hold (B), resid (B,L), force (B,L,n,3)) of ``hold_terms`` on contacts that are NOT contact candidates of the hand: the
    points and outward object normals (B,n,3) of ``CloseResult.contacts(n)``.  It is the same launch without kinematics, so there
    are no joint torques: the torque of a force at an arbitrary link point needs a Jacobian of that point, which the package does
    not have.  A slot with a zero normal has an all-zero cone column (t1 = n x b1 = 0, f = 0, tau = r x f = 0) and carries
    nothing, so padded slots stand for "no contact".  Values only."""
    if not contact_pts.is_cuda:
        raise RuntimeError("graspqp_amd ops need CUDA (ROCm) tensors; got a CPU tensor")
    if contact_pts.dim() != 3 or contact_pts.shape[2] != 3 or tuple(obj_normal.shape) != tuple(contact_pts.shape):
        raise ValueError(f"hold_contacts: contact_pts and obj_normal must both be (B,n,3), got {tuple(contact_pts.shape)} / "
                         f"{tuple(obj_normal.shape)}")
    B, n = contact_pts.shape[:2]
    if int(batch_each) < 1 or B % int(batch_each):
        raise ValueError(f"hold_contacts: batch_each = {batch_each!r} must divide the batch {B}")
    lw = hold_check(None, n, n_cone_vecs, loads, max_force, ridge, iterations, friction, torque_weight, None, B // int(batch_each),
                    who="hold_contacts")
    dev = contact_pts.device
    lw = lw.to(dev)
    L = lw.shape[1]
    e, resid, force = torch.empty(B, device=dev), torch.empty(B, L, device=dev), torch.empty(B, L, n, 3, device=dev)
    _hold_call(None, None, None, None, None, _c(obj_normal.detach()), _c(contact_pts.detach()), _hold_cog(cog, B, batch_each, "hold_contacts"),
               lw, B if lw.shape[0] == 1 else int(batch_each), n_cone_vecs, friction, torque_weight, max_force, ridge, iterations, None,
               None, 0.0, e, resid, None, force, None, None, 0, None)
    return e, resid, force


# ----------------------------------------------------------------------------------------------------------
# finger closing (csrc/close.hip): the joints stepped along a closing direction until the links touch the object grid, S + 1
# dependent rounds of kinematics, grid query, per-link minimum, masks and update as ONE launch.  Values only.
# ----------------------------------------------------------------------------------------------------------
CLOSE_DEFAULTS = {"steps": 32, "touch": 5e-4, "step_revolute": 0.01, "step_prismatic": 5e-4}


class CloseResult(NamedTuple):
    """What ``close_fingers`` and ``GraspStepper.close`` return: the final state of finger closing (include/graspqp_hip.h)."""
    theta: Tensor       # (B,JA) closed joints
    touch_step: Tensor  # (B,L) int32, the first step at which link l touched; -1: never
    joint_stop: Tensor  # (B,JA) int32, the first step at which a touch stopped joint a; -1: not stopped by a touch
    phi: Tensor         # (B,L) smallest phi over the link's samples inside the volume, +inf without one; max(-phi, 0): overshoot
    sample: Tensor      # (B,L) int32, the sample that has it, -1 if none
    point: Tensor       # (B,L,3) its world position
    normal: Tensor      # (B,L,3) the object's outward normal there, zeros where there is none
    touched: Tensor     # (B,L) bool, touch_step >= 0

    def contacts(self, n):
        """-> (contact_pts, obj_normal), both (B,n,3), for ``hold_contacts``: the touched links in link order, at most ``n`` of
        them; the unused slots hold zero points and ZERO normals, which give all-zero cone columns.  No host synchronisation."""
        B, L = self.touched.shape
        n = int(n)
        if n < 1:
            raise ValueError(f"CloseResult.contacts: n = {n} must be >= 1")
        order = torch.sort((~self.touched).to(torch.int32), dim=1, stable=True).indices  # touched links first, in link order
        if n > L:
            order = torch.cat([order, order[:, :1].expand(B, n - L)], 1)
        order = order[:, :n]
        used = torch.arange(n, device=order.device)[None] < self.touched.sum(1, keepdim=True)
        pick = order.unsqueeze(-1).expand(B, n, 3)
        keep = used.unsqueeze(-1)
        zero = torch.zeros((), device=order.device)
        return (torch.where(keep, self.point.gather(1, pick), zero).contiguous(),
                torch.where(keep, self.normal.gather(1, pick), zero).contiguous())


def _close_spec(spec_or_hand):
    spec = getattr(spec_or_hand, "spec", spec_or_hand)
    J, JA, L = int(spec.n_nodes), int(spec.n_dofs), int(spec.n_links)
    C = np.asarray(spec.coupling, np.float64).reshape(J, JA) != 0 if spec.is_coupled else np.eye(J, dtype=bool)
    return spec, J, JA, L, C


def close_stop_masks_host(spec_or_hand) -> np.ndarray:
    """``joint_links`` (JA) uint64 on the host: bit l of entry a is set when link l rides on a tree node in the subtree of a tree
    node that actuated joint a drives (``coupling[j, a] != 0``; an uncoupled hand drives node a alone)."""
    spec, J, JA, L, C = _close_spec(spec_or_hand)
    if L > 64 or J > 64 or JA > 64:
        raise ValueError(f"close: the hand must have at most 64 joints and 64 links, got J={J} JA={JA} L={L}")
    parent = [int(p) for p in spec.node_parent]
    masks = np.zeros(JA, np.uint64)
    for l in range(L):
        j = int(spec.link_node[l])
        while j >= 0:  # the nodes between the link and the base
            for a in np.nonzero(C[j])[0]:
                masks[a] |= np.uint64(1) << np.uint64(l)
            j = parent[j]
    return masks


def close_stop_masks(hand: HandHandle) -> Tensor:
    """The ``joint_links`` tensor of ``close_fingers`` for ``hand``: (JA) int64 on the hand's device (the bits of the uint64 masks of
    ``close_stop_masks_host``), built once per hand and kept on the handle."""
    m = getattr(hand, "_close_masks", None)
    if m is None:
        m = torch.from_numpy(close_stop_masks_host(hand).view(np.int64).copy()).to(hand.device)
        hand._close_masks = m
    return m


def close_default_step(spec_or_hand) -> np.ndarray:
    """The default ``step`` (JA) float32: 0.01 rad for an actuated joint that drives revolute nodes, 5e-4 m for one that drives
    prismatic nodes; a joint that drives both kinds (or none) raises ValueError."""
    spec, J, JA, L, C = _close_spec(spec_or_hand)
    ntype = np.asarray(spec.node_type).reshape(-1)
    step = np.zeros(JA, np.float32)
    for a in range(JA):
        kinds = {int(ntype[j]) == 1 for j in np.nonzero(C[:, a])[0]}
        if len(kinds) != 1:
            raise ValueError(f"close: actuated joint {a} drives {'no node' if not kinds else 'revolute and prismatic nodes'}; pass step=")
        step[a] = CLOSE_DEFAULTS["step_revolute"] if kinds.pop() else CLOSE_DEFAULTS["step_prismatic"]
    return step


def _close_step(hand, step):
    """``step`` (None, a scalar or (JA)) -> (JA) float32 numpy"""
    if step is None:
        return close_default_step(hand)
    s = np.asarray(step.detach().cpu() if torch.is_tensor(step) else step, dtype=np.float32).reshape(-1)
    if s.size == 1:
        s = np.full(hand.J, s[0], np.float32)
    if s.shape != (hand.J,):
        raise ValueError(f"close: step must be a scalar or ({hand.J},), got {tuple(s.shape)}")
    return np.ascontiguousarray(s)


def _scene_arg(grid, batch, who):
    """An ``ops.SceneSDF`` or ``ops.SceneSDFSet`` whose grids divide the batch, else ValueError -> rows per grid."""
    if not isinstance(grid, (SceneSDF, SceneSDFSet)):
        raise ValueError(f"{who}: grid must be an ops.SceneSDF or an ops.SceneSDFSet")
    G = grid.n_grids if isinstance(grid, SceneSDFSet) else 1
    if int(batch) % G:
        raise ValueError(f"{who}: batch = {batch} is not divisible by n_grids = {G}")
    return int(batch) // G


def close_check(grid, batch, hand, n_samples, steps, step, touch):
    """gq_close_check (host only): the grid or stack against the batch, ``steps`` in 1..64, ``step`` (JA, numpy) finite and > 0,
    ``touch`` finite and >= 0, at most 64 joints and links; raises ValueError with the library's message."""
    rows = _scene_arg(grid, batch, "close")
    spec = getattr(hand, "spec", hand)
    st = None if step is None else np.ascontiguousarray(np.asarray(step, np.float32))
    if st is not None and st.shape != (int(spec.n_dofs),):
        raise ValueError(f"close: step must be ({int(spec.n_dofs)},), got {tuple(st.shape)}")
    try:
        _C.call("gq_close_check", ctypes.byref(_pregrasp_grids(grid.values, grid.origin, grid.voxel)), ctypes.c_int64(int(batch)),
                ctypes.c_int64(rows), int(spec.n_nodes), int(spec.n_dofs), int(spec.n_links), ctypes.c_int64(int(n_samples)),
                int(steps), None if st is None else st.ctypes.data_as(ctypes.c_void_p), float(touch))
    except RuntimeError as e:
        raise ValueError(f"close: {e}") from None


def _close_call(hand, grids, points, link, hp, Rg, direction, steps, step, touch, masks, theta, touch_step, joint_stop, phi, sample,
                point, normal, st=None):
    """gq_close_fingers on arguments the caller has checked (close_check): the host copy of ``step`` is not passed."""
    p, (B, D) = _dev, hp.shape
    _C.call("gq_close_fingers", hand.handle, ctypes.byref(grids), ctypes.c_int64(B // max(grids.n_grids, 1)), _C.f32(points),
            p(link, torch.int32), ctypes.c_int64(points.shape[0]), _C.f32(hp), D, p(Rg), ctypes.c_int64(B), p(direction), int(steps),
            p(step), None, float(touch), p(masks, torch.int64), p(theta), p(touch_step, torch.int32), p(joint_stop, torch.int32), p(phi),
            p(sample, torch.int32), p(point), p(normal), _C.stream_ptr() if st is None else st)


def _close_outputs(hp, L):
    B, JA, dev = hp.shape[0], hp.shape[1] - 9, hp.device
    f = lambda *s: torch.empty(*s, device=dev)
    i = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
    return f(B, JA), i(B, L), i(B, JA), f(B, L), i(B, L), f(B, L, 3), f(B, L, 3)


@_custom_op("graspqp_amd::close_fingers", mutates_args=(), device_types="cuda")
def _close_op(hand_pose: Tensor, points: Tensor, link: Tensor, hand: int, Rg: Tensor, values: Tensor, origin: List[float],
              voxel: float, direction: Tensor, steps: int, step: Tensor, touch: float,
              joint_links: Tensor) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """-> (theta (B,JA), touch_step (B,L) int32, joint_stop (B,JA) int32, phi (B,L), sample (B,L) int32, point (B,L,3), normal
    (B,L,3)): finger closing of the rows of ``hand_pose`` along ``direction`` (B,JA) on one grid (nx,ny,nz) or a stack
    (G,nx,ny,nz) that contains the target; ``step`` (JA) and ``joint_links`` (JA) int64 on the device.  Values only."""
    h = _handle(hand)
    hp, v = _c(hand_pose), _c(values)
    out = _close_outputs(hp, h.L)
    _close_call(h, _pregrasp_grids(v, origin, voxel), _c(points), _c(link, torch.int32), hp, _c(Rg), _c(direction), steps, _c(step), touch,
                _c(joint_links, torch.int64), *out)
    return out


@_close_op.register_fake
def _(hand_pose, points, link, hand, Rg, values, origin, voxel, direction, steps, step, touch, joint_links):
    B, JA, L = hand_pose.shape[0], hand_pose.shape[1] - 9, _handle(hand).L
    f = hand_pose.new_empty
    i = lambda *s: hand_pose.new_empty(*s, dtype=torch.int32)
    return f(B, JA), i(B, L), i(B, JA), f(B, L), i(B, L), f(B, L, 3), f(B, L, 3)


def _close_setup(ctx, inputs, output):
    ctx.n_in = len(inputs)
    ctx.mark_non_differentiable(*output)


def _close_bwd(ctx, *grads):
    return (None,) * ctx.n_in


torch.library.register_autograd("graspqp_amd::close_fingers", _close_bwd, setup_context=_close_setup)


def close_fingers(hand_pose, hand: HandHandle, samples: SurfaceSamples, Rg, grid, direction, steps=32, step=None, touch=5e-4):
    """Close the fingers until they touch -> ``CloseResult``.  From the joints of ``hand_pose`` (B, 9 + JA; ``Rg`` its rotation, as
    fk_contacts returns it) the actuated joints move along ``direction`` (B,JA), the fastest one by exactly its ``step`` per step,
    for ``steps`` steps in 1..64.  After every step each link's smallest phi over its surface ``samples`` is read from ``grid``, an
    ``ops.SceneSDF`` or an ``ops.SceneSDFSet`` (row b reads grid b // (B / G)) that CONTAINS THE TARGET; a link touches when that
    phi is at or under ``touch`` metres, and from then on its own joint and every joint between it and the palm stand still
    (``close_stop_masks``), while the joints beyond it keep closing up to their limits.  ``step`` (a scalar or (JA)) = None takes
    0.01 rad for revolute and 5e-4 m for prismatic actuated joints.  There is no sub-step refinement: the overshoot is at most
    step x lever arm and ``max(-phi, 0)`` reports it.  Values only: nothing here is differentiable.  One launch, bitwise
    reproducible, graph-capturable."""
    if not hand_pose.is_cuda:
        raise RuntimeError("graspqp_amd ops need CUDA (ROCm) tensors; got a CPU tensor")
    if samples.n_links != hand.L:
        raise ValueError(f"close_fingers: the samples refer to {samples.n_links} links, the hand has {hand.L}")
    B = hand_pose.shape[0]
    if hand_pose.dim() != 2 or hand_pose.shape[1] != 9 + hand.J:
        raise ValueError(f"close_fingers: hand_pose must be (B, {9 + hand.J}), got {tuple(hand_pose.shape)}")
    if tuple(direction.shape) != (B, hand.J):
        raise ValueError(f"close_fingers: direction must be ({B}, {hand.J}), got {tuple(direction.shape)}")
    st = _close_step(hand, step)
    close_check(grid, B, hand, samples.Ns, steps, st, touch)
    dev = hand_pose.device
    out = _Eager.close_fingers(_c(hand_pose.detach()), samples.points, samples.link, hand.hid, _c(Rg.detach()), grid.values,
                               list(grid.origin), grid.voxel, _c(direction.detach()), int(steps), torch.from_numpy(st).to(dev),
                               float(touch), close_stop_masks(hand))
    return CloseResult(*out, out[1] >= 0)


# ----------------------------------------------------------------------------------------------------------
# arm reachability: E_reach (csrc/reach.hip), batched damped-least-squares wrist IK as ONE launch: eight lanes per IK problem, the
# seeds and stations of a row side by side in one block, the gradient in the gRt layout the FK backward takes
# ----------------------------------------------------------------------------------------------------------
REACH_DEFAULTS = {"distance": 0.10, "stations": 0, "iterations": 24, "damping": 1e-4, "rot_scale": 0.1}


class ArmHandle(_DeviceObject):
    """Device copy of an ``ArmSpec`` (gq_arm_create: the set-up owner of csrc/setup.h holds the memory)."""

    def __init__(self, spec: ArmSpec, device=None):
        if not isinstance(spec, ArmSpec):
            raise ValueError("ArmHandle: spec must be an ops.ArmSpec")
        self.spec = spec
        keep = []

        def arr(a, dt):
            a = np.ascontiguousarray(np.asarray(a, dtype=dt))
            keep.append(a)
            return a.ctypes.data_as(ctypes.c_void_p)

        d = _C.ArmDesc()
        d.n_joints, d.n_seeds = spec.n_joints, spec.n_seeds
        d.joint_type, d.joint_T, d.joint_axis = arr(spec.joint_type, np.int32), arr(spec.joint_T, np.float32), arr(spec.joint_axis, np.float32)
        d.lower, d.upper = arr(spec.lower, np.float32), arr(spec.upper, np.float32)
        d.tool_T = arr(spec.tool_T, np.float32)
        # float32 of a seed on a limit may round across it: keep every seed inside the float32 limits
        lo32, hi32 = np.asarray(spec.lower, np.float32), np.asarray(spec.upper, np.float32)
        d.seeds = arr(np.clip(np.asarray(spec.seeds, np.float32), lo32, hi32), np.float32)
        super().__init__("gq_arm_create", "gq_arm_destroy", device, ctypes.byref(d))
        self.N, self.S = spec.n_joints, spec.n_seeds
        # the collision spheres of the arm clearance term (arm_terms), if the spec has any: float32 / int32 on the device
        self.Ns, self.sphere_link, self.sphere_centre, self.sphere_radius = spec.n_spheres, None, None, None
        if spec.n_spheres:
            up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt))).to(self.device)
            self.sphere_link, self.sphere_centre = up(spec.sphere_link, np.int32), up(spec.sphere_centre, np.float32)
            self.sphere_radius = up(spec.sphere_radius, np.float32)
        self.hid = _register_handle(self)


def reach_check(arm, distance=0.10, stations=0, iterations=24, damping=1e-4, rot_scale=0.1, grasp_axis=(0.0, 0.0, 1.0),
                who="reach_terms"):
    """The parameters of the reach term (no GPU): ``arm`` an ArmSpec or ArmHandle (None: not checked), stations in 0..3, a finite
    distance > 0 when there are stations, iterations in 0..4096, finite damping > 0 and rot_scale > 0, a finite non-zero grasp_axis;
    raises ValueError."""
    if arm is not None and not isinstance(arm, (ArmSpec, ArmHandle)):
        raise ValueError(f"{who}: arm must be an ops.ArmSpec or an ops.ArmHandle, got {type(arm).__name__}")
    if int(stations) != stations or not 0 <= int(stations) <= 3:
        raise ValueError(f"{who}: reach_stations = {stations!r} must be an integer in 0..3")
    if int(stations) > 0 and not 0.0 < float(distance) < float("inf"):
        raise ValueError(f"{who}: reach_distance = {distance!r} must be finite and > 0")
    if int(iterations) != iterations or not 0 <= int(iterations) <= 4096:
        raise ValueError(f"{who}: reach_iterations = {iterations!r} must be an integer in 0..4096")
    if not 0.0 < float(damping) < float("inf"):
        raise ValueError(f"{who}: reach_damping = {damping!r} must be finite and > 0")
    if not 0.0 < float(rot_scale) < float("inf"):
        raise ValueError(f"{who}: reach_rot_scale = {rot_scale!r} must be finite and > 0")
    a = _axis3(grasp_axis)
    if not all(abs(x) < float("inf") for x in a) or not any(x != 0.0 for x in a):
        raise ValueError(f"{who}: grasp_axis = {a!r} must be finite and not all zero")


def reach_base(arm_base, n_obj, who="reach_terms"):
    """``arm_base`` (3,4) / (4,4) or (n_obj,3,4) / (n_obj,4,4), numpy or tensor -> float32 CPU tensor (n_obj,3,4); raises ValueError."""
    b = torch.as_tensor(np.asarray(arm_base.detach().cpu()) if torch.is_tensor(arm_base) else np.asarray(arm_base, dtype=np.float64))
    if b.dim() == 2:
        b = b.unsqueeze(0).expand(int(n_obj), *b.shape)
    if b.dim() != 3 or b.shape[0] != int(n_obj) or tuple(b.shape[1:]) not in ((3, 4), (4, 4)):
        raise ValueError(f"{who}: arm_base must be (3,4) or ({n_obj},3,4), got {tuple(b.shape)}")
    if not bool(torch.isfinite(b).all()):
        raise ValueError(f"{who}: arm_base is not finite")
    return b[:, :3, :].to(torch.float32).contiguous()


def _reach_call(arm, hp, Rg, base_T, batch_each, axis, distance, stations, iterations, damping, rot_scale, up, w, e, q, seed,
                accumulate, gRt, st=None):
    p, (B, D) = _dev, hp.shape
    _C.call("gq_reach_terms", arm.handle, _C.f32(hp), D, p(Rg), ctypes.c_int64(B), p(base_T), ctypes.c_int64(B // int(batch_each)),
            ctypes.c_int64(int(batch_each)), ctypes.cast(_axis_c(axis), ctypes.c_void_p), float(distance), int(stations),
            int(iterations), float(damping), float(rot_scale), p(up), float(w), p(e), p(q), p(seed, torch.int32), int(accumulate),
            p(gRt), _C.stream_ptr() if st is None else st)


@_custom_op("graspqp_amd::reach_terms", mutates_args=(), device_types="cuda")
def _reach_op(arm: int, hand_pose: Tensor, Rg: Tensor, base_T: Tensor, batch_each: int, grasp_axis: List[float], distance: float,
              stations: int, iterations: int, damping: float, rot_scale: float) -> Tuple[Tensor, Tensor, Tensor]:
    """-> (E_reach (B), unweighted; reach_q (B,K+1,N), the winning arm configuration per station; reach_seed (B,K+1) int32) of
    the root pose (hand_pose[:, :3], Rg)."""
    a = _handle(arm)
    hp = _c(hand_pose)
    B, dev = hp.shape[0], hp.device
    e, q = torch.empty(B, device=dev), torch.empty(B, stations + 1, a.N, device=dev)
    seed = torch.empty(B, stations + 1, dtype=torch.int32, device=dev)
    _reach_call(a, hp, _c(Rg), _c(base_T), batch_each, grasp_axis, distance, stations, iterations, damping, rot_scale, None, 0.0, e, q,
                seed, 0, None)
    return e, q, seed


@_reach_op.register_fake
def _(arm, hand_pose, Rg, base_T, batch_each, grasp_axis, distance, stations, iterations, damping, rot_scale):
    B = hand_pose.shape[0]
    return (hand_pose.new_empty(B), hand_pose.new_empty(B, stations + 1, _handle(arm).N),
            hand_pose.new_empty(B, stations + 1, dtype=torch.int32))


@_custom_op("graspqp_amd::reach_terms_backward", mutates_args=(), device_types="cuda")
def _reach_bwd_op(arm: int, hand_pose: Tensor, Rg: Tensor, base_T: Tensor, batch_each: int, grasp_axis: List[float], distance: float,
                  stations: int, iterations: int, damping: float, rot_scale: float, g_reach: Tensor) -> Tensor:
    """Upstream row gradients (B) on E_reach -> gRt (B,12) for fk_backward.  One launch (the iteration runs again: the term keeps
    no state)."""
    a = _handle(arm)
    hp = _c(hand_pose)
    gRt = torch.empty(hp.shape[0], 12, device=hp.device)
    _reach_call(a, hp, _c(Rg), _c(base_T), batch_each, grasp_axis, distance, stations, iterations, damping, rot_scale, _c(g_reach), 1.0,
                None, None, None, 0, gRt)
    return gRt


@_reach_bwd_op.register_fake
def _(arm, hand_pose, Rg, base_T, batch_each, grasp_axis, distance, stations, iterations, damping, rot_scale, g_reach):
    return hand_pose.new_empty(hand_pose.shape[0], 12)


class _ReachTerms(torch.autograd.Function):
    """Glue between two registered ops (reach_terms + fk_backward), as _ApproachTerms: the backward launch writes gRt with the
    per-row upstream, the FK backward turns it into the root translation and rotation gradient.  The joints get none."""

    @staticmethod
    def forward(ctx, hand_pose, hand, idx, Rg, LT, ws, arm, base_T, batch_each, axis, par):
        hp = _c(hand_pose.detach())
        e, q, seed = _Eager.reach_terms(arm.hid, hp, Rg, base_T, batch_each, axis, *par)
        ctx.save_for_backward(hp, idx, Rg, LT, ws, base_T)
        ctx.hand, ctx.arm, ctx.par = hand, arm, (batch_each, axis) + tuple(par)
        ctx.mark_non_differentiable(q, seed)
        return e, q, seed

    @staticmethod
    def backward(ctx, g_reach, _gq, _gs):
        hp, idx, Rg, LT, ws, base_T = ctx.saved_tensors
        gRt = _Eager.reach_terms_backward(ctx.arm.hid, hp, Rg, base_T, *ctx.par, _c(g_reach))
        gp = _fk_backward(ctx.hand, hp, idx, Rg, LT, ws, None, None, None, None, gRt, None)
        return (gp,) + (None,) * 10


def reach_terms(hand_pose, hand: HandHandle, idx, Rg, LT, ws, arm: ArmHandle, base_T, batch_each, grasp_axis, distance=0.10,
                stations=0, iterations=24, damping=1e-4, rot_scale=0.1, return_q=False):
    """-> E_reach (B) in m^2 = the mean over the stations k = 0..K of min over the arm's seeds of |e|^2, e = [p* - p(q) ;
    rot_scale log(R* R(q)')] after ``iterations`` damped-least-squares updates of the arm's joints q from the seed (include/
    graspqp_hip.h, "arm reachability", has the iteration); the target of station k is the root pose of ``hand_pose`` moved back by
    ``distance`` k / K along ``grasp_axis`` (hand frame), station 0 the grasp pose itself.  ``base_T`` (n_obj,3,4) places the arm
    base in the frame of each object; row b takes ``base_T[b // batch_each]``.  Unweighted; differentiable w.r.t. the root
    translation and rotation of ``hand_pose`` -- the partial derivative with respect to the target at the final q, which is the
    gradient of the converged energy where the iteration has converged and an approximation elsewhere.  ``idx``, ``Rg``, ``LT``,
    ``ws`` are the kinematic state of ``hand_pose`` (fk_contacts).  ``return_q``: also reach_q (B,K+1,N), the winning configuration
    per station, and reach_seed (B,K+1) int32."""
    if not hand_pose.is_cuda:
        raise RuntimeError("graspqp_amd ops need CUDA (ROCm) tensors; got a CPU tensor")
    if not isinstance(arm, ArmHandle):
        raise ValueError("reach_terms: arm must be an ops.ArmHandle")
    axis = [float(a) for a in _axis3(grasp_axis)]
    reach_check(arm, distance, stations, iterations, damping, rot_scale, axis)
    B = hand_pose.shape[0]
    if int(batch_each) < 1 or B % int(batch_each):
        raise ValueError(f"reach_terms: batch = {B} is not divisible by batch_each = {batch_each}")
    if tuple(base_T.shape) != (B // int(batch_each), 3, 4):
        raise ValueError(f"reach_terms: base_T must be ({B // int(batch_each)}, 3, 4), got {tuple(base_T.shape)}")
    e, q, seed = _ReachTerms.apply(hand_pose, hand, _c(idx, torch.int64), _c(Rg.detach()), _c(LT.detach()), ws, arm,
                                   _c(base_T.detach()), int(batch_each), axis,
                                   (float(distance), int(stations), int(iterations), float(damping), float(rot_scale)))
    return (e, q, seed) if return_q else e


# ----------------------------------------------------------------------------------------------------------
# approach tracking: E_track (csrc/track.hip), damped-least-squares tracking of the straight approach line from ONE start
# configuration, each waypoint warm-started from the one before; ONE launch: eight lanes per row, eight rows per wavefront
# ----------------------------------------------------------------------------------------------------------
def track_check(arm, distance=0.10, waypoints=8, updates=3, damping=1e-4, rot_scale=0.1, grasp_axis=(0.0, 0.0, 1.0), stations=0,
                with_station_q=False, who="track_terms"):
    """The parameters of the tracking term (no GPU): ``arm`` an ArmSpec or ArmHandle (None: not checked), waypoints in 1..64, updates
    in 1..16, finite distance, damping and rot_scale > 0, stations in 0..3 (>= 1 and a divisor of ``waypoints`` when
    ``with_station_q``), a finite non-zero grasp_axis.  Raises ValueError; the library's message (gq_track_check) is kept."""
    if arm is not None and not isinstance(arm, (ArmSpec, ArmHandle)):
        raise ValueError(f"{who}: arm must be an ops.ArmSpec or an ops.ArmHandle, got {type(arm).__name__}")
    for name, v in (("track_waypoints", waypoints), ("track_updates", updates), ("reach_stations", stations)):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f"{who}: {name} = {v!r} must be an integer")
    spec = arm.spec if isinstance(arm, ArmHandle) else arm
    a = _axis3(grasp_axis)
    try:
        _C.call("gq_track_check", 1 if spec is None else int(spec.n_joints), float(distance), int(waypoints), int(updates), float(damping),
                float(rot_scale), int(stations), int(bool(with_station_q)), ctypes.cast(_axis_c(a), ctypes.c_void_p))
    except RuntimeError as err:
        raise ValueError(f"{who}: {err}") from None


def _track_call(arm, hp, Rg, base_T, batch_each, axis, distance, waypoints, updates, damping, rot_scale, q_start, stations, up, w, e,
                q, worst, step, station_q, accumulate, gRt, st=None):
    """``q_start`` (B,N) may be a view with a row stride (``reach_q[:, K]``): it is passed by pointer and stride, without a copy."""
    p, (B, D) = _dev, hp.shape
    if q_start.dim() != 2 or q_start.shape[0] != B or q_start.shape[1] != arm.N or q_start.stride(1) != 1 or q_start.dtype != torch.float32:
        raise ValueError(f"track_terms: q_start must be float32 ({B}, {arm.N}) with unit stride along the joints, got "
                         f"{tuple(q_start.shape)} {q_start.dtype} strides {q_start.stride()}")
    if not q_start.is_cuda:
        raise RuntimeError("graspqp_amd ops need CUDA (ROCm) tensors; got a CPU tensor")
    stride = q_start.stride(0) if B > 1 else arm.N
    _C.call("gq_track_terms", arm.handle, _C.f32(hp), D, p(Rg), ctypes.c_int64(B), p(base_T), ctypes.c_int64(B // int(batch_each)),
            ctypes.c_int64(int(batch_each)), ctypes.cast(_axis_c(axis), ctypes.c_void_p), float(distance), int(waypoints), int(updates),
            float(damping), float(rot_scale), ctypes.c_void_p(q_start.data_ptr()), ctypes.c_int64(int(stride)), int(stations), p(up),
            float(w), p(e), p(q), p(worst), p(step), p(station_q), int(accumulate), p(gRt), _C.stream_ptr() if st is None else st)


@_custom_op("graspqp_amd::track_terms", mutates_args=(), device_types="cuda")
def _track_op(arm: int, hand_pose: Tensor, Rg: Tensor, base_T: Tensor, batch_each: int, grasp_axis: List[float], distance: float,
              waypoints: int, updates: int, damping: float, rot_scale: float, q_start: Tensor,
              stations: int) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """-> (E_track (B), unweighted; track_q (B,T+1,N); track_worst (B); track_step (B); track_station_q (B,K+1,N), empty (B,0,N) for
    stations = 0) of the root pose (hand_pose[:, :3], Rg) from the start configuration q_start (B,N), which may be a strided view."""
    a = _handle(arm)
    hp = _c(hand_pose)
    B, dev = hp.shape[0], hp.device
    e, q = torch.empty(B, device=dev), torch.empty(B, waypoints + 1, a.N, device=dev)
    worst, step = torch.empty(B, device=dev), torch.empty(B, device=dev)
    sq = torch.empty(B, stations + 1 if stations else 0, a.N, device=dev)
    _track_call(a, hp, _c(Rg), _c(base_T), batch_each, grasp_axis, distance, waypoints, updates, damping, rot_scale, q_start, stations,
                None, 0.0, e, q, worst, step, sq if stations else None, 0, None)
    return e, q, worst, step, sq


@_track_op.register_fake
def _(arm, hand_pose, Rg, base_T, batch_each, grasp_axis, distance, waypoints, updates, damping, rot_scale, q_start, stations):
    B, N = hand_pose.shape[0], _handle(arm).N
    return (hand_pose.new_empty(B), hand_pose.new_empty(B, waypoints + 1, N), hand_pose.new_empty(B), hand_pose.new_empty(B),
            hand_pose.new_empty(B, stations + 1 if stations else 0, N))


@_custom_op("graspqp_amd::track_terms_backward", mutates_args=(), device_types="cuda")
def _track_bwd_op(arm: int, hand_pose: Tensor, Rg: Tensor, base_T: Tensor, batch_each: int, grasp_axis: List[float], distance: float,
                  waypoints: int, updates: int, damping: float, rot_scale: float, q_start: Tensor, g_track: Tensor) -> Tensor:
    """Upstream row gradients (B) on E_track -> gRt (B,12) for fk_backward.  One launch (the iteration runs again: the term keeps
    no state)."""
    a = _handle(arm)
    hp = _c(hand_pose)
    gRt = torch.empty(hp.shape[0], 12, device=hp.device)
    _track_call(a, hp, _c(Rg), _c(base_T), batch_each, grasp_axis, distance, waypoints, updates, damping, rot_scale, q_start, 0,
                _c(g_track), 1.0, None, None, None, None, None, 0, gRt)
    return gRt


@_track_bwd_op.register_fake
def _(arm, hand_pose, Rg, base_T, batch_each, grasp_axis, distance, waypoints, updates, damping, rot_scale, q_start, g_track):
    return hand_pose.new_empty(hand_pose.shape[0], 12)


class _TrackTerms(torch.autograd.Function):
    """Glue between two registered ops (track_terms + fk_backward), as _ReachTerms: the backward launch writes gRt with the per-row
    upstream, the FK backward turns it into the root translation and rotation gradient.  The joints and q_start get none."""

    @staticmethod
    def forward(ctx, hand_pose, hand, idx, Rg, LT, ws, arm, base_T, batch_each, axis, q_start, par, stations):
        hp = _c(hand_pose.detach())
        e, q, worst, step, sq = _Eager.track_terms(arm.hid, hp, Rg, base_T, batch_each, axis, *par, q_start, stations)
        ctx.save_for_backward(hp, idx, Rg, LT, ws, base_T, q_start)
        ctx.hand, ctx.arm, ctx.par = hand, arm, (batch_each, axis) + tuple(par)
        ctx.mark_non_differentiable(q, worst, step, sq)
        return e, q, worst, step, sq

    @staticmethod
    def backward(ctx, g_track, *_):
        hp, idx, Rg, LT, ws, base_T, q_start = ctx.saved_tensors
        gRt = _Eager.track_terms_backward(ctx.arm.hid, hp, Rg, base_T, *ctx.par, q_start, _c(g_track))
        gp = _fk_backward(ctx.hand, hp, idx, Rg, LT, ws, None, None, None, None, gRt, None)
        return (gp,) + (None,) * 12


def track_terms(hand_pose, hand: HandHandle, idx, Rg, LT, ws, arm: ArmHandle, base_T, batch_each, grasp_axis, q_start, distance=0.10,
                waypoints=8, updates=3, damping=1e-4, rot_scale=0.1, stations=0, return_path=False):
    """-> E_track (B) in m^2 = the mean over the waypoints i = 0..T of |e_i|^2 along the straight approach line: waypoint i is the
    root pose of ``hand_pose`` moved back by ``distance`` (T - i) / T along ``grasp_axis`` (waypoint 0 the retreated pose, waypoint T
    the grasp pose), the arm starts at ``q_start`` (B,N) -- a strided view such as ``reach_q[:, K]`` is taken without a copy -- and
    every waypoint runs ``updates`` damped-least-squares updates of the reach term from the configuration of the one before
    (include/graspqp_hip.h, "approach tracking").  ``base_T``, ``batch_each``, ``damping``, ``rot_scale`` as in ``reach_terms``.
    Unweighted; differentiable w.r.t. the root translation and rotation of ``hand_pose``: the partial derivative with respect to the
    targets with every q_i held fixed -- the gradient of the converged path energy where every waypoint is at a fixed point with no
    joint on a limit, an approximation elsewhere (finite ``updates``, a clamped joint, the two-cycle out of range).
    ``return_path``: also track_q (B,T+1,N), track_worst (B) = max_i E_i, track_step (B) = the largest joint move between
    neighbouring waypoints, and track_station_q (B,K+1,N) for ``stations`` = K >= 1 dividing T (None for K = 0): the waypoints that
    are the reach term's stations, in the layout of reach_q, for ``arm_terms``."""
    if not hand_pose.is_cuda:
        raise RuntimeError("graspqp_amd ops need CUDA (ROCm) tensors; got a CPU tensor")
    if not isinstance(arm, ArmHandle):
        raise ValueError("track_terms: arm must be an ops.ArmHandle")
    axis = [float(a) for a in _axis3(grasp_axis)]
    track_check(arm, distance, waypoints, updates, damping, rot_scale, axis, stations, int(stations) > 0)
    B = hand_pose.shape[0]
    if int(batch_each) < 1 or B % int(batch_each):
        raise ValueError(f"track_terms: batch = {B} is not divisible by batch_each = {batch_each}")
    if tuple(base_T.shape) != (B // int(batch_each), 3, 4):
        raise ValueError(f"track_terms: base_T must be ({B // int(batch_each)}, 3, 4), got {tuple(base_T.shape)}")
    if tuple(q_start.shape) != (B, arm.N):
        raise ValueError(f"track_terms: q_start must be ({B}, {arm.N}), got {tuple(q_start.shape)}")
    e, q, worst, step, sq = _TrackTerms.apply(hand_pose, hand, _c(idx, torch.int64), _c(Rg.detach()), _c(LT.detach()), ws, arm,
                                              _c(base_T.detach()), int(batch_each), axis, q_start.detach(),
                                              (float(distance), int(waypoints), int(updates), float(damping), float(rot_scale)),
                                              int(stations))
    return (e, q, worst, step, sq if int(stations) else None) if return_path else e


# ----------------------------------------------------------------------------------------------------------
# arm clearance: E_arm (csrc/armscene.hip), the arm's collision spheres on the scene grid at the joints the reach launch has left in
# reach_q; ONE launch: a block per row, a wavefront per station, lane = sphere; the gradient in the gRt layout the FK backward takes
# ----------------------------------------------------------------------------------------------------------
ARM_DEFAULTS = {"margin": 0.0, "damping": 1e-6, "rot_scale": 0.1, "distance": 0.10, "stations": 0}


def _arm_scene_grids(scene, who="arm_terms"):
    if not isinstance(scene, (SceneSDF, SceneSDFSet)):
        raise ValueError(f"{who}: arm scene must be an ops.SceneSDF or an ops.SceneSDFSet, got {type(scene).__name__}")
    return _pregrasp_grids(scene.values, scene.origin, scene.voxel)


def arm_check(arm, grids=None, batch=1, margin=0.0, damping=1e-6, rot_scale=0.1, distance=0.10, stations=0,
              grasp_axis=(0.0, 0.0, 1.0), who="arm_terms"):
    """The parameters of the arm clearance term (no GPU): ``arm`` an ArmSpec or ArmHandle WITH collision spheres; ``grids`` a
    ``_C.ClutterGrids`` (or None: the parameters alone are checked, before a scene exists), ``batch`` divisible by its n_grids; a finite margin >= 0, finite damping > 0 and rot_scale > 0, stations in 0..3, a finite
    distance > 0 when there are stations, a finite non-zero grasp_axis.  Raises ValueError; the library's message (gq_arm_check)
    contains "arm" and names the argument."""
    if not isinstance(arm, (ArmSpec, ArmHandle)):
        raise ValueError(f"{who}: arm must be an ops.ArmSpec or an ops.ArmHandle, got {type(arm).__name__}")
    spec = arm.spec if isinstance(arm, ArmHandle) else arm
    if not spec.n_spheres:
        raise ValueError(f"{who}: the arm has no collision spheres (ArmSpec.with_spheres / with_link_spheres)")
    if int(stations) != stations:
        raise ValueError(f"{who}: arm stations = {stations!r} must be an integer in 0..3")
    G = 1 if grids is None else max(int(grids.n_grids), 1)  # None: gq_arm_check takes a NULL stack and checks the parameters alone
    if int(batch) % G:
        raise ValueError(f"{who}: arm: batch = {batch} is not divisible by n_grids = {G}")
    ax = _axis_c(_axis3(grasp_axis))
    try:
        _C.call("gq_arm_check", None if grids is None else ctypes.byref(grids), ctypes.c_int64(int(batch)), ctypes.c_int64(int(batch) // G), int(spec.n_joints),
                int(spec.n_spheres), float(margin), float(damping), float(rot_scale), float(distance), int(stations),
                ctypes.cast(ax, ctypes.c_void_p))
    except RuntimeError as e:
        raise ValueError(f"{who}: {e}") from None


def _arm_call(arm, grids, margin, damping, rot_scale, hp, Rg, base_T, batch_each, axis, distance, stations, reach_q, up, w, e,
              accumulate, gRt, st=None):
    p, (B, D) = _dev, hp.shape
    _C.call("gq_arm_terms", arm.handle, ctypes.byref(grids), ctypes.c_int64(B // max(grids.n_grids, 1)), float(margin), float(damping),
            float(rot_scale), _C.i32(arm.sphere_link), _C.f32(arm.sphere_centre), _C.f32(arm.sphere_radius), int(arm.Ns), _C.f32(hp), D,
            p(Rg), ctypes.c_int64(B), p(base_T), ctypes.c_int64(B // int(batch_each)), ctypes.c_int64(int(batch_each)),
            ctypes.cast(_axis_c(axis), ctypes.c_void_p), float(distance), int(stations), p(reach_q), p(up), float(w), p(e),
            int(accumulate), p(gRt), _C.stream_ptr() if st is None else st)


@_custom_op("graspqp_amd::arm_terms", mutates_args=(), device_types="cuda")
def _arm_op(arm: int, hand_pose: Tensor, Rg: Tensor, base_T: Tensor, batch_each: int, values: Tensor, origin: List[float],
            voxel: float, grasp_axis: List[float], distance: float, stations: int, reach_q: Tensor, margin: float, damping: float,
            rot_scale: float) -> Tensor:
    """-> E_arm (B), unweighted, in metres: the mean over the stations of the hinge sum of the arm's collision spheres at the joints
    ``reach_q`` (B,K+1,N).  ``values`` is one grid (nx,ny,nz) or a stack (G,nx,ny,nz)."""
    a = _handle(arm)
    hp, v = _c(hand_pose), _c(values)
    e = torch.empty(hp.shape[0], device=hp.device)
    _arm_call(a, _pregrasp_grids(v, origin, voxel), margin, damping, rot_scale, hp, _c(Rg), _c(base_T), batch_each, grasp_axis,
              distance, stations, _c(reach_q), None, 0.0, e, 0, None)
    return e


@_arm_op.register_fake
def _(arm, hand_pose, Rg, base_T, batch_each, values, origin, voxel, grasp_axis, distance, stations, reach_q, margin, damping, rot_scale):
    return hand_pose.new_empty(hand_pose.shape[0])


@_custom_op("graspqp_amd::arm_terms_backward", mutates_args=(), device_types="cuda")
def _arm_bwd_op(arm: int, hand_pose: Tensor, Rg: Tensor, base_T: Tensor, batch_each: int, values: Tensor, origin: List[float],
                voxel: float, grasp_axis: List[float], distance: float, stations: int, reach_q: Tensor, margin: float, damping: float,
                rot_scale: float, g_arm: Tensor) -> Tensor:
    """Upstream row gradients (B) on E_arm -> gRt (B,12) for fk_backward.  One launch."""
    a = _handle(arm)
    hp, v = _c(hand_pose), _c(values)
    gRt = torch.empty(hp.shape[0], 12, device=hp.device)
    _arm_call(a, _pregrasp_grids(v, origin, voxel), margin, damping, rot_scale, hp, _c(Rg), _c(base_T), batch_each, grasp_axis,
              distance, stations, _c(reach_q), _c(g_arm), 1.0, None, 0, gRt)
    return gRt


@_arm_bwd_op.register_fake
def _(arm, hand_pose, Rg, base_T, batch_each, values, origin, voxel, grasp_axis, distance, stations, reach_q, margin, damping, rot_scale,
      g_arm):
    return hand_pose.new_empty(hand_pose.shape[0], 12)


class _ArmTerms(torch.autograd.Function):
    """Glue between two registered ops (arm_terms + fk_backward), as _ReachTerms: the backward launch writes gRt with the per-row
    upstream, the FK backward turns it into the root translation and rotation gradient.  The hand's joints get none."""

    @staticmethod
    def forward(ctx, hand_pose, hand, idx, Rg, LT, ws, arm, base_T, batch_each, scene, axis, reach_q, par):
        hp = _c(hand_pose.detach())
        distance, stations, margin, damping, rot_scale = par
        args = (arm.hid, hp, Rg, base_T, batch_each, scene.values, list(scene.origin), scene.voxel, axis, distance, stations, reach_q,
                margin, damping, rot_scale)
        e = _Eager.arm_terms(*args)
        ctx.save_for_backward(hp, idx, Rg, LT, ws, base_T, scene.values, reach_q)
        ctx.hand, ctx.arm, ctx.args = hand, arm, args
        return e

    @staticmethod
    def backward(ctx, g_arm):
        hp, idx, Rg, LT, ws, base_T, values, reach_q = ctx.saved_tensors
        gRt = _Eager.arm_terms_backward(*ctx.args, _c(g_arm))
        gp = _fk_backward(ctx.hand, hp, idx, Rg, LT, ws, None, None, None, None, gRt, None)
        return (gp,) + (None,) * 12


def arm_terms(hand_pose, hand: HandHandle, idx, Rg, LT, ws, arm: ArmHandle, base_T, batch_each, scene, grasp_axis, reach_q,
              distance=0.10, stations=0, margin=0.0, damping=1e-6, rot_scale=0.1):
    """-> E_arm (B) in metres = the mean over the stations k = 0..K of sum_s max(margin + r_s - phi(x_s), 0): the arm's collision
    spheres (``ArmSpec.with_spheres``) at the arm configuration ``reach_q`` (B,K+1,N) -- what ``reach_terms(..., return_q=True)``
    returned for the same poses and the same ``distance`` / ``stations`` / ``rot_scale`` -- on the grid of ``scene``, an
    ``ops.SceneSDF`` or an ``ops.SceneSDFSet`` (row b reads grid b // (B / G)).  ``base_T`` (n_obj,3,4) as in ``reach_terms``.
    Unweighted; differentiable w.r.t. the root translation and rotation of ``hand_pose`` through the minimum-norm joint motion
    that follows the target, dq = J' (J J' + damping I)^-1 de (include/graspqp_hip.h, "arm clearance": exact along that tracking for
    a reached target with no joint on a limit, an approximation elsewhere).  ``idx``, ``Rg``, ``LT``, ``ws`` are the kinematic state
    of ``hand_pose`` (fk_contacts)."""
    if not hand_pose.is_cuda:
        raise RuntimeError("graspqp_amd ops need CUDA (ROCm) tensors; got a CPU tensor")
    if not isinstance(arm, ArmHandle):
        raise ValueError("arm_terms: arm must be an ops.ArmHandle")
    axis = [float(a) for a in _axis3(grasp_axis)]
    B = hand_pose.shape[0]
    arm_check(arm, _arm_scene_grids(scene), B, margin, damping, rot_scale, distance, stations, axis)
    if int(batch_each) < 1 or B % int(batch_each):
        raise ValueError(f"arm_terms: batch = {B} is not divisible by batch_each = {batch_each}")
    if tuple(base_T.shape) != (B // int(batch_each), 3, 4):
        raise ValueError(f"arm_terms: base_T must be ({B // int(batch_each)}, 3, 4), got {tuple(base_T.shape)}")
    if tuple(reach_q.shape) != (B, int(stations) + 1, arm.N):
        raise ValueError(f"arm_terms: reach_q must be ({B}, {int(stations) + 1}, {arm.N}), got {tuple(reach_q.shape)}")
    return _ArmTerms.apply(hand_pose, hand, _c(idx, torch.int64), _c(Rg.detach()), _c(LT.detach()), ws, arm, _c(base_T.detach()),
                           int(batch_each), scene, axis, _c(reach_q.detach()),
                           (float(distance), int(stations), float(margin), float(damping), float(rot_scale)))


# ----------------------------------------------------------------------------------------------------------
# lift clearance: E_lift, the hand and the held object on the way out (csrc/lift.hip).  One launch; a single grid crosses as
# the stack of one
# ----------------------------------------------------------------------------------------------------------
def lift_direction(direction) -> List[float]:
    """``direction`` normalised once in double: the unit vector the launches use as given.  Raises ValueError for a vector that
    is not three finite numbers or has no length."""
    u = np.asarray(direction.detach().cpu().tolist() if torch.is_tensor(direction) else direction, dtype=np.float64).reshape(-1)
    if u.shape != (3,) or not np.isfinite(u).all() or not np.linalg.norm(u) > 0.0:
        raise ValueError(f"lift: direction = {direction!r} must be three finite numbers, not all zero")
    return [float(x) for x in u / np.linalg.norm(u)]


def lift_check(scene=None, batch=1, n_links=1, n_samples=1, n_obj=None, batch_each=None, n_object_points=0, height=0.05, retreat=0.0,
               stations=4, grasp_axis=(0.0, 0.0, 1.0), direction=(0.0, 0.0, 1.0), margin=0.0, object_margin=0.0, who="lift_terms"):
    """gq_lift_check (host only, no GPU) of the scene (an ``ops.SceneSDF``, an ``ops.SceneSDFSet``, or None: the parameters alone,
    before a scene exists), a launch's shapes and the carry: ``batch`` = n_grids * rows_per_grid = ``n_obj`` * ``batch_each``,
    ``n_object_points`` >= 0, finite ``height`` >= 0 and ``retreat`` >= 0 that are not both zero, ``stations`` in 1..32, a finite
    non-zero ``grasp_axis`` and ``direction`` (used as given), a finite ``margin`` >= 0 and a finite ``object_margin``.  Raises
    ValueError; the library's message contains "lift" and names the argument."""
    if scene is not None and not isinstance(scene, (SceneSDF, SceneSDFSet)):
        raise ValueError(f"{who}: lift: scene must be an ops.SceneSDF or an ops.SceneSDFSet, got {type(scene).__name__}")
    if int(stations) != stations:
        raise ValueError(f"{who}: lift: n_stations = {stations!r} must be an integer in 1..32")
    grids = None if scene is None else _pregrasp_grids(scene.values, scene.origin, scene.voxel)
    G = 1 if grids is None else max(int(grids.n_grids), 1)
    if int(batch) % G:
        raise ValueError(f"{who}: lift: batch = {batch} is not divisible by n_grids = {G}")
    if batch_each is None:
        batch_each = int(batch) if n_obj is None else int(batch) // max(int(n_obj), 1)
    if n_obj is None:
        n_obj = int(batch) // max(int(batch_each), 1)
    ax, u = _axis_c(_axis3(grasp_axis)), _axis_c(_axis3(direction))
    try:
        _C.call("gq_lift_check", None if grids is None else ctypes.byref(grids), ctypes.c_int64(int(batch)),
                ctypes.c_int64(int(batch) // G), int(n_links), ctypes.c_int64(int(n_samples)), ctypes.c_int64(int(n_obj)),
                ctypes.c_int64(int(batch_each)), ctypes.c_int64(int(n_object_points)), float(height), float(retreat), int(stations),
                ctypes.cast(ax, ctypes.c_void_p), ctypes.cast(u, ctypes.c_void_p), float(margin), float(object_margin))
    except RuntimeError as e:
        raise ValueError(f"{who}: {e}") from None


def _lift_call(grids, margin, object_margin, height, retreat, stations, hp, points, link, n_links, Rg, LT, object_points, n_obj,
               batch_each, n_object_points, axis, direction, up_lift, w_lift, e_lift, e_object, accumulate, wrench, gRt, st=None):
    p, (B, D) = _dev, hp.shape
    _C.call("gq_lift_terms", ctypes.byref(grids), ctypes.c_int64(B // max(grids.n_grids, 1)), float(margin), float(object_margin),
            float(height), float(retreat), int(stations), _C.f32(points), p(link, torch.int32), ctypes.c_int64(points.shape[0]),
            int(n_links), _C.f32(hp), D, p(Rg), p(LT), ctypes.c_int64(B), p(object_points) if n_object_points else None,
            ctypes.c_int64(int(n_obj)), ctypes.c_int64(int(batch_each)), ctypes.c_int64(int(n_object_points)),
            ctypes.cast(_axis_c(axis), ctypes.c_void_p), ctypes.cast(_axis_c(direction), ctypes.c_void_p), p(up_lift), float(w_lift),
            p(e_lift), p(e_object), int(accumulate), p(wrench), p(gRt), _C.stream_ptr() if st is None else st)


@_custom_op("graspqp_amd::lift_terms", mutates_args=(), device_types="cuda")
def _lift_op(hand_pose: Tensor, points: Tensor, link: Tensor, n_links: int, Rg: Tensor, LT: Tensor, values: Tensor,
             origin: List[float], voxel: float, grasp_axis: List[float], direction: List[float], height: float, retreat: float,
             stations: int, object_points: Tensor, batch_each: int, margin: float, object_margin: float) -> Tuple[Tensor, Tensor]:
    """-> (E_lift (B), the object's share of it (B)), unweighted: the mean over the stations k = 1..stations of the hinge sums of
    the hand's surface samples and of ``object_points`` (n_obj,M,3) carried by (k / stations) (height direction - retreat R
    grasp_axis).  ``values`` is one grid (nx,ny,nz) or a stack (G,nx,ny,nz).  The kinematic state (Rg, link_T) is the one of
    ``hand_pose``."""
    hp, v, op = _c(hand_pose), _c(values), _c(object_points)
    B = hp.shape[0]
    e, eo = torch.empty(B, device=hp.device), torch.empty(B, device=hp.device)
    _lift_call(_pregrasp_grids(v, origin, voxel), margin, object_margin, height, retreat, stations, hp, _c(points),
               _c(link, torch.int32), n_links, _c(Rg), _c(LT), op, op.shape[0], batch_each, op.shape[1], grasp_axis, direction, None,
               0.0, e, eo, 0, None, None)
    return e, eo


@_lift_op.register_fake
def _(hand_pose, points, link, n_links, Rg, LT, values, origin, voxel, grasp_axis, direction, height, retreat, stations,
      object_points, batch_each, margin, object_margin):
    return hand_pose.new_empty(hand_pose.shape[0]), hand_pose.new_empty(hand_pose.shape[0])


@_custom_op("graspqp_amd::lift_terms_backward", mutates_args=(), device_types="cuda")
def _lift_bwd_op(hand_pose: Tensor, points: Tensor, link: Tensor, n_links: int, Rg: Tensor, LT: Tensor, values: Tensor,
                 origin: List[float], voxel: float, grasp_axis: List[float], direction: List[float], height: float, retreat: float,
                 stations: int, object_points: Tensor, batch_each: int, margin: float, object_margin: float,
                 g_lift: Tensor) -> Tuple[Tensor, Tensor]:
    """Upstream row gradients (B) on E_lift -> (link wrench (B,L,6), gRt (B,12)) for fk_backward.  One launch."""
    hp, v, op = _c(hand_pose), _c(values), _c(object_points)
    B, dev = hp.shape[0], hp.device
    wrench, gRt = torch.empty(B, n_links, 6, device=dev), torch.empty(B, 12, device=dev)
    _lift_call(_pregrasp_grids(v, origin, voxel), margin, object_margin, height, retreat, stations, hp, _c(points),
               _c(link, torch.int32), n_links, _c(Rg), _c(LT), op, op.shape[0], batch_each, op.shape[1], grasp_axis, direction,
               _c(g_lift), 0.0, None, None, 0, wrench, gRt)
    return wrench, gRt


@_lift_bwd_op.register_fake
def _(hand_pose, points, link, n_links, Rg, LT, values, origin, voxel, grasp_axis, direction, height, retreat, stations,
      object_points, batch_each, margin, object_margin, g_lift):
    B = hand_pose.shape[0]
    return hand_pose.new_empty(B, n_links, 6), hand_pose.new_empty(B, 12)


class _LiftTerms(torch.autograd.Function):
    """Glue between two registered ops (lift_terms + fk_backward), as _ApproachTerms.  The object's share comes back beside the
    energy and is not differentiable on its own: its gradient is part of E_lift's."""

    @staticmethod
    def forward(ctx, hand_pose, hand, samples, idx, Rg, LT, ws, scene, object_points, par):
        hp = _c(hand_pose.detach())
        args = (hp, samples.points, samples.link, hand.L, Rg, LT, scene.values, list(scene.origin), scene.voxel) + par[:5] + \
               (object_points,) + par[5:]
        e, eo = _Eager.lift_terms(*args)
        ctx.save_for_backward(hp, idx, Rg, LT, ws, samples.points, samples.link, scene.values, object_points)
        ctx.hand, ctx.args = hand, args
        ctx.mark_non_differentiable(eo)
        return e, eo

    @staticmethod
    def backward(ctx, g_lift, _g_object):
        hp, idx, Rg, LT, ws = ctx.saved_tensors[:5]
        wrench, gRt = _Eager.lift_terms_backward(*ctx.args, _c(g_lift))
        gp = _fk_backward(ctx.hand, hp, idx, Rg, LT, ws, None, None, None, wrench, gRt, None)
        return (gp,) + (None,) * 9


def lift_terms(hand_pose, hand: HandHandle, samples: SurfaceSamples, idx, Rg, LT, ws, scene, grasp_axis, height, retreat, stations,
               object_points, batch_each, direction=(0.0, 0.0, 1.0), margin=0.0, object_margin=0.0, return_object=False):
    """-> E_lift (B) = (1/K) sum over the stations k = 1..K of [ sum over ``samples`` of max(margin - phi(x_w^k), 0) + sum over the
    object's points of max(object_margin - phi(x^{j,k}), 0) ] on the grid of ``scene`` (an ``ops.SceneSDF`` or an
    ``ops.SceneSDFSet``, row b reads grid b // (B / G); it must not contain the target): hand and held object carried together by
    (k / K) (``height`` u - ``retreat`` R a), u = ``direction`` (object frame, normalised here once in double), a = ``grasp_axis``
    (hand frame).  ``object_points`` (n_obj,M,3) in the object's frame, row b carries object b // ``batch_each``; None or M = 0 is
    the hand alone.  ``object_margin`` may be negative.  Unweighted, differentiable w.r.t. ``hand_pose``; ``return_object`` = True
    returns (E_lift, the object's share (B)).  ``idx``, ``Rg``, ``LT``, ``ws`` are the kinematic state of ``hand_pose``
    (fk_contacts); K = ``stations`` in 1..32, ``height`` and ``retreat`` >= 0 in metres, not both zero."""
    if not hand_pose.is_cuda:
        raise RuntimeError("graspqp_amd ops need CUDA (ROCm) tensors; got a CPU tensor")
    if samples.n_links != hand.L:
        raise ValueError(f"lift_terms: the samples refer to {samples.n_links} links, the hand has {hand.L}")
    if not isinstance(scene, (SceneSDF, SceneSDFSet)):
        raise ValueError(f"lift_terms: scene must be an ops.SceneSDF or an ops.SceneSDFSet, got {type(scene).__name__}")
    B = hand_pose.shape[0]
    if int(batch_each) != batch_each or int(batch_each) < 1 or B % int(batch_each):
        raise ValueError(f"lift_terms: batch = {B} is not divisible by batch_each = {batch_each!r}")
    n_obj = B // int(batch_each)
    if object_points is None:
        object_points = hand_pose.new_empty(n_obj, 0, 3)
    if object_points.dim() != 3 or object_points.shape[0] != n_obj or object_points.shape[2] != 3:
        raise ValueError(f"lift_terms: object_points must be ({n_obj}, M, 3), got {tuple(object_points.shape)}")
    axis, u = [float(a) for a in _axis3(grasp_axis)], lift_direction(direction)
    lift_check(scene, B, hand.L, samples.Ns, n_obj, int(batch_each), object_points.shape[1], height, retreat, stations, axis, u, margin,
               object_margin)
    par = (axis, u, float(height), float(retreat), int(stations), int(batch_each), float(margin), float(object_margin))
    e, eo = _LiftTerms.apply(hand_pose, hand, samples, _c(idx, torch.int64), Rg.detach(), LT.detach(), ws, scene,
                             _c(object_points.detach()).to(hand_pose.device), par)
    return (e, eo) if return_object else e


@_custom_op("graspqp_amd::scene_compose", mutates_args=("out_values",), device_types="cuda")
def _scene_compose_op(out_values: Tensor, origin: List[float], voxel: float, target_T: Tensor, part_values: List[Tensor],
                      part_origins: List[float], part_voxels: List[float], part_T: Tensor, exclude: Optional[Tensor],
                      base_values: Optional[Tensor], base_origin: List[float], base_voxel: float, far: float) -> None:
    """gq_clutter_compose: writes out_values (G,nx,ny,nz) in place.  Part p is (part_values[p], part_origins[3p:3p+3],
    part_voxels[p]); the poses (G,12) / (n_parts,12) and exclude (G) int32 are read on the device at launch."""
    n = len(part_values)
    arr = (_C.SceneGrid * max(n, 1))(*(_scene_grid(v, part_origins[3 * p:3 * p + 3], part_voxels[p]) for p, v in enumerate(part_values)))
    base = None if base_values is None else _scene_grid(base_values, base_origin, base_voxel)
    grids = _clutter_grids(out_values, origin, voxel)
    _C.call("gq_clutter_compose", ctypes.byref(grids), _C.f32(out_values), _C.f32(target_T), ctypes.cast(arr, ctypes.c_void_p), n,
            _C.f32(part_T) if n else None, _C.i32(exclude), ctypes.byref(base) if base is not None else None, float(far),
            _C.stream_ptr())


@_scene_compose_op.register_fake
def _(out_values, origin, voxel, target_T, part_values, part_origins, part_voxels, part_T, exclude, base_values, base_origin,
      base_voxel, far):
    return None


@_custom_op("graspqp_amd::tsdf_integrate", mutates_args=("values", "weight"), device_types="cuda")
def _tsdf_integrate_op(values: Tensor, weight: Tensor, origin: List[float], voxel: float, depth: Tensor, labels: Optional[Tensor],
                       cam_T: Tensor, intrinsics: List[float], depth_range: List[float], target_T: Optional[Tensor],
                       skip: Optional[Tensor], trunc: float, max_weight: float) -> None:
    """gq_tsdf_integrate: updates values and weight (G,nx,ny,nz) in place from depth (V,H,W), labels (V,H,W) int32 or None and
    cam_T (V,12); intrinsics = [fx, fy, cx, cy], depth_range = [depth_min, depth_max]; target_T (G,12) or None and skip (G) int32
    or None are read on the device at launch."""
    G, V = values.shape[0], depth.shape[0]
    for t, dtype in ((depth, torch.float32), (labels, torch.int32), (cam_T, torch.float32)):
        _C.ptr(t, dtype)  # CUDA, contiguous, the element type the kernel reads
    if not (values.dim() == 4 and weight.shape == values.shape and depth.dim() == 3 and cam_T.numel() == 12 * V
            and (labels is None or labels.shape == depth.shape) and (target_T is None or target_T.numel() == 12 * G)
            and (skip is None or skip.numel() == G)):
        raise RuntimeError("tsdf_integrate: weight must have values' shape (G,nx,ny,nz), labels depth's (V,H,W), cam_T 12 V floats, "
                           "target_T 12 G floats and skip G entries")
    grids = _clutter_grids(values, origin, voxel)
    views = _depth_views(depth, labels, cam_T, intrinsics, depth_range)
    _C.call("gq_tsdf_integrate", ctypes.byref(grids), _C.f32(values), _C.f32(weight), _C.f32(target_T), ctypes.byref(views),
            _C.i32(skip), float(trunc), float(max_weight), _C.stream_ptr())


@_tsdf_integrate_op.register_fake
def _(values, weight, origin, voxel, depth, labels, cam_T, intrinsics, depth_range, target_T, skip, trunc, max_weight):
    return None


@_custom_op("graspqp_amd::tsdf_surfels", mutates_args=("points", "normals", "count", "workspace"), device_types="cuda")
def _tsdf_surfels_op(values: Tensor, weight: Optional[Tensor], origin: List[float], voxel: float, region: List[int], min_weight: float,
                     trunc: float, points: Optional[Tensor], normals: Optional[Tensor], count: Tensor, workspace: Tensor) -> None:
    """gq_tsdf_surfels: the surfels of values / weight (G,nx,ny,nz) into points, normals (G,capacity,3) and count (G,2) int32;
    region = [i0,i1,j0,j1,k0,k1] or [] for the whole grid; points = normals = None runs the count only.  No gradient."""
    G = values.shape[0]
    if not (values.dim() == 4 and (weight is None or weight.shape == values.shape) and len(region) in (0, 6)
            and (points is None) == (normals is None) and tuple(count.shape) == (G, 2)
            and (points is None or (points.dim() == 3 and points.shape[0] == G and points.shape[2] == 3 and normals.shape == points.shape))):
        raise RuntimeError("tsdf_surfels: weight must have values' shape (G,nx,ny,nz), region 0 or 6 entries, points and normals "
                           "(G,capacity,3) or both None, count (G,2)")
    grids = _clutter_grids(values, origin, voxel)
    need = _size_call("gq_tsdf_surfels_workspace_bytes", ctypes.byref(grids))
    if workspace.numel() * workspace.element_size() < need:
        raise RuntimeError(f"tsdf_surfels: workspace holds {workspace.numel() * workspace.element_size()} bytes, {need} are needed")
    reg = (ctypes.c_int32 * 6)(*(int(r) for r in region)) if len(region) else None
    capacity = 0 if points is None else int(points.shape[1])
    _C.call("gq_tsdf_surfels", ctypes.byref(grids), _C.f32(values), _C.f32(weight), reg, float(min_weight), float(trunc), _C.f32(points),
            _C.f32(normals), ctypes.c_int64(capacity), _C.i32(count), _C.ptr(workspace), _C.stream_ptr())


@_tsdf_surfels_op.register_fake
def _(values, weight, origin, voxel, region, min_weight, trunc, points, normals, count, workspace):
    return None


@_custom_op("graspqp_amd::scene_esdf", mutates_args=("out_values", "workspace"), device_types="cuda")
def _scene_esdf_op(values: Tensor, origin: List[float], voxel: float, trunc: float, max_distance: float, out_values: Tensor,
                   workspace: Tensor) -> None:
    """gq_esdf: the Euclidean distance field of the TSDF stack values (G,nx,ny,nz) into out_values of the same shape (not values'
    memory); workspace holds gq_esdf_workspace_bytes.  No gradient."""
    if not (values.dim() == 4 and out_values.shape == values.shape):
        raise RuntimeError("scene_esdf: values and out_values must be (G,nx,ny,nz) of one shape")
    src, dst = _clutter_grids(values, origin, voxel), _clutter_grids(out_values, origin, voxel)
    need = _size_call("gq_esdf_workspace_bytes", ctypes.byref(src))
    if workspace.numel() * workspace.element_size() < need:
        raise RuntimeError(f"scene_esdf: workspace holds {workspace.numel() * workspace.element_size()} bytes, {need} are needed")
    _C.f32(values)  # CUDA, contiguous, the element type the kernels read
    _C.call("gq_esdf", ctypes.byref(src), ctypes.byref(dst), _C.f32(out_values), float(trunc), float(max_distance), _C.ptr(workspace),
            _C.stream_ptr())


@_scene_esdf_op.register_fake
def _(values, origin, voxel, trunc, max_distance, out_values, workspace):
    return None


@_custom_op("graspqp_amd::self_pen", mutates_args=(), device_types="cuda")
def _self_pen_op(centers: Tensor, hand: int) -> Tuple[Tensor, Tensor]:
    """E_spen (B,) of world sphere centres (B,S,3) and dE/dcentres (hand_model.py:989-1040)."""
    c = _c(centers)
    B = c.shape[0]
    e = torch.empty(B, device=c.device)
    g = torch.empty_like(c)
    _C.call("gq_self_pen_forward", _handle(hand).handle, _C.f32(c), B, 1.0, _C.f32(e), _C.f32(g), _C.stream_ptr())
    return e, g


@_self_pen_op.register_fake
def _(centers, hand):
    return centers.new_empty(centers.shape[0]), torch.empty_like(centers)


def _self_pen_setup(ctx, inputs, output):
    ctx.save_for_backward(output[1])
    ctx.mark_non_differentiable(output[1])


def _self_pen_bwd(ctx, ge, gg):
    (g,) = ctx.saved_tensors
    return g * ge.view(-1, 1, 1), None


torch.library.register_autograd("graspqp_amd::self_pen", _self_pen_bwd, setup_context=_self_pen_setup)


def self_pen(centers, hand: HandHandle):
    if hand.S == 0:
        return torch.zeros(centers.shape[0], device=centers.device)
    return _Eager.self_pen(centers, hand.hid)[0]


# ----------------------------------------------------------------------------------------------------------
# energy terms of the class surface, one launch each (csrc/terms.hip): the forward launch also writes the term's
# derivative, the backward is a broadcast multiply with the upstream row gradient
# ----------------------------------------------------------------------------------------------------------
@_custom_op("graspqp_amd::signed_distance", mutates_args=(), device_types="cuda")
def _signed_distance_op(dist_sq: Tensor, sign: Tensor, normal: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """ObjectModel.cal_distance (object_model.py:222-227): (sqrt(dist_sq + 1e-8) * (-sign), normal * sign, d dis / d dist_sq)."""
    d2, sg, nr = _c(dist_sq), _c(sign, torch.int32), _c(normal)
    dis, nout, g = torch.empty_like(d2), torch.empty_like(nr), torch.empty_like(d2)
    _C.call("gq_signed_distance", _C.f32(d2), _C.i32(sg), _C.f32(nr), d2.numel(), _C.f32(dis), _C.f32(nout), _C.f32(g),
            _C.stream_ptr())
    return dis, nout, g


@_signed_distance_op.register_fake
def _(dist_sq, sign, normal):
    return torch.empty_like(dist_sq), torch.empty_like(normal), torch.empty_like(dist_sq)


def _signed_distance_setup(ctx, inputs, output):
    ctx.save_for_backward(output[2])
    ctx.mark_non_differentiable(output[1], output[2])


def _signed_distance_bwd(ctx, g_dis, g_n, g_g):
    (g,) = ctx.saved_tensors
    return g_dis * g, None, None


torch.library.register_autograd("graspqp_amd::signed_distance", _signed_distance_bwd, setup_context=_signed_distance_setup)


def signed_distance(dist_sq, sign, normal):
    dis, nout, _ = _Eager.signed_distance(dist_sq, sign, normal)
    return dis, nout


@_custom_op("graspqp_amd::energy_dis", mutates_args=(), device_types="cuda")
def _energy_dis_op(distance: Tensor, obj_normal: Tensor, hand_normal: Tensor, with_normals: bool) -> Tuple[Tensor, Tensor, Tensor]:
    """E_dis (energy.py:25-28): with_normals ("gendexgrasp") sum_j exp(1 - (-n_obj . n_hand)) |d|, else sum_j |d|;
    -> (e (B,), d e / d distance (B,n), d e / d hand_normal (B,n,3))."""
    d = _c(distance)
    B, n = d.shape
    e, gd = torch.empty(B, device=d.device), torch.empty_like(d)
    if with_normals:
        on, hn = _c(obj_normal), _c(hand_normal)
        gh = torch.empty_like(hn)
        _C.call("gq_energy_dis", _C.f32(d), _C.f32(on), _C.f32(hn), B, n, _C.f32(e), _C.f32(gd), _C.f32(gh), _C.stream_ptr())
    else:
        gh = d.new_zeros(B, n, 3)
        _C.call("gq_energy_dis", _C.f32(d), None, None, B, n, _C.f32(e), _C.f32(gd), None, _C.stream_ptr())
    return e, gd, gh


@_energy_dis_op.register_fake
def _(distance, obj_normal, hand_normal, with_normals):
    B, n = distance.shape
    return distance.new_empty(B), torch.empty_like(distance), distance.new_empty(B, n, 3)


def _energy_dis_setup(ctx, inputs, output):
    ctx.save_for_backward(output[1], output[2])
    ctx.with_normals = bool(inputs[3])
    ctx.mark_non_differentiable(output[1], output[2])


def _energy_dis_bwd(ctx, ge, g1, g2):
    gd, gh = ctx.saved_tensors
    return ge.unsqueeze(-1) * gd, None, (ge.view(-1, 1, 1) * gh) if ctx.with_normals else None, None


torch.library.register_autograd("graspqp_amd::energy_dis", _energy_dis_bwd, setup_context=_energy_dis_setup)


def energy_dis(distance, obj_normal, hand_normal, with_normals=True):
    return _Eager.energy_dis(distance, obj_normal.detach(), hand_normal, bool(with_normals))[0]


@_custom_op("graspqp_amd::energy_joints", mutates_args=(), device_types="cuda")
def _energy_joints_op(hand_pose: Tensor, lower: Tensor, upper: Tensor) -> Tuple[Tensor, Tensor]:
    """E_joints (energy.py:47-52) over the last len(lower) columns of hand_pose -> (e (B,), d e / d hand_pose (B,D))."""
    hp, lo, hi = _c(hand_pose), _c(lower), _c(upper)
    B, D = hp.shape
    e, g = torch.empty(B, device=hp.device), torch.empty_like(hp)
    _C.call("gq_energy_joints", _C.f32(hp), _C.f32(lo), _C.f32(hi), B, D, lo.numel(), _C.f32(e), _C.f32(g), _C.stream_ptr())
    return e, g


@_energy_joints_op.register_fake
def _(hand_pose, lower, upper):
    return hand_pose.new_empty(hand_pose.shape[0]), torch.empty_like(hand_pose)


def _energy_joints_setup(ctx, inputs, output):
    ctx.save_for_backward(output[1])
    ctx.mark_non_differentiable(output[1])


def _energy_joints_bwd(ctx, ge, g1):
    (g,) = ctx.saved_tensors
    return ge.unsqueeze(-1) * g, None, None


torch.library.register_autograd("graspqp_amd::energy_joints", _energy_joints_bwd, setup_context=_energy_joints_setup)


def energy_joints(hand_pose, lower, upper):
    return _Eager.energy_joints(hand_pose, lower, upper)[0]


@_custom_op("graspqp_amd::energy_pen", mutates_args=(), device_types="cuda")
def _energy_pen_op(distances: Tensor) -> Tensor:
    """E_pen (energy.py:58-61): sum over the surface points of where(distances <= 0, 0, distances) -> (B,)."""
    d = _c(distances)
    B, P = d.shape
    e = torch.empty(B, device=d.device)
    _C.call("gq_energy_pen", _C.f32(d), B, P, _C.f32(e), _C.stream_ptr())
    return e


@_energy_pen_op.register_fake
def _(distances):
    return distances.new_empty(distances.shape[0])


def _energy_pen_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0])


def _energy_pen_bwd(ctx, ge):
    (d,) = ctx.saved_tensors
    return torch.where(d > 0, ge.unsqueeze(-1), ge.new_zeros(()))


torch.library.register_autograd("graspqp_amd::energy_pen", _energy_pen_bwd, setup_context=_energy_pen_setup)


def energy_pen(distances):
    return _Eager.energy_pen(distances)



# ----------------------------------------------------------------------------------------------------------
# grasp-set selection: feasible, ranked, distinct grasps (csrc/select.hip, include/graspqp_hip.h)
# ----------------------------------------------------------------------------------------------------------
class GraspSelection(NamedTuple):
    """Result of ``grasp_select`` (device tensors): ``sel`` (n_obj,K) int32 global row indices in pick order (ascending score),
    unused slots -1; ``n_selected`` (n_obj) int32; ``n_feasible`` (n_obj) int32, not capped by K; ``feasible`` (B) int32 0/1."""
    sel: Tensor
    n_selected: Tensor
    n_feasible: Tensor
    feasible: Tensor


def _grasp_common(hand_pose, Rg, LT, moments):
    hp, Rg, LT, mom = _c(hand_pose), _c(Rg), _c(LT), _c(moments)
    B, L = hp.shape[0], mom.shape[0]
    # fk_contacts gives (B,3,3) and (B,L,3,4), the stepper keeps (B,9) and (B,L,12): the same memory
    if hp.dim() != 2 or Rg.shape[0] != B or Rg.numel() != B * 9 or LT.shape[0] != B or LT.numel() != B * L * 12 or mom.shape != (L, 10):
        raise ValueError(f"grasp_select: hand_pose must be (B,D), Rg ({B},9), LT ({B},{L},12) and the link moments ({L},10), got "
                         f"{tuple(hp.shape)}, {tuple(Rg.shape)}, {tuple(LT.shape)}, {tuple(mom.shape)}")
    nb = _size_call("gq_grasp_select_workspace_bytes", ctypes.c_int64(B), L)
    return hp, Rg, LT, mom, B, L, nb


@_custom_op("graspqp_amd::grasp_distances", mutates_args=(), device_types="cuda")
def _grasp_distances_op(hand_pose: Tensor, Rg: Tensor, LT: Tensor, moments: Tensor, n_samples: int, batch_each: int) -> Tensor:
    """-> (n_obj, batch_each, batch_each): RMS displacement of the hand surface (metres) between every two rows of an object."""
    hp, Rg, LT, mom, B, L, nb = _grasp_common(hand_pose, Rg, LT, moments)
    be = int(batch_each)
    dist = torch.empty(B // max(be, 1), be, be, device=hp.device)
    _C.call("gq_grasp_distances", _C.f32(hp), hp.shape[1], _C.f32(Rg), _C.f32(LT), _C.f32(mom), L, ctypes.c_int64(n_samples),
            ctypes.c_int64(B), ctypes.c_int64(be), _C.f32(dist), _C.ptr(_ws(nb, hp.device)), nb, _C.stream_ptr())
    return dist


@_grasp_distances_op.register_fake
def _(hand_pose, Rg, LT, moments, n_samples, batch_each):
    return hand_pose.new_empty(hand_pose.shape[0] // batch_each, batch_each, batch_each)


@_custom_op("graspqp_amd::grasp_select", mutates_args=(), device_types="cuda")
def _grasp_select_op(hand_pose: Tensor, Rg: Tensor, LT: Tensor, moments: Tensor, n_samples: int, batch_each: int, score: Tensor,
                     terms: Tensor, tol: List[float], k: int, radius: float) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """-> (sel (n_obj,k) int32, n_selected (n_obj) int32, n_feasible (n_obj) int32, feasible (B) int32); the rule is stated in
    include/graspqp_hip.h ("grasp-set selection")."""
    hp, Rg, LT, mom, B, L, nb = _grasp_common(hand_pose, Rg, LT, moments)
    be, k, nT = int(batch_each), int(k), len(tol)
    score, terms = _c(score), _c(terms)
    if score.shape != (B,) or terms.shape != (nT, B):
        raise ValueError(f"grasp_select: score must be ({B}) and terms ({nT},{B}), got {tuple(score.shape)}, {tuple(terms.shape)}")
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=hp.device)
    n_obj = B // max(be, 1)
    sel, n_sel, n_feas, feas = i32(n_obj, max(k, 0)), i32(n_obj), i32(n_obj), i32(B)
    tol_c = (ctypes.c_float * max(nT, 1))(*[float(t) for t in tol])
    _C.call("gq_grasp_select", _C.f32(hp), hp.shape[1], _C.f32(Rg), _C.f32(LT), _C.f32(mom), L, ctypes.c_int64(n_samples),
            ctypes.c_int64(B), ctypes.c_int64(be), _C.f32(score), _C.f32(terms) if nT else None,
            ctypes.cast(tol_c, ctypes.c_void_p), nT, ctypes.c_int64(k), float(radius), _C.i32(sel), _C.i32(n_sel), _C.i32(n_feas),
            _C.i32(feas), _C.ptr(_ws(nb, hp.device)), nb, _C.stream_ptr())
    return sel, n_sel, n_feas, feas


@_grasp_select_op.register_fake
def _(hand_pose, Rg, LT, moments, n_samples, batch_each, score, terms, tol, k, radius):
    B = hand_pose.shape[0]
    i32 = lambda *s: hand_pose.new_empty(*s, dtype=torch.int32)
    return i32(B // batch_each, k), i32(B // batch_each), i32(B // batch_each), i32(B)


def _grasp_check(name, hand_pose, samples):
    if not hand_pose.is_cuda:
        raise RuntimeError("graspqp_amd ops need CUDA (ROCm) tensors; got a CPU tensor")
    if not isinstance(samples, SurfaceSamples):
        raise TypeError(f"{name}: samples must be an ops.SurfaceSamples")


def grasp_distances(hand_pose, Rg, LT, samples: SurfaceSamples, batch_each: int) -> Tensor:
    """-> (n_obj, batch_each, batch_each) float32: d(i,j) = sqrt of the mean over ``samples`` of |x_w,i(s) - x_w,j(s)|^2 for the
    rows i, j of each object (rows object-major), in metres, in closed form from the link moments of ``samples``.  ``Rg`` (B,9)
    and ``LT`` (B,L,12) are the kinematic state of ``hand_pose`` (fk_contacts).  The diagonal is exactly 0 and the matrix exactly
    symmetric.  batch_each <= 4096.  No autograd."""
    _grasp_check("grasp_distances", hand_pose, samples)
    return _Eager.grasp_distances(hand_pose.detach(), Rg.detach(), LT.detach(), samples.link_moments, samples.Ns, int(batch_each))


def grasp_select(hand_pose, Rg, LT, samples: SurfaceSamples, batch_each: int, score, terms, tol, k: int,
                 radius: float) -> GraspSelection:
    """Per object the ``k`` best rows that are feasible and pairwise at least ``radius`` (metres, ``grasp_distances``) apart.
    ``score`` (B): lower is better.  ``terms`` (nT,B) with ``tol`` (nT floats, nT <= 16): row b is feasible iff score[b] is
    finite and terms[t,b] <= tol[t] for every t with tol[t] < inf.  Greedy: pick the best remaining feasible row (ties: the
    smaller row), suppress the remaining rows closer than ``radius`` (strictly; 0 suppresses nothing), at most ``k`` times.
    Fewer than ``k`` is an answer: there is no fill.  Device tensors come back, the host does not wait.  No autograd."""
    _grasp_check("grasp_select", hand_pose, samples)
    tol = [float(t) for t in (tol.tolist() if torch.is_tensor(tol) else tol)]
    if terms is None:
        terms = hand_pose.new_empty(0, hand_pose.shape[0])
    return GraspSelection(*_Eager.grasp_select(hand_pose.detach(), Rg.detach(), LT.detach(), samples.link_moments, samples.Ns,
                                               int(batch_each), score.detach(), terms.detach(), tol, int(k), float(radius)))


# eager routes of the registered ops (see the module docstring)
_eager("sdf_backward", _sdf_backward)
_eager("compute_sdf", _compute_sdf_op, _sdf_bwd, _sdf_setup)
_eager("sdf_meshset", _sdf_meshset_op, _sdf_ms_bwd, _sdf_ms_setup)
_eager("sdf_bvh", _sdf_bvh_op, _sdf_bvh_bwd, _sdf_ms_setup)
_eager("sdf_cloud", _sdf_cloud_op, _sdf_ms_bwd, _sdf_ms_setup)
_eager("box_qp", _box_qp_op, _box_qp_bwd, _box_qp_setup)
_eager("box_qp_backward", _box_qp_bwd_op)
_eager("lsq_box_qp", _lsq_box_qp_op, _lsq_bwd, _lsq_setup)
_eager("lsq_box_qp_backward", _lsq_box_qp_bwd_op)
_eager("fc_energy", _fc_energy_op, _fc_bwd, _fc_setup)
_eager("fc_energy_backward", _fc_energy_bwd_op)
_eager("lsq_box_exact", _lsq_box_exact_op)
_eager("span_exact", _span_exact_op)
_eager("dexgrasp_energy", _dexgrasp_op, _alt_bwd, _alt_setup)
_eager("tdg_energy", _tdg_op, _alt_bwd, _alt_setup)
_eager("fk_contacts", _fk_op, _fk_bwd, _fk_setup)
_eager("fk_backward", _fk_bwd_op)
_eager("hand_pen", _hand_pen_op)
_eager("hand_pen_backward", _hand_pen_bwd_op)
_eager("tabletop_terms", _tabletop_op)
_eager("tabletop_terms_backward", _tabletop_bwd_op)
_eager("scene_distance", _scene_distance_op, _scene_distance_bwd, _scene_distance_setup)
_eager("scene_terms", _scene_op)
_eager("scene_terms_backward", _scene_bwd_op)
_eager("approach_terms", _approach_op)
_eager("approach_terms_backward", _approach_bwd_op)
_eager("scene_distance_set", _scene_distance_set_op, _scene_distance_bwd, _scene_distance_setup)
_eager("scene_terms_set", _scene_set_op)
_eager("scene_terms_set_backward", _scene_set_bwd_op)
_eager("approach_terms_set", _approach_set_op)
_eager("approach_terms_set_backward", _approach_set_bwd_op)
_eager("pregrasp_terms", _pregrasp_op)
_eager("pregrasp_terms_backward", _pregrasp_bwd_op)
_eager("squeeze_terms", _squeeze_op)
_eager("squeeze_terms_backward", _squeeze_bwd_op)
_eager("hold_terms", _hold_op, _hold_bwd, _hold_setup)
_eager("hold_terms_backward", _hold_bwd_op)
_eager("close_fingers", _close_op)
_eager("reach_terms", _reach_op)
_eager("reach_terms_backward", _reach_bwd_op)
_eager("track_terms", _track_op)
_eager("track_terms_backward", _track_bwd_op)
_eager("arm_terms", _arm_op)
_eager("arm_terms_backward", _arm_bwd_op)
_eager("lift_terms", _lift_op)
_eager("lift_terms_backward", _lift_bwd_op)
_eager("scene_compose", _scene_compose_op)
_eager("tsdf_integrate", _tsdf_integrate_op)
_eager("tsdf_surfels", _tsdf_surfels_op)
_eager("scene_esdf", _scene_esdf_op)
_eager("self_pen", _self_pen_op, _self_pen_bwd, _self_pen_setup)
_eager("signed_distance", _signed_distance_op, _signed_distance_bwd, _signed_distance_setup)
_eager("energy_dis", _energy_dis_op, _energy_dis_bwd, _energy_dis_setup)
_eager("energy_joints", _energy_joints_op, _energy_joints_bwd, _energy_joints_setup)
_eager("energy_pen", _energy_pen_op, _energy_pen_bwd, _energy_pen_setup)
_eager("grasp_distances", _grasp_distances_op)
_eager("grasp_select", _grasp_select_op)
