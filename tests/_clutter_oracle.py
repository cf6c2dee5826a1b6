"""The compose contract (include/graspqp_hip.h, "clutter scenes") written in torch fp64, on top of tests/_scene_oracle.py, and
the layouts the compose tests share: node (g,i,j,k) of target g is min(far, base(x_w) if inside, phi_p(R_p'(x_w - t_p)) if inside,
p != exclude[g]) at x_w = R_g (origin + h (i,j,k)) + t_g.  Poses are (n,3,4) [R|t]; the float32 numbers a kernel is given are the
inputs, everything after them is float64."""
import numpy as np
import torch

import _scene_oracle as so

EDGE = 1e-4  # a part-frame coordinate closer than this (in cells) to a volume's boundary plane u = 0 or u = n - 1: the inside
#              rule jumps there, and an fp32 kernel cannot be asked for the oracle's side


def rotation(gen):
    """A general rotation from a seeded unit quaternion, float64."""
    q = torch.nn.functional.normalize(torch.randn(4, generator=gen, dtype=torch.float64), dim=0)
    w, x, y, z = (float(v) for v in q)
    return torch.tensor([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                         [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], dtype=torch.float64)


def poses(n, seed, spread):
    """(n,3,4) float32 [R|t]: general rotations (rounded to float32: used as given), translations uniform in +-spread."""
    gen = torch.Generator().manual_seed(seed)
    T = torch.zeros(n, 3, 4, dtype=torch.float64)
    for k in range(n):
        T[k, :, :3] = rotation(gen)
        T[k, :, 3] = (torch.rand(3, generator=gen, dtype=torch.float64) * 2 - 1) * spread
    return T.to(torch.float32)


def identity(n):
    T = torch.zeros(n, 3, 4, dtype=torch.float32)
    T[:, :, :3] = torch.eye(3)
    return T


def centred(shape, voxel, shift=(0.0, 0.0, 0.0)):
    """Origin of a grid whose volume is centred on ``shift``."""
    return tuple(float(s) - 0.5 * float(np.float32(voxel)) * (n - 1) for n, s in zip(shape, shift))


class Out:
    """Geometry of the output stack (no values)."""

    def __init__(self, n_grids, shape, origin, voxel):
        self.n_grids, self.shape = int(n_grids), tuple(int(n) for n in shape)
        self.origin, self.voxel = np.asarray(origin, dtype=np.float32), np.float32(voxel)

    def nodes(self):
        ax = [float(o) + float(self.voxel) * torch.arange(n, dtype=torch.float64) for o, n in zip(self.origin, self.shape)]
        return torch.stack(torch.meshgrid(*ax, indexing="ij"), -1)


def compose(out, target_T, parts, part_T, exclude=None, base=None, far=0.02, use_grid=None):
    """-> (phi (G,nx,ny,nz) float64, info): info["edge"] is the smallest distance (cells) of a part-frame coordinate of an
    (node, included part or base) pair to that volume's boundary planes u = 0 and u = n - 1; info["inside"] the fraction of (node, included part) pairs inside."""
    tT, pT = target_T.to(torch.float64), part_T.to(torch.float64)
    xf = out.nodes()
    phi = torch.full((out.n_grids,) + out.shape, float(far), dtype=torch.float64)
    edge, n_in, n_pairs = float("inf"), 0, 0

    def edge_of(field, q):
        n = torch.tensor(field.shape, dtype=torch.float64)
        u = (q - torch.as_tensor(field.origin, dtype=torch.float64)) / float(field.voxel)
        return float(torch.minimum(u.abs(), (u - (n - 1)).abs()).min())  # to the two boundary planes of every axis

    for g in range(out.n_grids):
        xw = xf @ tT[g, :, :3].T + tT[g, :, 3]
        fin = torch.isfinite(xw).all(-1)
        val = phi[g]
        if base is not None:
            val = torch.minimum(val, so.phi(base, xw, use_grid))
            if fin.all():
                edge = min(edge, edge_of(base, xw))
        for p, F in enumerate(parts):
            if exclude is not None and int(exclude[g]) == p:
                continue
            q = (xw - pT[p, :, 3]) @ pT[p, :, :3]  # R' (x - t)
            v = so.phi(F, q, use_grid)
            val = torch.minimum(val, v)  # propagates a NaN
            if torch.isfinite(q).all():
                edge = min(edge, edge_of(F, q))
                n_in += int(torch.isfinite(v).sum())
                n_pairs += v.numel()
        phi[g] = torch.where(fin, val, torch.full_like(val, float("nan")))
    return phi, dict(edge=edge, inside=n_in / max(n_pairs, 1))


# the layout of the GPU compose cases (and of the host build's): three targets, three parts, a base
G, OUT_SHAPE, OUT_H, FAR = 3, (7, 6, 9), 0.0125, 0.02
PART_SHAPES, PART_H = ((5, 4, 3), (4, 6, 5), (2, 2, 2)), (0.02, 0.015, 0.05)
BASE_SHAPE, BASE_H = (6, 7, 5), 0.03
EXCLUDE = (0, -1, 2)
OUT_SHAPE_TILES = (5, 9, 17)  # two tiles of 4 x 4 x 16 nodes along x and z, three along y, none of them full
SEEDS = (2, 3)  # the random case's admissible seeds among the first six, chosen on the CPU (the tests assert the guards)


def layout(seed, kind, out_shape=OUT_SHAPE):
    """-> (out, target_T, parts, part_T, exclude, base) of the case: ``kind`` "affine" (oracle: the closed form) or "random"."""
    out = Out(G, out_shape, centred(out_shape, OUT_H), OUT_H)
    target_T, part_T = poses(G, 100 + seed, 0.01), poses(len(PART_SHAPES), 200 + seed, 0.015)
    normals = ((0.36, -0.48, 0.8), (-0.6, 0.0, 0.8), (0.48, 0.64, -0.6))
    parts = []
    for p, (shape, h) in enumerate(zip(PART_SHAPES, PART_H)):
        o = centred(shape, h)
        parts.append(so.affine(shape, o, h, n=normals[p], c=0.004 * p) if kind == "affine" else so.random_field(shape, o, h, 300 + 10 * seed + p))
    ob = centred(BASE_SHAPE, BASE_H, (0.004, -0.003, 0.002))
    base = so.affine(BASE_SHAPE, ob, BASE_H, n=(0.0, 0.6, 0.8), c=-0.01) if kind == "affine" else so.random_field(BASE_SHAPE, ob, BASE_H, 399 + seed)
    return out, target_T, parts, part_T, torch.tensor(EXCLUDE, dtype=torch.int32), base
