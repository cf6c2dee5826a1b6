"""The scene term's contract (include/graspqp_hip.h, "scene obstacles") written in torch, shared by the scene tests: the test
fields, phi of a grid at world points, and E_scene of an oracle hand with autograd to hand_pose.  Everything runs in the
dtype of its inputs (float64 for the oracle; float32 for the oracle's own rounding noise)."""
import numpy as np
import torch

from ref_cpu import models as omodels

NEAR = 2e-5  # a sample whose phi is closer to the margin than this is too close to ask an fp32 kernel for the oracle's side
FACE = 1e-4  # ... and one closer to a cell face than this, in cell units, for the oracle's cell


class Field:
    """A test grid.  ``origin`` / ``voxel`` are the float32 numbers the struct holds; ``values`` (nx,ny,nz) float32 are phi at
    the nodes; ``analytic`` (x (...,3) -> phi) is set for the fields every cell reproduces exactly."""

    def __init__(self, shape, origin, voxel, values=None, analytic=None):
        self.shape = tuple(int(n) for n in shape)
        self.origin = np.asarray(origin, dtype=np.float32)
        self.voxel = np.float32(voxel)
        self.analytic = analytic
        if values is None:  # the field at the nodes, computed in float64 and rounded once
            values = analytic(self.nodes()).to(torch.float32)
        self.values = torch.as_tensor(values, dtype=torch.float32).contiguous()
        assert self.values.shape == self.shape

    def nodes(self):
        ax = [float(o) + float(self.voxel) * torch.arange(n, dtype=torch.float64) for o, n in zip(self.origin, self.shape)]
        return torch.stack(torch.meshgrid(*ax, indexing="ij"), -1)

    def scene(self, gq):
        return gq.ops.SceneSDF(self.values.cuda(), [float(o) for o in self.origin], float(self.voxel))


def affine(shape, origin, voxel, n=(0.36, -0.48, 0.8), c=0.02):
    """(a) phi = n . x - c with a tilted unit n: grad phi = n everywhere, the choice of cell cannot matter."""
    nv = torch.tensor(n, dtype=torch.float64)
    assert abs(float(nv.norm()) - 1.0) < 1e-12
    return Field(shape, origin, voxel, analytic=lambda x: (x * nv.to(x.dtype)).sum(-1) - c)


def multilinear(shape, origin, voxel, c=(-0.05, 0.5, -0.3, 0.8, 0.7, -0.6, 0.4, 1.5)):
    """(b) phi = c0 + c1 x + c2 y + c3 z + c4 xy + c5 yz + c6 xz + c7 xyz: reproduced exactly by every cell."""
    assert len(set(c)) == 8 and all(v != 0 for v in c)

    def f(p):
        x, y, z = p[..., 0], p[..., 1], p[..., 2]
        return c[0] + c[1] * x + c[2] * y + c[3] * z + c[4] * x * y + c[5] * y * z + c[6] * x * z + c[7] * x * y * z

    return Field(shape, origin, voxel, analytic=f)


def plane(shape, origin, voxel, table_z):
    """phi = z - table_z: E_scene with margin 0 is E_wall."""
    return Field(shape, origin, voxel, analytic=lambda x: x[..., 2] - table_z)


def random_field(shape, origin, voxel, seed, amp=0.03):
    """(c) seeded node values, uniform in [-amp, amp]: the only kind that exposes a wrong cell or an off-by-one."""
    v = (torch.rand(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 2 - 1) * amp
    return Field(shape, origin, voxel, values=v.to(torch.float32))


def locate(field, x):
    """-> (inside (...) bool, cell index (...,3) long, weights f (...,3) in [0,1], u (...,3)) by the contract: u = (x - origin)/h,
    inside iff every u_a is finite and 0 <= u_a <= n_a - 1, i_a = min(floor(u_a), n_a - 2), f_a = u_a - i_a."""
    o = torch.as_tensor(field.origin, dtype=x.dtype)
    n = torch.tensor(field.shape, dtype=x.dtype)
    u = (x - o) / x.new_tensor(float(field.voxel))
    inside = torch.isfinite(x).all(-1) & torch.isfinite(u).all(-1) & ((u >= 0) & (u <= n - 1)).all(-1)
    us = torch.where(inside.unsqueeze(-1), u, torch.zeros_like(u))
    i = torch.minimum(us.detach().floor(), n - 2).clamp_min(0).long()
    return inside, i, us - i.to(x.dtype), u


def phi(field, x, use_grid=None):
    """phi (...) at world points x (...,3): +inf outside the volume, NaN at a non-finite point; differentiable w.r.t. x.
    Inside, the analytic formula where the field has one (unless ``use_grid``), else the trilinear interpolant of the cell."""
    inside, i, f, _ = locate(field, x)
    if field.analytic is not None and not use_grid:
        val = field.analytic(torch.where(inside.unsqueeze(-1), x, torch.zeros_like(x)))
    else:
        v = field.values.to(x.dtype)
        val = 0
        for a in (0, 1):
            for b in (0, 1):
                for c in (0, 1):
                    w = (f[..., 0] if a else 1 - f[..., 0]) * (f[..., 1] if b else 1 - f[..., 1]) * (f[..., 2] if c else 1 - f[..., 2])
                    val = val + w * v[i[..., 0] + a, i[..., 1] + b, i[..., 2] + c]
    out = torch.where(inside, val, torch.full_like(val, float("inf")))
    return torch.where(torch.isfinite(x).all(-1), out, torch.full_like(out, float("nan")))


def hand_oracle(spec, pts, lnk, dtype=torch.float64):
    oh = omodels.OracleHand(spec, dtype)
    oh.surface_points, oh.surface_link = np.asarray(pts, dtype=np.float64), np.asarray(lnk)
    return oh


def e_scene(spec, pts, lnk, hp, field, margin, scale=3.0, dtype=torch.float64, keep=None):
    """-> dict: E (B) E_scene, grad (B,D) d (scale sum E) / d hand_pose, phi (B,Ns), inside (B,Ns), active (B,Ns), face
    (distance of the sample coordinates to the nearest cell face, in cell units), x (B,Ns,3).  ``keep``
    (B,Ns) bool zeroes the contribution of the samples it leaves out."""
    oh = hand_oracle(spec, pts, lnk, dtype)
    hp = hp.detach().to(dtype).clone().requires_grad_()
    oh.set_parameters(hp, torch.zeros(hp.shape[0], 1, dtype=torch.long))
    x = oh.get_surface_points()
    p = phi(field, x)
    inside, _, _, u = locate(field, x.detach())
    hinge = torch.where(inside, torch.relu(margin - torch.where(inside, p, torch.zeros_like(p))), torch.zeros_like(p))
    if keep is not None:
        hinge = torch.where(keep, hinge, torch.zeros_like(hinge))
    E = hinge.sum(-1)
    if E.requires_grad:
        (scale * E).sum().backward()
    ud = u.detach()
    face = (ud - ud.round()).abs().amin(-1)  # outside points too: one just beyond the volume may be inside in float32
    pd = p.detach()
    g = oh.hand_pose.grad
    return dict(E=E.detach().numpy(), grad=(torch.zeros_like(hp) if g is None else g).detach().numpy(), phi=pd.numpy(), inside=inside.numpy(),
                active=(inside & (pd < margin)).numpy(), face=face.numpy(), x=x.detach().numpy())


def guards(res, margin):
    """The two conditions on the INPUTS of a random-field case: no sample coordinate within FACE of a cell face, no sample with
    |phi - margin| < NEAR."""
    ins = res["inside"]
    near = np.abs(res["phi"][ins] - margin).min() if ins.any() else np.inf
    return float(res["face"].min()), float(near)
