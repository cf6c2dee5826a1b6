"""The device body of the scene term (csrc/scene_dev.h: cell, weights, value and gradient of the trilinear interpolant, the
code both scene kernels inline) compiled for the HOST with AddressSanitizer and UBSan and compared with the fp64 oracle, at the
bounds of the GPU tests (values rtol 1e-5 / atol 1e-6, gradients norm-wise 1e-4).  The vector-holding buffer is exactly the grid,
so a node read outside it, or a float -> int conversion of an out-of-range value, ends the program.  No GPU involved."""
import os
import subprocess

import numpy as np
import pytest
import torch

import _host_program
import _scene_oracle as so
from graspqp_amd.hands import get_hand_spec



@pytest.fixture(scope="module")
def body(tmp_path_factory):
    d = tmp_path_factory.mktemp("scene_body")
    exe = _host_program.build("scene_body_host", d)

    def run(field, x):
        x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, 3)
        with open(d / "in.bin", "wb") as f:
            f.write(np.array(field.shape, dtype=np.int32).tobytes())
            f.write(np.array(list(field.origin) + [field.voxel], dtype=np.float32).tobytes())
            f.write(np.array([len(x)], dtype=np.int32).tobytes())
            f.write(field.values.numpy().tobytes())
            f.write(x.tobytes())
        subprocess.check_call([exe, str(d / "in.bin"), str(d / "out.bin")])
        o = np.fromfile(d / "out.bin", dtype=np.float32).reshape(-1, 5)
        return o[:, 0], o[:, 1:4], o[:, 4].astype(int)

    return run


def _fields(shape, origin, voxel, seed):
    return {"affine": so.affine(shape, origin, voxel), "multilinear": so.multilinear(shape, origin, voxel),
            "random": so.random_field(shape, origin, voxel, seed)}


def _special_points():
    """The (5,4,3) grid of the GPU query test (node positions exact in float32) and its special points."""
    shape, origin, h = (5, 4, 3), (-0.25, -0.25, -0.125), 0.125
    lo, hi = np.array(origin), np.array(origin) + h * (np.array(shape) - 1)
    f32, up, dn = np.float32, np.float32(np.inf), np.float32(-np.inf)
    inside = [lo + h * np.array(ijk) for ijk in ((1, 2, 1), (0, 0, 0), (4, 3, 2), (3, 0, 2))]
    inside += [(hi[0], -0.1, 0.03), (0.1, hi[1], -0.06), (-0.2, 0.05, hi[2])]  # on the last node plane of each axis
    outside = [(np.nextafter(f32(hi[0]), up), -0.1, 0.03), (0.1, np.nextafter(f32(hi[1]), up), -0.06),
               (-0.2, 0.05, np.nextafter(f32(hi[2]), up)), (np.nextafter(f32(lo[0]), dn), 0.0, 0.0), (100.0, 0.0, 0.0),
               (0.0, -1e30, 0.0), (0.0, 0.0, 3e38)]
    nonfinite = [(0.0, np.nan, 0.0), (np.inf, 0.0, 0.0), (0.0, 0.0, -np.inf)]
    rnd = np.random.default_rng(3).uniform(lo - 0.05, hi + 0.05, (240, 3))
    x = np.concatenate([rnd, np.array(inside, dtype=np.float64), np.array(outside, dtype=np.float64), np.array(nonfinite)]).astype(np.float32)
    return shape, origin, h, x, (np.arange(240, 247), np.arange(247, 254), np.arange(254, 257))


@pytest.mark.parametrize("kind", ["affine", "multilinear", "random"])
def test_body_on_the_special_points(body, kind):
    shape, origin, h, x, (i_in, i_out, i_nan) = _special_points()
    F = _fields(shape, origin, h, 7)[kind]
    phi, grad, where = body(F, x)
    x64 = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    ref = so.phi(F, x64)
    ins, _, _, u = so.locate(F, x64.detach())
    ref[torch.isfinite(ref)].sum().backward()
    ins, rphi, rgrad = ins.numpy(), ref.detach().numpy(), x64.grad.numpy()
    ur = u.numpy()[:240]
    assert np.abs(ur - np.round(ur)).min() >= so.FACE  # a guard on the inputs: the seeded points stay clear of the cell faces
    assert np.array_equal(where == 1, ins) and ins[i_in].all()
    assert (where[i_out] == 0).all() and np.isposinf(phi[i_out]).all() and (grad[i_out] == 0).all()
    assert (where[i_nan] == 2).all() and np.isnan(phi[i_nan]).all()
    np.testing.assert_allclose(phi[ins], rphi[ins], rtol=1e-5, atol=1e-6)
    assert np.linalg.norm(grad[ins] - rgrad[ins]) <= 1e-4 * np.linalg.norm(rgrad[ins])
    nodes = i_in[:4]
    ijk = np.round((x[nodes] - np.array(origin)) / h).astype(int)
    np.testing.assert_allclose(phi[nodes], F.values.numpy()[ijk[:, 0], ijk[:, 1], ijk[:, 2]], rtol=0, atol=1e-7)


@pytest.mark.parametrize("kind", ["affine", "multilinear", "random"])
def test_body_on_the_hand_samples_of_the_sphere_fixture(body, golden_dir, kind):
    g = np.load(os.path.join(golden_dir, "energy_allegro_sphere_b4_n4.npz"), allow_pickle=False)
    spec = get_hand_spec("allegro")
    origin, h = (-0.40137, -0.40291, -0.40173), 0.01
    F = _fields((62, 64, 80) if kind == "random" else (80, 80, 80), origin, h, 5)[kind]
    hp0 = torch.tensor(g["opt_hand_pose"], dtype=torch.float32)
    for dz in (0.0, 0.1, 0.15):
        hp = hp0.clone()
        hp[:, 2] += dz
        for margin in (0.0, 0.01):
            ref = so.e_scene(spec, g["opt_surface_points"], g["opt_surface_link"], hp.double(), F, margin, scale=3.0)
            face, near = so.guards(ref, margin)
            assert face >= so.FACE and near >= so.NEAR and ref["active"].sum() >= 5 and ref["inside"].all()
            xs = ref["x"].astype(np.float32)  # the oracle's sample positions, rounded once: what a kernel would hold
            phi, grad, where = (a.reshape(xs.shape[:2] + a.shape[1:]) for a in body(F, xs.reshape(-1, 3)))
            act = (where == 1) & ~(phi >= margin)
            assert np.array_equal(act, ref["active"])
            E = np.where(act, margin - phi.astype(np.float64), 0.0).sum(-1)
            g_t = 3.0 * np.where(act[..., None], -grad.astype(np.float64), 0.0).sum(1)  # d (3 E) / d translation = sum g_w
            np.testing.assert_allclose(E, ref["E"], rtol=1e-5, atol=1e-6)
            assert np.linalg.norm(g_t - ref["grad"][:, :3]) <= 1e-4 * np.linalg.norm(ref["grad"][:, :3])
