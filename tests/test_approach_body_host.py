"""The device body of the approach term (csrc/approach_dev.h: the stations of one hand surface sample, the loop a lane of
gq_approach_kernel runs) compiled for the HOST with AddressSanitizer and UBSan and compared with the fp64 oracle, at the bounds
of the GPU tests (values rtol 1e-5 / atol 1e-6, gradients norm-wise 1e-4).  The buffer the program reads is exactly the grid, so
a node read outside it ends the program.  No GPU involved."""
import subprocess

import numpy as np
import pytest
import torch

import ref_cpu  # noqa: F401

import _approach_oracle as ao
import _host_program
import _scene_oracle as so
from graspqp_amd.hands import get_hand_spec
from graspqp_amd.utils import meshes

G_SHAPE, G_ORIGIN, G_H = (100, 96, 104), (-0.5, -0.48, -0.52), 0.01


def _build(tmp_path_factory, name, flags=()):
    d = tmp_path_factory.mktemp(name)
    exe = _host_program.build("approach_body_host", d, flags)

    def run(field, R, t, a, D, margin, K, xh):
        xh = np.ascontiguousarray(xh, dtype=np.float32).reshape(-1, 3)
        with open(d / "in.bin", "wb") as f:
            f.write(np.array(field.shape, dtype=np.int32).tobytes())
            f.write(np.array(list(field.origin) + [field.voxel], dtype=np.float32).tobytes())
            f.write(np.concatenate([np.ravel(R), np.ravel(t), np.ravel(a), [D, margin]]).astype(np.float32).tobytes())
            f.write(np.array([K, len(xh)], dtype=np.int32).tobytes())
            f.write(field.values.numpy().tobytes())
            f.write(xh.tobytes())
        subprocess.check_call([exe, str(d / "in.bin"), str(d / "out.bin")])
        o = np.fromfile(d / "out.bin", dtype=np.float32).reshape(-1, 13)
        run.raw = o.copy()  # the float32 results of the last call, for the comparison of the two forms
        o = o.astype(np.float64)
        return o[:, 0], o[:, 1:4], o[:, 4:].reshape(-1, 3, 3)

    return run


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    """The loop the kernel is built with."""
    return _build(tmp_path_factory, "approach_body")


@pytest.fixture(scope="module")
def rotated(tmp_path_factory):
    """The variant build of approach_dev.h: split body, loads of station k + 1 issued before station k is consumed."""
    return _build(tmp_path_factory, "approach_body_rotated", ("-DGQ_APPROACH_ROTATED",))


@pytest.fixture(scope="module")
def body(plain, rotated):
    """Both forms on the same inputs: the rotated one must give the plain one's bits; -> the plain one's results."""
    def run(*args):
        out = plain(*args)
        rotated(*args)
        assert plain.raw.tobytes() == rotated.raw.tobytes(), "the two forms of the station loop differ"
        return out

    return run


def _pose(spec, B, seed, spread=0.1):
    gen = torch.Generator().manual_seed(seed)
    t = spread * torch.randn(B, 3, generator=gen)
    th = torch.tensor(spec.default_state)[None] + 0.3 * torch.randn(B, spec.n_dofs, generator=gen)
    return torch.cat([t, torch.randn(B, 6, generator=gen), th], 1).float()


CASES = [(63, 4, 0.08, "random", 0.0), (128, 4, 0.08, "random", 0.01), (512, 1, 0.08, "random", 0.0),
         (512, 3, 0.08, "multilinear", 0.01), (65, 8, 0.10, "multilinear", 0.01), (128, 4, 0.08, "affine", 0.01),
         (512, 32, 0.10, "multilinear", 0.0)]


@pytest.mark.parametrize("Ns,K,D,kind,margin", CASES)
def test_station_loop_matches_the_oracle(body, Ns, K, D, kind, margin):
    spec = get_hand_spec("allegro")
    pts, lnk = meshes.hand_surface_samples(spec, 512)
    if Ns < 512:
        pick = np.random.default_rng(Ns).permutation(512)[:Ns]
        pts, lnk = pts[pick], lnk[pick]
    F = {"affine": so.affine, "multilinear": so.multilinear}[kind](G_SHAPE, G_ORIGIN, G_H) if kind != "random" else \
        so.random_field(G_SHAPE, G_ORIGIN, G_H, 11)
    for seed in range(100 + Ns, 300 + Ns):  # one row; the conditions of tests/test_gpu_approach.py on the inputs
        hp = _pose(spec, 1, seed)
        ref = ao.e_approach(spec, pts, lnk, hp.double(), F, margin, D, K, scale=1.0)
        face, near = ao.guards(ref, margin)
        if (face >= ao.FACE or kind != "random") and near >= ao.NEAR and ref["active"].sum() >= 5 and ref["active"].any(axis=(0, 2)).all():
            break
    else:
        raise AssertionError("no seeded pose passes the guards")
    oh = so.hand_oracle(spec, pts, lnk)
    oh.set_parameters(hp.double(), torch.zeros(1, 1, dtype=torch.long))
    R, t, a = oh.global_rotation[0].detach(), hp[0, :3].double(), oh.grasp_axis.double()
    xw0 = oh.get_surface_points()[0].detach()
    xh = (xw0 - t) @ R  # R' (x_w - t), row-wise
    # the oracle's g_w = d hinge / d x_w per station point, g_h = R' g_w; then G, K9 and E of the row
    x = torch.tensor(ref["x"][0], requires_grad=True)  # (K,Ns,3)
    p = so.phi(F, x)
    ins = torch.tensor(ref["inside"][0])
    torch.where(ins, torch.relu(margin - torch.where(ins, p, torch.zeros_like(p))), torch.zeros_like(p)).sum().backward()
    gw = x.grad  # g_w = -grad phi at the active points: the gradient of the hinge w.r.t. the point (upstream 1)
    gh = gw @ R
    d = D * torch.arange(1, K + 1, dtype=torch.float64) / K
    y = xh[None] - d[:, None, None] * a
    G_ref = gh.sum(0).numpy()  # (Ns,3)
    K9_ref = torch.einsum("ksa,ksj->saj", gh, y).numpy()
    e, G, K9 = body(F, R.numpy(), t.numpy(), a.numpy(), D, margin, K, xh.numpy())
    E = e.sum() / K
    print(f"[{kind} Ns={Ns} K={K}] E err {abs(E - ref['E'][0]):.3e} (E {ref['E'][0]:.3e}), G rel err "
          f"{np.linalg.norm(G - G_ref) / np.linalg.norm(G_ref):.3e}, K9 rel err {np.linalg.norm(K9 - K9_ref) / np.linalg.norm(K9_ref):.3e}")
    np.testing.assert_allclose(E, ref["E"][0], rtol=1e-5, atol=1e-6)
    assert np.linalg.norm(G - G_ref) <= 1e-4 * np.linalg.norm(G_ref)
    assert np.linalg.norm(K9 - K9_ref) <= 1e-4 * np.linalg.norm(K9_ref)
    # d E / d t = (1/K) R sum g_h, against the oracle's autograd through the whole hand
    g_t = (R.numpy() @ G.sum(0)) / K
    assert np.linalg.norm(g_t - ref["grad"][0, :3]) <= 1e-4 * np.linalg.norm(ref["grad"][0, :3])


def test_station_points_outside_and_non_finite(body):
    F = so.random_field((6, 5, 4), (-0.25, -0.25, -0.125), 0.125, 7)
    eye, zero, a = np.eye(3), np.zeros(3), np.array([0.0, 0.0, 1.0])
    xh = np.array([[0.0, 0.0, 0.2], [100.0, 0.0, 0.0], [0.0, np.nan, 0.0], [np.inf, 0.0, 0.0], [0.0, 0.0, 3e38]], dtype=np.float32)
    e, G, K9 = body(F, eye, zero, a, 0.6, 0.5, 4, xh)  # stations at z - 0.15, -0.3, -0.45, -0.6: the first sample leaves the volume
    assert e[0] > 0 and np.isfinite(e[0]) and np.isfinite(K9[0]).all()
    assert e[1] == 0 and (G[1] == 0).all() and (K9[1] == 0).all()  # outside: free space
    assert np.isnan(e[2]) and np.isnan(e[3]) and np.isnan(G[2]).all()  # non-finite: NaN, nothing loaded
    assert e[4] == 0  # finite but far outside
