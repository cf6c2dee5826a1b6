"""The device bodies of the lift term (csrc/lift_dev.h: the stations of one hand surface sample and of one object point, the loops a
lane of gq_lift_kernel runs) compiled for the HOST with AddressSanitizer and UBSan, run as a stand-alone program, and compared with
the fp64 oracle at the inputs and the bounds of the GPU tests (tests/test_gpu_lift.py: values rtol 1e-5 / atol 1e-6, gradients
norm-wise 1e-4).  The buffer the program reads is exactly the grid, so a node read outside it ends the program.  No GPU involved."""
import subprocess

import numpy as np
import pytest
import torch

import ref_cpu  # noqa: F401

import _host_program
import _scene_oracle as so
import test_gpu_lift as tg  # the seeded inputs of the GPU tests and their guards; nothing of it touches a GPU here
from graspqp_amd.hands import get_hand_spec


@pytest.fixture(scope="module")
def body(tmp_path_factory):
    d = tmp_path_factory.mktemp("lift_body")
    exe = _host_program.build("lift_body_host", d)

    def run(field, R, t, a, u, H, D, m_h, m_o, K, xh, P):
        xh = np.ascontiguousarray(xh, dtype=np.float32).reshape(-1, 3)
        P = np.ascontiguousarray(P, dtype=np.float32).reshape(-1, 3)
        with open(d / "in.bin", "wb") as f:
            f.write(np.array(field.shape, dtype=np.int32).tobytes())
            f.write(np.array(list(field.origin) + [field.voxel], dtype=np.float32).tobytes())
            f.write(np.concatenate([np.ravel(R), np.ravel(t), np.ravel(a), np.ravel(u), [H, D, m_h, m_o]]).astype(np.float32).tobytes())
            f.write(np.array([K, len(xh), len(P)], dtype=np.int32).tobytes())
            f.write(field.values.numpy().tobytes())
            f.write(xh.tobytes())
            f.write(P.tobytes())
        subprocess.check_call([exe, str(d / "in.bin"), str(d / "out.bin")])
        o = np.fromfile(d / "out.bin", dtype=np.float32).reshape(-1, 13).astype(np.float64)
        hand, obj = o[:len(xh)], o[len(xh):]
        return (hand[:, 0], hand[:, 1:4], hand[:, 4:].reshape(-1, 3, 3)), (obj[:, 0], obj[:, 1:4], obj[:, 4:].reshape(-1, 3, 3))

    return run


def _hinge_grad(F, x, inside, margin):
    """g_w = d hinge / d x per station point (upstream 1): -grad phi at the active points, zero elsewhere."""
    x = torch.tensor(x, requires_grad=True)
    if x.numel() == 0:
        return torch.zeros_like(x)
    p = so.phi(F, x)
    ins = torch.tensor(inside)
    torch.where(ins, torch.relu(margin - torch.where(ins, p, torch.zeros_like(p))), torch.zeros_like(p)).sum().backward()
    return x.grad


CASES = [c for c in tg.TABLE if c[0] == "allegro"] + [("allegro", 128, 128, 1, 3, "multilinear", 0.01, -0.01)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v) for v in c[1:]))
def test_station_loops_match_the_oracle(body, case):
    hand_name, Ns, M, B, K, kind = case[:6]
    m_h, m_o = case[6:] if len(case) > 6 else (0.0, 0.0)
    H, D, U = tg.H0, tg.D0, np.array(tg.U0)
    spec = get_hand_spec(hand_name)
    pts, lnk = tg._samples(hand_name, Ns)
    F = tg._field(kind)
    hp, P, ref, _ = tg._guarded(hand_name, Ns, M, B, K, kind, m_h, m_o)
    tg._assert_guards(ref, m_h, m_o, str(case), Ns, M, B, K, kind == "random")
    oh = so.hand_oracle(spec, pts, lnk)
    oh.set_parameters(hp.double(), torch.zeros(B, 1, dtype=torch.long))
    a = oh.grasp_axis.double()
    d = D * torch.arange(1, K + 1, dtype=torch.float64) / K
    for b in range(B):
        R, t = oh.global_rotation[b].detach(), hp[b, :3].double()
        xh = (oh.get_surface_points()[b].detach() - t) @ R  # R' (x_w - t), row-wise
        (eh, G, K9h), (eo, Go, K9o) = body(F, R.numpy(), t.numpy(), a.numpy(), U, H, D, m_h, m_o, K, xh.numpy(), P[0])
        E, Eo = (eh.sum() + eo.sum()) / K, eo.sum() / K
        gh = _hinge_grad(F, ref["hand"]["x"][b], ref["hand"]["inside"][b], m_h) @ R  # (K,Ns,3): g_h = R' g_w
        go = _hinge_grad(F, ref["object"]["x"][b], ref["object"]["inside"][b], m_o) @ R  # (K,M,3)
        y = xh[None] - d[:, None, None] * a
        G_ref = gh.sum(0).numpy()
        K9_ref = (torch.einsum("ksa,ksj->aj", gh, y) + torch.einsum("ksa,kj->aj", go, -d[:, None] * a[None])).numpy()
        K9 = K9h.sum(0) + K9o.sum(0)
        print(f"[{case} row {b}] E err {abs(E - ref['E'][b]):.3e} (E {ref['E'][b]:.3e}), object share err {abs(Eo - ref['E_object'][b]):.3e}, "
              f"G rel err {np.linalg.norm(G - G_ref) / np.linalg.norm(G_ref):.3e}, K9 rel err "
              f"{np.linalg.norm(K9 - K9_ref) / np.linalg.norm(K9_ref):.3e}")
        np.testing.assert_allclose(E, ref["E"][b], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(Eo, ref["E_object"][b], rtol=1e-5, atol=1e-6)
        assert (Go == 0).all()  # the object has no gsum and no wrench
        assert np.linalg.norm(G - G_ref) <= 1e-4 * np.linalg.norm(G_ref)
        assert np.linalg.norm(K9 - K9_ref) <= 1e-4 * np.linalg.norm(K9_ref)
        # d E / d t = (1/K) R sum g_h of the hand alone, against the oracle's autograd through the whole hand (scale 3)
        g_t = 3.0 * (R.numpy() @ G.sum(0)) / K
        assert np.linalg.norm(g_t - ref["grad"][b, :3]) <= 1e-4 * np.linalg.norm(ref["grad"][b, :3])


def test_points_outside_add_nothing_and_non_finite_points_give_nan(body):
    F = so.random_field((6, 5, 4), (-0.25, -0.25, -0.125), 0.125, 7)
    eye, zero, a, u = np.eye(3), np.zeros(3), np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.0, 0.0])
    pts = np.array([[0.0, 0.0, 0.2], [100.0, 0.0, 0.0], [0.0, np.nan, 0.0], [np.inf, 0.0, 0.0], [0.0, 0.0, 3e38], [-0.2, 0.0, 0.0]],
                   dtype=np.float32)
    # stations at z - 0.05 k and x + 0.1 k: the first point leaves the volume through its side, the last through its bottom
    (eh, G, K9h), (eo, Go, K9o) = body(F, eye, zero, a, u, 0.4, 0.2, 0.5, 0.5, 4, pts, pts)
    for e, K9 in ((eh, K9h), (eo, K9o)):
        assert e[0] > 0 and np.isfinite(e[0]) and np.isfinite(K9[0]).all()
        assert e[1] == 0 and (K9[1] == 0).all()  # outside: free space, exactly nothing
        assert np.isnan(e[2]) and np.isnan(e[3]) and np.isnan(K9[2]).any()  # non-finite: NaN, nothing loaded
        assert e[4] == 0  # finite but far outside
        assert e[5] > 0 and np.isfinite(e[5])
    assert (G[1] == 0).all() and np.isnan(G[2]).all() and (Go == 0).all()
    # same points, same carry: hand and object see the same stations when R = I and t = 0, so their energies agree to rounding
    np.testing.assert_allclose(eh[[0, 5]], eo[[0, 5]], rtol=1e-5)
