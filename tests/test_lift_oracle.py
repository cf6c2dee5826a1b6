"""The fp64 oracle of the lift term (tests/_lift_oracle.py) against what it must reduce to: the approach oracle with no height and
no object, a pure lift whose object share cannot depend on the pose, a central difference, and the closed form on an affine field.
No GPU involved."""
import numpy as np
import torch

import ref_cpu  # noqa: F401

import _approach_oracle as ao
import _lift_oracle as lo
import _scene_oracle as so
from graspqp_amd.hands import get_hand_spec
from graspqp_amd.utils import meshes

G_SHAPE, G_ORIGIN, G_H = (100, 96, 104), (-0.5, -0.48, -0.52), 0.01
H, D, U = 0.05, 0.08, (0.0, 0.6, 0.8)


def _pose(spec, B, seed, spread=0.1):
    gen = torch.Generator().manual_seed(seed)
    t = spread * torch.randn(B, 3, generator=gen)
    th = torch.tensor(spec.default_state)[None] + 0.3 * torch.randn(B, spec.n_dofs, generator=gen)
    return torch.cat([t, torch.randn(B, 6, generator=gen), th], 1).double()


def _hand(Ns=96):
    spec = get_hand_spec("allegro")
    pts, lnk = meshes.hand_surface_samples(spec, 512)
    pick = np.random.default_rng(Ns).permutation(512)[:Ns]
    return spec, pts[pick], lnk[pick]


def _sphere(n_obj, M, seed, radius=0.04):
    P = np.random.default_rng(seed).standard_normal((n_obj, M, 3))
    return radius * P / np.linalg.norm(P, axis=-1, keepdims=True)


def test_no_height_and_no_object_is_the_approach_oracle():
    spec, pts, lnk = _hand()
    F = so.multilinear(G_SHAPE, G_ORIGIN, G_H)
    hp = _pose(spec, 3, 5)
    for K in (1, 4):
        a = ao.e_approach(spec, pts, lnk, hp, F, 0.01, D, K)
        l = lo.e_lift(spec, pts, lnk, hp, F, 0.01, 0.0, 0.0, D, K, U, np.zeros((1, 0, 3)), 3)
        assert a["E"].max() > 0
        np.testing.assert_allclose(l["E"], a["E"], rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(l["grad"], a["grad"], rtol=1e-12, atol=1e-12)
        assert (l["E_object"] == 0).all() and np.array_equal(l["hand"]["active"], a["active"])


def test_pure_lift_object_share_has_no_gradient_and_is_equal_across_rows():
    spec, pts, lnk = _hand()
    F = so.random_field(G_SHAPE, G_ORIGIN, G_H, 11)
    hp = _pose(spec, 4, 6)
    P = _sphere(2, 50, 1)
    l = lo.e_lift(spec, pts, lnk, hp, F, 0.0, 0.0, H, 0.0, 3, U, P, 2)
    assert (l["E_object"] > 0).all() and (l["grad_object"] == 0).all()
    assert l["E_object"][0] == l["E_object"][1] and l["E_object"][2] == l["E_object"][3] and l["E_object"][0] != l["E_object"][2]
    assert np.abs(l["grad"]).max() > 0  # the hand's part does depend on the pose
    # with a retreat the object's share does depend on the rotation, and only on it
    l = lo.e_lift(spec, pts, lnk, hp, F, 0.0, 0.0, H, D, 3, U, P, 2)
    assert np.abs(l["grad_object"][:, 3:9]).max() > 0 and (l["grad_object"][:, :3] == 0).all() and (l["grad_object"][:, 9:] == 0).all()


def test_gradient_matches_a_central_difference():
    spec, pts, lnk = _hand(48)
    F = so.random_field(G_SHAPE, G_ORIGIN, G_H, 11)
    K, h = 3, 1e-6
    P = _sphere(1, 40, 2)
    for seed in range(200):  # a pose whose station points keep h-proof distances from the cell faces and from the margins
        hp = _pose(spec, 1, seed)
        ref = lo.e_lift(spec, pts, lnk, hp, F, 0.0, 0.0, H, D, K, U, P, 1, scale=1.0)
        face, near = lo.guards(ref, 0.0, 0.0)
        if face >= 3 * lo.FACE and near >= lo.NEAR and ref["hand"]["active"].any() and ref["object"]["active"].any():  # 3 x: the step h is FACE itself
            break
    else:
        raise AssertionError("no seeded pose passes the guards")
    fd = np.zeros_like(ref["grad"][0])
    for i in range(hp.shape[1]):
        e = []
        for s in (+1, -1):
            q = hp.clone()
            q[0, i] += s * h
            e.append(lo.e_lift(spec, pts, lnk, q, F, 0.0, 0.0, H, D, K, U, P, 1)["E"][0])
        fd[i] = (e[0] - e[1]) / (2 * h)
    err = np.linalg.norm(fd - ref["grad"][0]) / np.linalg.norm(ref["grad"][0])
    print(f"central difference h={h}: rel err {err:.3e}")
    assert err <= 1e-6


def test_affine_field_closed_form():
    spec, pts, lnk = _hand()
    F = so.affine(G_SHAPE, G_ORIGIN, G_H)
    B, K, m_h, m_o = 3, 4, 0.01, 0.005
    hp = _pose(spec, B, 7)
    P = _sphere(1, 64, 3)
    l = lo.e_lift(spec, pts, lnk, hp, F, m_h, m_o, H, D, K, U, P, B)
    assert l["hand"]["inside"].all() and l["object"]["inside"].all() and l["hand"]["active"].any() and l["object"]["active"].any()
    at_pose = so.e_scene(spec, pts, lnk, hp, F, m_h)
    oh = so.hand_oracle(spec, pts, lnk)
    oh.set_parameters(hp, torch.zeros(B, 1, dtype=torch.long))
    n, c0 = np.array([0.36, -0.48, 0.8]), 0.02
    slope = H * (n @ np.array(U)) - D * ((oh.global_rotation @ oh.grasp_axis).numpy() @ n)  # (B): H n.u - D n.(R a)
    hand = sum(np.maximum(m_h - (at_pose["phi"] + (k / K) * slope[:, None]), 0.0).sum(-1) for k in range(1, K + 1)) / K
    obj = sum(np.maximum(m_o - ((P[0] @ n - c0)[None] + (k / K) * slope[:, None]), 0.0).sum(-1) for k in range(1, K + 1)) / K
    np.testing.assert_allclose(l["E_object"], obj, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(l["E"], hand + obj, rtol=1e-9, atol=1e-12)
