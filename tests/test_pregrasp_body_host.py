"""The device bodies of the pre-grasp term (csrc/pregrasp_dev.h: the opened joint value, the station loop of a sample, the fold
task per (node, component), the joint torque) compiled for the HOST with AddressSanitizer and UBSan.  tests/pregrasp_body_host.cpp
walks one block of gq_pregrasp_kernel through them serially, every reduction in the kernel's order, and the float32 results are
held to the fp64 oracle at the bounds of the GPU tests (values rtol 1e-5 / atol 1e-6, gradients norm-wise 1e-4), on their shapes.
Every buffer the program reads is exactly sized, so an index outside one ends the program.  No GPU involved."""
import subprocess

import numpy as np
import pytest
import torch

import ref_cpu  # noqa: F401

import _host_program
import _pregrasp_cases as pc
import _pregrasp_oracle as po
import _scene_oracle as so


@pytest.fixture(scope="module")
def body(tmp_path_factory):
    d = tmp_path_factory.mktemp("pregrasp_body")
    pc.set_synthetic_root(tmp_path_factory.mktemp("synthetic_hands"))
    exe = _host_program.build("pregrasp_body_host", d)

    def run(F, R, t, a, D, margin, alpha, up, K, link_node, node_type, tables, T, W, aw, theta, q_open, pts, lnk):
        depth, child_off, child_idx, max_depth = tables
        L, J = len(link_node), len(node_type)
        f32 = lambda x: np.ascontiguousarray(x, dtype=np.float32).tobytes()
        i32 = lambda x: np.ascontiguousarray(x, dtype=np.int32).tobytes()
        with open(d / "in.bin", "wb") as f:
            f.write(i32(list(F.shape) + [K, len(pts), L, J, max_depth]))
            f.write(f32(list(F.origin) + [F.voxel]))
            f.write(f32(np.concatenate([np.ravel(R), np.ravel(t), np.ravel(a), [D, margin, alpha, up]])))
            f.write(i32(link_node) + i32(node_type) + i32(depth) + i32(child_off) + i32(child_idx))
            f.write(f32(np.asarray(T)[:, :3, :]) + f32(np.asarray(W)[:, :3, :]) + f32(aw))
            f.write(f32(theta) + f32(q_open))
            f.write(f32(pts) + i32(lnk))
            f.write(F.values.numpy().tobytes())
        subprocess.check_call([exe, str(d / "in.bin"), str(d / "out.bin")])
        o = np.fromfile(d / "out.bin", dtype=np.float32)
        assert o.size == 2 * J + 13
        return o[:J].copy(), float(o[J]), o[J + 1:J + 13].astype(np.float64), o[J + 13:].astype(np.float64)

    return run


# the shapes of the GPU tests' table that an uncoupled hand covers with one row, and the synthetic trees (depth 63, 63 children,
# prismatic joints in the interior)
CASES = [("allegro", 63, 3, "random", 0.5, 0.0), ("allegro", 65, 0, "random", 0.5, 0.0), ("allegro", 128, 3, "random", 0.25, 0.01),
         ("allegro", 512, 0, "random", 0.5, 0.0), ("allegro", 512, 3, "multilinear", 0.5, 0.01), ("allegro", 512, 32, "multilinear", 0.5, 0.0),
         ("allegro", 512, 3, "multilinear", 0.0, 0.01), ("allegro", 512, 3, "multilinear", 1.0, 0.01),
         ("shadow_hand", 512, 3, "multilinear", 0.75, 0.01),
         ("chain64", 128, 2, "multilinear", 0.5, 0.01), ("star63", 128, 2, "multilinear", 0.5, 0.01), ("comb43", 128, 2, "multilinear", 0.5, 0.01)]


@pytest.mark.parametrize("name,Ns,K,kind,alpha,margin", CASES)
def test_block_matches_the_oracle(body, name, Ns, K, kind, alpha, margin):
    spec = pc.spec_of(name)
    assert not spec.is_coupled  # C' is a plain product of the kernel; the coupled hands are the GPU tests'
    pts, lnk = pc.samples(name, Ns)
    Ns, D, F, up = len(pts), pc.corridor(K), pc.field(kind), 3.0
    pc.assert_caps(Ns, 1, K, kind)
    hp, ref = pc.guarded(name, Ns, 1, K, D, kind, alpha, margin)
    tag = f"{name} Ns={Ns} K={K} {kind} opening={alpha} margin={margin}"
    pc.assert_guards(ref, margin, tag, Ns, 1, K, kind == "random", alpha)
    q = pc.open_joints(spec)
    theta = hp[0, 9:].numpy()
    theta_o64 = (1.0 - alpha) * theta.astype(np.float64) + alpha * q.astype(np.float64)
    W, T, aw = pc.reduced_frames(spec, theta_o64)
    oh = so.hand_oracle(spec, pts, lnk)
    oh.set_parameters(po.opened_pose(hp.double(), q, alpha), torch.zeros(1, 1, dtype=torch.long))
    # the reduced walk is the oracle's hand, to the float32 round-off of the spec's folded tables (the kernel walks those too)
    np.testing.assert_allclose(T, oh.current_status[0].numpy(), rtol=0, atol=2e-7)
    R, t, a = oh.global_rotation[0].detach().numpy(), hp[0, :3].double().numpy(), oh.grasp_axis.double().numpy()
    theta_o, E, gRt, g_theta = body(F, R, t, a, D, margin, alpha, up, K, spec.link_node, spec.node_type, pc.tree_tables(spec), T, W, aw,
                                    theta, q, pts, lnk)
    # the opened joint value
    np.testing.assert_allclose(theta_o, theta_o64, rtol=2e-7, atol=1e-9)
    if alpha == 0.0:
        assert np.array_equal(theta_o, theta)
    if alpha == 1.0:
        assert np.array_equal(theta_o, q)
    # the oracle's g_w = d hinge / d x_w per station point (upstream 1), g_h = R' g_w, y_k = R' (x_w^k - t)
    x = torch.tensor(ref["x"][0], requires_grad=True)  # (K+1,Ns,3)
    p = so.phi(F, x)
    ins = torch.tensor(ref["inside"][0])
    torch.where(ins, torch.relu(margin - torch.where(ins, p, torch.zeros_like(p))), torch.zeros_like(p)).sum().backward()
    gh = x.grad.numpy() @ R
    y = (ref["x"][0] - t) @ R
    scale = up / (K + 1)
    gsum_ref = -scale * gh.sum((0, 1))
    K9_ref = scale * np.einsum("ksa,ksj->aj", gh, y).ravel()
    gth_ref = ref["grad"][0, 9:]  # the oracle's autograd through the opened pose, scale = up
    gerr = lambda a_, b_: np.linalg.norm(a_ - b_) / max(np.linalg.norm(b_), 1e-300)
    print(f"[{tag}] E err {abs(E - ref['E'][0]):.3e} (E {ref['E'][0]:.3e}), gsum rel err {gerr(gRt[:3], gsum_ref):.3e}, K9 rel err "
          f"{gerr(gRt[3:], K9_ref):.3e}, g_theta rel err {gerr(g_theta, gth_ref):.3e} (norm {np.linalg.norm(gth_ref):.3e})")
    np.testing.assert_allclose(E, ref["E"][0], rtol=1e-5, atol=1e-6)
    assert np.linalg.norm(gRt[:3] - gsum_ref) <= 1e-4 * np.linalg.norm(gsum_ref)
    assert np.linalg.norm(gRt[3:] - K9_ref) <= 1e-4 * np.linalg.norm(K9_ref)
    # d E / d t = -R gsum, against the oracle's autograd through the whole hand
    assert np.linalg.norm(-R @ gRt[:3] - ref["grad"][0, :3]) <= 1e-4 * np.linalg.norm(ref["grad"][0, :3])
    # the joint columns: norm-wise against the WHOLE gradient's norm, the bound of the GPU tests
    assert np.linalg.norm(g_theta - gth_ref) <= 1e-4 * np.linalg.norm(ref["grad"][0])
    if alpha == 1.0:
        assert (g_theta == 0).all() and (gth_ref == 0).all()
    else:
        assert np.linalg.norm(g_theta - gth_ref) <= 1e-4 * np.linalg.norm(gth_ref) / pc.JOINT_SHARE  # and not lost in the whole


def _tiny(body, pts, alpha=0.5, K=2):
    """One revolute joint about z at the origin, one link on it, a 6 x 5 x 4 random grid of 12.5 cm; R = I, t = 0, a = z."""
    F = so.random_field((6, 5, 4), (-0.25, -0.25, -0.125), 0.125, 7)
    eye4 = np.eye(4)
    tables = (np.zeros(1, np.int32), np.array([0, 0], np.int32), np.zeros(0, np.int32), 0)
    pts = np.asarray(pts, dtype=np.float32).reshape(-1, 3)
    return body(F, np.eye(3), np.zeros(3), np.array([0.0, 0.0, 1.0]), 0.3, 0.5, alpha, 1.0, K, [0], [1], tables, eye4[None], eye4[None],
                np.array([[0.0, 0.0, 1.0]]), [0.0], [0.0], pts, np.zeros(len(pts), np.int32))


def test_points_outside_contribute_exactly_nothing(body):
    _, E, gRt, g_theta = _tiny(body, [[0.1, 0.05, 0.2]])  # stations at z = 0.2, 0.05, -0.1: inside the volume
    assert E > 0 and np.isfinite(E) and np.abs(gRt).max() > 0 and np.isfinite(gRt).all() and np.isfinite(g_theta).all()
    _, E2, gRt2, g_theta2 = _tiny(body, [[0.1, 0.05, 0.2], [100.0, 0.0, 0.0], [0.0, 0.0, 3e38], [0.1, 0.2501, 0.2]])
    assert E2 == E and np.array_equal(gRt2, gRt) and np.array_equal(g_theta2, g_theta)  # the bits of the run without them
    _, E3, gRt3, g_theta3 = _tiny(body, [[100.0, 0.0, 0.0], [0.0, -7.0, 0.0]])
    assert E3 == 0 and (gRt3 == 0).all() and (g_theta3 == 0).all()


@pytest.mark.parametrize("bad", [[0.0, np.nan, 0.0], [np.inf, 0.0, 0.0], [0.0, 0.0, -np.inf]])
def test_a_non_finite_point_gives_nan_and_loads_nothing(body, bad):
    _, E, gRt, g_theta = _tiny(body, [[0.1, 0.05, 0.2], bad])  # a load at a non-finite index would end the program
    assert np.isnan(E) and np.isnan(gRt).all() and np.isnan(g_theta).all()


def test_no_station_is_the_grasp_pose_alone(body):
    """K = 0: one station, d = 0, no division by the station count."""
    _, E, gRt, _ = _tiny(body, [[0.1, 0.05, 0.2]], K=0)
    _, E2, _, _ = _tiny(body, [[0.1, 0.05, 0.2]], K=2)
    assert np.isfinite(E) and E > 0 and np.isfinite(gRt).all() and E != E2
