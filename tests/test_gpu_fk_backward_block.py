"""gq_fk_backward as one block of four wavefronts per row: grad_pose against the fp64 oracle for every shape at which the
block takes another path (one / many / more than 64 items, more than 128 fold tasks, the coupled hand, each optional input
absent, the glue route of ops._HandPen), and bit for bit against the outputs the parent commit's single-wavefront kernel
gave on the same inputs (tests/golden/fk_backward_parent_bits.npz, written by tools/make_golden_fk_backward.py).

Oracle loss (fkb.oracle_grad), fp64 autograd through oracle/ref_cpu: sum(cp . g_cpts) + sum(cn . g_cnrm) + sum(spheres . g_spheres) + sum(R . g_R)
+ sum(theta . g_theta) + a linear energy on link-fixed points (its hand-frame link wrenches (f, x cross f) are the kernel's
g_wrench) + a linear energy on world points seen from the hand frame (its [gsum, K] is the kernel's g_Rt) + w_joints E_joints
when the energy tail rides along.  Tolerances: those of test_gpu_parity.py::test_fk_contacts_forward_backward (1e-4 on the
norm, rtol 2e-3 / atol 2e-4 per element) and, for the penetration route, of test_hand_penetration_and_self_penetration (2e-3)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ref_cpu import models as omodels  # noqa: E402

import _fk_backward_case as fkb  # noqa: E402
from graspqp_amd.hands import get_hand_spec  # noqa: E402
from graspqp_amd.utils import meshes  # noqa: E402


@pytest.fixture(scope="module")
def gq():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from graspqp_amd import _C, ops

    _C.lib()
    return type("gq", (), {"ops": ops, "C": _C})


_hands = {}


def _hand(gq, name):
    if name not in _hands:
        _hands[name] = gq.ops.HandHandle(get_hand_spec(name))
    return _hands[name]


def _check(gq, hand_name, B, n, seed, present=fkb.GRAD_INPUTS, tail=True):
    """fkb.check (tests/_fk_backward_case.py, shared with the synthetic hands of test_gpu_kinematics_limits.py) on a shipped
    hand, with the fixed tolerances."""
    fkb.check(gq.C, get_hand_spec(hand_name), _hand(gq, hand_name), B, n, seed, present=present, tail=tail)


@pytest.mark.parametrize("n", [1, 12, 70])  # 70 contacts + the spheres: more than 64 items, the second pass of the item loop
def test_allegro_item_counts(gq, n):
    _check(gq, "allegro", 5, n, 40 + n)


def test_shadow_hand_more_tasks_than_two_wavefronts(gq):
    spec = get_hand_spec("shadow_hand")
    assert spec.n_nodes * 6 > 128
    _check(gq, "shadow_hand", 3, 16, 51)


def test_ability_hand_coupled_path(gq):
    assert get_hand_spec("ability_hand").is_coupled
    _check(gq, "ability_hand", 3, 12, 52)


@pytest.mark.parametrize("absent", fkb.GRAD_INPUTS)
def test_allegro_each_optional_input_absent(gq, absent):
    _check(gq, "allegro", 5, 12, 53, present=tuple(k for k in fkb.GRAD_INPUTS if k != absent), tail=False)


def test_allegro_only_wrench_and_gRt(gq):
    _check(gq, "allegro", 5, 12, 54, present=("g_wrench", "g_Rt"), tail=False)


def test_hand_pen_glue_route(gq):
    """ops._HandPen: the penetration query's link wrenches and [gsum, K] are the only inputs of the FK backward."""
    from graspqp_amd.core.hand_model import HandModel
    from graspqp_amd.core.object_model import ObjectModel

    spec = get_hand_spec("allegro")
    B, P = 5, 200
    fv = meshes.icosphere(2, 0.05)
    sp = meshes.surface_points(fv, P, oversample=4)
    inp = fkb.make_inputs(spec, B, 4, 55)
    hp = torch.tensor(inp["hand_pose"], dtype=torch.float64)
    hp[:, :3] *= 0.25  # the hand in and around the object -> many penetrating points
    idx = torch.tensor(inp["idx"])
    oh = omodels.OracleHand(spec, torch.float64)
    oo = omodels.OracleObject([fv], [sp], B, torch.float64)
    hpo = hp.clone().requires_grad_()
    oh.set_parameters(hpo, idx)
    dis_o = oh.cal_distance(oo.surface_points_tensor)
    assert (dis_o > 1e-4).sum() > 20, "test scene must contain penetrating points"
    torch.relu(dis_o).sum().backward()
    hm = HandModel(spec, "cuda")
    om = ObjectModel(batch_size_each=B, num_samples=P)
    om.initialize_from_meshes([fv], surface_points_list=[sp])
    hm.set_parameters(hp.float().cuda().requires_grad_(), idx.cuda())
    torch.relu(hm.cal_distance(om.surface_points_each)).sum().backward()
    go, gg = oh.hand_pose.grad.numpy(), hm.hand_pose.grad.cpu().numpy()
    nrm = np.linalg.norm(gg - go) / np.linalg.norm(go)
    print(f"hand_pen glue route: norm-wise {nrm:.3g}")
    assert nrm < 2e-3


@pytest.mark.parametrize("tag", ["n12", "n70"])
def test_bits_equal_the_parent_kernel(gq, golden_dir, tag):
    z = np.load(os.path.join(golden_dir, "fk_backward_parent_bits.npz"), allow_pickle=False)
    inp = {k[len(tag) + 4:]: z[k] for k in z.files if k.startswith(tag + ".in.")}
    ref = {k[len(tag) + 5:]: z[k] for k in z.files if k.startswith(tag + ".out.")}
    assert set(ref) >= {"grad_pose", "e_dis", "e_joints", "total", "accept", "pose", "grad", "idx", "terms"}
    assert 0 < ref["accept"].sum() < len(ref["accept"]), "the fixture must hold accepted and refused rows"
    out = fkb.run_backward(gq.C, _hand(gq, "allegro"), inp)
    bits = lambda a: a.view(np.uint32) if a.dtype == np.float32 else a
    for k, v in ref.items():
        assert out[k].dtype == v.dtype and np.array_equal(bits(out[k]), bits(v)), f"{tag}: {k} differs from the parent's bits"
