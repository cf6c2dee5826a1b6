"""The synthetic-hand builder of tests/_synthetic_hand.py, without a GPU: sizes of every topology (they are the reason the
topology exists), the orderings gq_hand_create insists on, and the fold of fixed joints -- oracle FK on the unfolded frame
tree (oracle/ref_cpu/kin.py) against a plain numpy fp64 walk of the reduced node tree, to 1e-12."""
import numpy as np
import pytest
import torch

from ref_cpu import kin as okin  # noqa: E402

import _synthetic_hand as sh  # noqa: E402


@pytest.fixture(scope="module")
def specs(tmp_path_factory):
    root = tmp_path_factory.mktemp("synthetic_hands")
    return {name: sh.build(name, root) for name in sh.TOPOLOGIES}


def _depth(spec):
    d = []
    for p in spec.node_parent:
        d.append(0 if p < 0 else d[p] + 1)
    return max(d)


def _n_groups(spec):
    sl = np.asarray(spec.sphere_link)
    return 0 if len(sl) == 0 else 1 + int((sl[1:] != sl[:-1]).sum())


# name -> (tree joints, actuated joints, links, spheres, sphere groups, depth of the reduced tree)
_SIZES = dict(chain64=(64, 64, 64, 256, 64, 63), star63=(64, 64, 64, 65, 18, 1), comb43=(43, 43, 49, 41, 17, 10),
              coupled12=(12, 5, 13, 26, 13, 2), coupled12_dense=(12, 5, 13, 26, 13, 2), nospheres=(5, 5, 6, 0, 0, 2))


@pytest.mark.parametrize("name", sh.TOPOLOGIES)
def test_sizes_and_orderings(specs, name):
    spec = specs[name]
    N, JA, L, S, NG, depth = _SIZES[name]
    assert (spec.n_nodes, spec.n_dofs, spec.n_links, spec.n_spheres, _n_groups(spec), _depth(spec)) == (N, JA, L, S, NG, depth)
    assert spec.n_contact_candidates == 2 * L
    assert spec.node_parent.shape == (N,) and spec.node_pre.shape == (N, 4, 4) and spec.node_axis.shape == (N, 3)
    assert spec.node_type.shape == (N,) and spec.link_node.shape == (L,) and spec.link_offset.shape == (L, 4, 4)
    assert spec.coupling.shape == (N, JA) and spec.coupling_offset.shape == (N,)
    assert spec.joints_lower.shape == (JA,) and (spec.joints_lower < spec.joints_upper).all()
    assert spec.sphere.shape == (spec.n_spheres, 4) and spec.sphere_link.shape == (spec.n_spheres,)
    assert all(-1 <= p < j for j, p in enumerate(spec.node_parent)), "node_parent must be topologically sorted"
    assert (np.diff(spec.sphere_link) >= 0).all(), "sphere_link must be non-decreasing"
    assert ((spec.cand_link >= 0) & (spec.cand_link < L)).all() and (np.diff(spec.cand_link) >= 0).all()
    assert set(np.unique(spec.node_type)) <= {1, 2} and (spec.node_type == 2).any(), "every hand has a prismatic joint"
    np.testing.assert_allclose(np.linalg.norm(spec.node_axis, axis=1), 1.0, atol=1e-6)


def test_what_each_topology_is_for(specs):
    c, s, m = specs["chain64"], specs["star63"], specs["comb43"]
    # chain64: one chain, prismatic joints in its interior, a link on the base, fixed joints folded away, 320 items at n = 64
    assert np.array_equal(c.node_parent, np.arange(-1, 63)) and c.link_node[0] == -1
    assert (c.node_type[1:-1] == 2).sum() >= 30 and len(c.frame_names) > 1 + 64, "fixed frames must exist to be folded"
    assert np.array_equal(np.bincount(c.sphere_link), [4] * 64) and 64 + c.n_spheres == 320
    assert not np.allclose(c.node_pre[2, :3, :3], np.asarray(c.frame_origin)[c.frame_dof.tolist().index(2), :3, :3]), \
        "the fixed joint before joint 2 must show in node_pre"
    # star63: 63 children of node 0; S = 65 = one sphere in the second stride; 18 groups = one group in the second scan pass
    assert s.node_parent[0] == -1 and (s.node_parent[1:] == 0).all()
    assert s.n_spheres == 65 and _n_groups(s) - 1 == 17
    # comb43: 258 fold tasks; 16 scanned groups
    assert m.n_nodes * 6 == 258 and _n_groups(m) - 1 == 16 and (m.link_node == -1).sum() == 1
    assert not np.allclose(m.link_offset[-1], np.eye(4)), "a fingertip link rides on a fixed joint below its node"
    # coupled hands: multipliers of both signs, offsets, and in the dense variant rows with two sources
    k, kd = specs["coupled12"], specs["coupled12_dense"]
    assert (k.coupling < 0).any() and (k.coupling_offset != 0).any() and ((k.coupling != 0).sum(1) == 1).all()
    assert ((kd.coupling != 0).sum(1) == 2).sum() == 3 and kd.is_coupled
    assert np.array_equal(k.node_pre, kd.node_pre)


@pytest.mark.parametrize("name", sh.TOPOLOGIES)
def test_reduced_tree_equals_frame_tree(specs, name):
    """The fold: fp64 FK of the oracle on frame_* against fp64 FK on node_* / link_*, on random joint values in and beyond
    the limits.  1e-12 holds because the generated URDFs keep the float32 tables of the spec exact under the fold."""
    spec = specs[name]
    r = np.random.RandomState(7)
    theta = np.asarray(spec.default_state, np.float64)[None] + 0.5 * sh.joint_scale(spec)[None] * r.standard_normal((5, spec.n_dofs))
    T_frames = okin.forward_kinematics(spec, torch.tensor(theta, dtype=torch.float64)).numpy()
    T_nodes = sh.reduced_forward_kinematics(spec, theta)
    assert T_frames.shape == T_nodes.shape == (5, spec.n_links, 4, 4)
    err = np.abs(T_frames - T_nodes).max()
    print(f"{name}: reduced tree vs frame tree, max abs {err:.3g}")
    assert err <= 1e-12
    assert np.abs(T_nodes[:, :, :3, 3]).max() > 0.01, "the hand must have moved away from the origin"


def test_layout_hands_hold_the_requested_sphere_groups(tmp_path):
    for sizes in ([1, 1], [3] * 6 + [5] * 8 + [1] * 3 + [9]):
        spec = sh.layout(tmp_path, sizes)
        assert np.array_equal(np.bincount(spec.sphere_link), sizes) and spec.n_links == len(sizes)
        assert (spec.sphere[:, 3] >= 0.005).all() and (spec.sphere[:, 3] <= 0.015).all()
    spec = sh.layout(tmp_path, [2, 2], radii=[0.005] * 4)
    assert (spec.sphere[:, 3] == np.float32(0.005)).all()
