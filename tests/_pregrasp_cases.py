"""Inputs of the pre-grasp tests, shared by tests/test_pregrasp_body_host.py (CPU) and tests/test_gpu_pregrasp.py: the grid and
fields of tests/test_gpu_approach.py, its pose generator and seeded search (at most 200 seeds) with the guards of the pre-grasp
term, and an fp64 walk of the reduced tree that also returns the node frames.  The oracle's results are computed once per case and
shared.  Nothing here needs a GPU.

Guards: conditions on the INPUTS, computed by the fp64 oracle over all B Ns (K+1) station points -- on the random field no
coordinate within FACE of a cell face; on every field no |phi - margin| < NEAR; at least min(5, Ns B) active points and one at
every station; for opening < 1 and Ns > 1 the oracle's joint columns carry at least 5e-3 of the gradient norm.
Caps: B Ns (K+1) <= 512 on the random field (beyond a few thousand points no seed in 200 passes NEAR there) and <= 4 096 on the
smooth ones; K = 32 stands on its own with B = 1."""
import functools

import numpy as np
import torch

import _pregrasp_oracle as po
import _scene_oracle as so
import _synthetic_hand as sh
from graspqp_amd.hands import get_hand_spec
from graspqp_amd.utils import meshes

G_SHAPE, G_ORIGIN, G_H = (100, 96, 104), (-0.5, -0.48, -0.52), 0.01
JOINT_SHARE = 5e-3
SYNTHETIC = ("chain64", "star63", "comb43", "coupled12_dense")
_SPECS = {}


def set_synthetic_root(root):
    """Where the generated URDFs of the synthetic hands go (a temporary directory of the test session)."""
    _SPECS["root"] = str(root)


def spec_of(name):
    if name in SYNTHETIC:
        if name not in _SPECS:
            _SPECS[name] = sh.build(name, _SPECS["root"])
        return _SPECS[name]
    return get_hand_spec(name)


@functools.lru_cache(maxsize=None)
def samples(name, Ns):
    """``hand_surface_samples(spec, 512)``, or a seeded subset of it in shuffled order; synthetic hands: Ns samples as drawn."""
    if name in SYNTHETIC:
        return meshes.hand_surface_samples(spec_of(name), Ns)
    pts, lnk = meshes.hand_surface_samples(spec_of(name), 512)
    if Ns < 512:
        pick = np.random.default_rng(Ns).permutation(512)[:Ns]
        pts, lnk = pts[pick], lnk[pick]
    return pts, lnk


@functools.lru_cache(maxsize=None)
def field(kind, shape=G_SHAPE, origin=G_ORIGIN, voxel=G_H, seed=11):
    if kind == "affine":
        return so.affine(shape, origin, voxel)
    if kind == "multilinear":
        return so.multilinear(shape, origin, voxel)
    if kind == "random":
        return so.random_field(shape, origin, voxel, seed)
    raise KeyError(kind)


def open_joints(spec):
    """The default of the term: the default state clamped to the joint limits, float32."""
    return np.clip(np.asarray(spec.default_state, np.float32), np.asarray(spec.joints_lower, np.float32),
                   np.asarray(spec.joints_upper, np.float32))


def pose(spec, B, seed, spread=0.1):
    """The pose generator of test_gpu_approach._pose.  The synthetic hands draw their joint noise in units of a +-0.3 rad joint
    (_synthetic_hand.joint_scale: a +-5 mm prismatic joint moves by millimetres); the shipped hands take the noise as it is."""
    gen = torch.Generator().manual_seed(seed)
    t = spread * torch.randn(B, 3, generator=gen)
    sc = torch.tensor(sh.joint_scale(spec)) if getattr(spec, "name", "") in SYNTHETIC else 1.0
    th = torch.tensor(np.asarray(spec.default_state, np.float32))[None] + 0.3 * sc * torch.randn(B, spec.n_dofs, generator=gen)
    return torch.cat([t, torch.randn(B, 6, generator=gen), th], 1).float()


def joint_share(ref):
    g = ref["grad"]
    return float(np.linalg.norm(g[:, 9:]) / max(np.linalg.norm(g), 1e-300))


def conditions(ref, margin, Ns, B, cells, opening):
    face, near = po.guards(ref, margin)
    act = ref["active"]
    return ((face >= po.FACE or not cells) and near >= po.NEAR and act.sum() >= min(5, Ns * B) and bool(act.any(axis=(0, 2)).all())
            and (opening >= 1.0 or Ns <= 1 or joint_share(ref) >= JOINT_SHARE))


def assert_guards(ref, margin, tag, Ns, B, K, cells, opening):
    face, near = po.guards(ref, margin)
    act = ref["active"]
    print(f"[{tag}] guards over {act.size} points: nearest cell face {face:.2e} cells, nearest |phi - margin| {near:.2e} m, active "
          f"per station {act.sum(axis=(0, 2)).tolist()}, joint share of the gradient {joint_share(ref):.2e}")
    assert act.size == B * Ns * (K + 1)
    if cells:
        assert face >= po.FACE, (tag, face)
    assert near >= po.NEAR, (tag, near)
    assert act.sum() >= min(5, Ns * B) and act.any(axis=(0, 2)).all(), tag
    if opening < 1.0 and Ns > 1:
        assert joint_share(ref) >= JOINT_SHARE, (tag, joint_share(ref))


def assert_caps(Ns, B, K, kind):
    assert B * Ns * (K + 1) <= (512 if kind == "random" else 4096) or (K == 32 and B == 1), (Ns, B, K, kind)


@functools.lru_cache(maxsize=None)
def guarded(name, Ns, B, K, D, kind, opening, margin, seed0=None):
    """Seeded float32 pose whose B Ns (K+1) station points pass the guards, and the oracle's results at it (computed once)."""
    spec = spec_of(name)
    pts, lnk = samples(name, Ns)
    Ns = len(pts)
    F = field(kind)
    q = open_joints(spec)
    seed0 = 100 * B + Ns if seed0 is None else seed0
    for seed in range(seed0, seed0 + 200):
        hp = pose(spec, B, seed)
        ref = po.e_pregrasp(spec, pts, lnk, hp.double(), q, opening, F, margin, D, K)
        if conditions(ref, margin, Ns, B, kind == "random", opening):
            return hp, ref
    raise AssertionError("no seeded pose passes the guards")


# (hand, Ns, B, K, field, opening, margin): the table of the issue, D = 0.08 m (0.10 m at K >= 8)
TABLE = [("allegro", 1, 1, 4, "random", 0.5, 0.0), ("allegro", 63, 1, 3, "random", 0.5, 0.0), ("allegro", 65, 1, 0, "random", 0.5, 0.0),
         ("allegro", 128, 1, 3, "random", 0.25, 0.01), ("allegro", 512, 1, 0, "random", 0.5, 0.0),
         ("allegro", 512, 3, 1, "multilinear", 0.5, 0.01), ("allegro", 65, 7, 8, "multilinear", 0.5, 0.01),
         ("panda", 512, 2, 3, "multilinear", 0.5, 0.01), ("schunk2", 512, 2, 3, "multilinear", 0.5, 0.01),
         ("ability_hand", 512, 2, 3, "multilinear", 0.5, 0.01), ("shadow_hand", 512, 2, 3, "multilinear", 0.75, 0.01),
         ("allegro", 512, 1, 32, "multilinear", 0.5, 0.0), ("allegro", 512, 2, 3, "multilinear", 1.0, 0.01),
         ("allegro", 512, 2, 3, "multilinear", 0.0, 0.01), ("robotiq3", 128, 2, 2, "multilinear", 0.5, 0.01)]
TABLE_SYNTHETIC = [(name, 128, 2, 2, "multilinear", 0.5, 0.01) for name in SYNTHETIC]


def corridor(K):
    return 0.10 if K >= 8 else 0.08


# ---- an fp64 walk of the REDUCED tree (what the kernel walks), with the node frames ---------------------------------------
def reduced_frames(spec, theta):
    """Actuated joints (JA) -> (W (J,4,4) node frames, T (L,4,4) link transforms, aw (J,3) joint axes in the hand frame), fp64,
    from node_pre / node_axis / node_type / node_parent / link_node / link_offset (and the coupling) alone."""
    theta = np.asarray(theta, np.float64)
    q = theta
    if spec.is_coupled:
        q = np.asarray(spec.coupling, np.float64) @ theta + np.asarray(spec.coupling_offset, np.float64)
    W = []
    for j in range(spec.n_nodes):
        M = np.eye(4)
        a = np.asarray(spec.node_axis[j], np.float64)
        if int(spec.node_type[j]) == 1:
            Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
            M[:3, :3] = np.eye(3) + np.sin(q[j]) * Kx + (1 - np.cos(q[j])) * (Kx @ Kx)
        else:
            M[:3, 3] = a * q[j]
        A = np.asarray(spec.node_pre[j], np.float64) @ M
        p = int(spec.node_parent[j])
        W.append(A if p < 0 else W[p] @ A)
    W = np.stack(W)
    T = np.stack([np.asarray(spec.link_offset[l], np.float64) if int(spec.link_node[l]) < 0 else
                  W[int(spec.link_node[l])] @ np.asarray(spec.link_offset[l], np.float64) for l in range(spec.n_links)])
    aw = np.einsum("jab,jb->ja", W[:, :3, :3], np.asarray(spec.node_axis, np.float64))
    return W, T, aw


def tree_tables(spec):
    """(depth (J), child_off (J+1), child_idx, max_depth) as gq_hand_create derives them from node_parent."""
    parent = [int(p) for p in spec.node_parent]
    J = len(parent)
    depth = [0] * J
    for j in range(J):
        depth[j] = 0 if parent[j] < 0 else depth[parent[j]] + 1
    off, idx = [], []
    for p in range(J):
        off.append(len(idx))
        idx += [j for j in range(J) if parent[j] == p]
    off.append(len(idx))
    return np.array(depth, np.int32), np.array(off, np.int32), np.array(idx, np.int32), max(depth)
