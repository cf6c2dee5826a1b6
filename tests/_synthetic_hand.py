"""Synthetic hands at the declared limits of the kinematics kernels (J <= 64 tree joints, L <= 64 links, S <= 256 spheres,
64 sphere groups, 320 FK-backward items), for tests/test_synthetic_hand.py and tests/test_gpu_kinematics_limits.py.

Every hand is a generated URDF + one tetrahedron OBJ (about 1 cm, shared by every link) + the two JSON side files, written
into a directory the caller provides, and turned into a HandSpec by the project's own build_hand_spec: the fold of fixed
joints into the reduced node_* tree is therefore part of what is tested.  The oracle (oracle/ref_cpu/kin.py) walks the
unfolded frame_* tree.  Everything is drawn from np.random.RandomState(seed); nothing generated is committed.

Numbers of the generated URDFs: every translation is a multiple of 2^-10 m and every FIXED joint turns by multiples of a
right angle.  The spec stores its tables in float32; with these numbers the folded products (fixed origin x joint origin)
round to the same float32 values as their factors, so the reduced tree and the frame tree agree to fp64 round-off (1e-12)
and the fold is pinned exactly, not to 1e-7.  Moving joints have arbitrary axes and arbitrary rotations in their origins.

Topologies (each the smallest that reaches its path, see the functions):
  chain64          64 joints in one chain (depth 63), revolute / prismatic alternating, L = 64, S = 256, NG = 64
  star63           one root joint with 63 children (63 child-list entries), S = 65 over 18 groups
  comb43           3 wrist joints + 5 fingers of 8 (258 fold tasks), NG = 17
  coupled12        12 tree joints, 5 actuated (joint_filter + coupling, a negative multiplier, non-zero offsets)
  coupled12_dense  the same tree with a coupling matrix that has two non-zeros in some rows (set after the build)
  nospheres        5 joints, S = 0
  layout(sizes)    a flat hand whose only purpose is its sphere groups (self-penetration scan on given centres)"""
import copy
import json
import os

import numpy as np

from graspqp_amd.hands.spec import build_hand_spec

TOPOLOGIES = ("chain64", "star63", "comb43", "coupled12", "coupled12_dense", "nospheres")
GRID = 2.0 ** -10  # m: every translation of the URDFs is a multiple of this

_TETRA = "v 0 0 0\nv 0.01 0 0\nv 0 0.01 0\nv 0 0 0.01\nf 1 3 2\nf 1 2 4\nf 1 4 3\nf 2 3 4\n"
_REV, _PRI = (-0.3, 0.3), (-0.005, 0.005)


class _Tree:
    """Links and joints in file order (children of a link are visited in joint file order), spheres and contacts per link."""

    def __init__(self, seed):
        self.r = np.random.RandomState(seed)
        self.links, self.joints, self.spheres, self.contacts = [], [], {}, {}
        self.n_moving = self.n_fixed = 0

    def _unit(self):
        v = self.r.standard_normal(3)
        return v / np.linalg.norm(v)

    def _xyz(self, seg):
        """A grid vector of about `seg` metres, never zero."""
        k = np.rint(self._unit() * seg / GRID)
        if not k.any():
            k[0] = 1.0
        return k * GRID

    def link(self, name, geom=True, n_spheres=0, n_contacts=2, radius=(0.003, 0.006)):
        self.links.append((name, geom))
        if geom and n_spheres:
            c = self.r.uniform(-0.005, 0.005, (n_spheres, 3))
            self.spheres[name] = np.concatenate([c, self.r.uniform(*radius, (n_spheres, 1))], 1).tolist()
        if geom and n_contacts:
            n = self.r.standard_normal((n_contacts, 3))
            self.contacts[name] = dict(contact_candidates=self.r.uniform(-0.005, 0.005, (n_contacts, 3)).tolist(),
                                       normal_candidates=(n / np.linalg.norm(n, axis=1, keepdims=True)).tolist())
        return name

    def moving(self, parent, child, prismatic=False, seg=0.01, limit=None, name=None):
        name = name or f"j{self.n_moving}"
        self.n_moving += 1
        lo, hi = limit or (_PRI if prismatic else _REV)
        self.joints.append(dict(name=name, type="prismatic" if prismatic else "revolute", parent=parent, child=child,
                                xyz=self._xyz(seg), rpy=self.r.uniform(-0.6, 0.6, 3), axis=self._unit(), lower=lo, upper=hi))
        return name

    def fixed(self, parent, child, seg=0.01):
        self.joints.append(dict(name=f"fix{self.n_fixed}", type="fixed", parent=parent, child=child, xyz=self._xyz(seg),
                                rpy=self.r.randint(-1, 3, 3) * (np.pi / 2)))
        self.n_fixed += 1

    def urdf(self, name):
        v = lambda a: " ".join(repr(float(x)) for x in a)
        out = [f'<?xml version="1.0"?>\n<robot name="{name}">']
        for ln, geom in self.links:
            g = '<visual><geometry><mesh filename="tetra.obj"/></geometry></visual>' if geom else ""
            out.append(f'  <link name="{ln}">{g}</link>')
        for j in self.joints:
            s = (f'  <joint name="{j["name"]}" type="{j["type"]}"><parent link="{j["parent"]}"/><child link="{j["child"]}"/>'
                 f'<origin xyz="{v(j["xyz"])}" rpy="{v(j["rpy"])}"/>')
            if j["type"] != "fixed":
                s += f'<axis xyz="{v(j["axis"])}"/><limit lower="{j["lower"]!r}" upper="{j["upper"]!r}"/>'
            out.append(s + "</joint>")
        out.append("</robot>\n")
        return "\n".join(out)

    def spec(self, name, root, **kw):
        d = os.path.join(str(root), name)
        os.makedirs(d, exist_ok=True)
        files = {"hand.urdf": self.urdf(name), "tetra.obj": _TETRA, "penetration_points.json": json.dumps(self.spheres),
                 "contact_infos.json": json.dumps(self.contacts)}
        for fn, text in files.items():
            with open(os.path.join(d, fn), "w") as f:
                f.write(text)
        return build_hand_spec(name, os.path.join(d, "hand.urdf"), d, os.path.join(d, "penetration_points.json"),
                               os.path.join(d, "contact_infos.json"), **kw)


def chain64(root, seed=101):
    """64 moving joints in one serial chain (depth 63), revolute / prismatic alternating so that prismatic joints sit in the
    interior, a fixed joint before every third moving joint.  A geometry link on the base (link_node = -1) and one on every
    joint but the first: L = 64.  Four spheres per link: S = 256, NG = 64.  Two contact candidates per link.  Segments of
    about 1 cm, limits +-0.3 rad and +-5 mm."""
    t = _Tree(seed)
    prev = t.link("base", n_spheres=4)
    for i in range(64):
        if i % 3 == 2:
            t.fixed(prev, t.link(f"f{i}", geom=False))
            prev = f"f{i}"
        child = t.link(f"l{i}", geom=i > 0, n_spheres=4)
        t.moving(prev, child, prismatic=i % 2 == 1)
        prev = child
    return t.spec("chain64", root)


def star63(root, seed=102):
    """One root joint with 63 child joints: J = 64, depth 1, 63 entries in the child list.  One link per joint; 65 spheres
    over 18 groups (the first wrap of the sphere strides, exactly one group in the second pass of the scan)."""
    t = _Tree(seed)
    t.link("base", geom=False)
    sizes = dict(zip(range(0, 54, 3), [4] * 11 + [3] * 7))  # link -> spheres: 18 groups, 65 spheres
    big = (0.008, 0.012)  # the children sit within 2 cm of each other: with these radii every group penetrates a later one
    t.moving("base", t.link("l0", n_spheres=sizes[0], radius=big), limit=(-0.6, 0.6))
    for i in range(1, 64):
        t.moving("l0", t.link(f"l{i}", n_spheres=sizes.get(i, 0), radius=big), prismatic=i % 3 == 2,
                 limit=None if i % 3 == 2 else (-0.6, 0.6))
    return t.spec("star63", root)


def comb43(root, seed=103):
    """43 joints: a 3-joint wrist and 5 fingers of 8 joints (depth 10): 258 fold tasks, two in the second pass.  Every finger
    hangs on a fixed palm offset and ends in a fixed fingertip link; a geometry link on the base, on every joint and on
    every fingertip (L = 49).  17 sphere groups: ng = 16, one pass of the scan exactly full."""
    t = _Tree(seed)
    with_spheres = set(range(0, 49, 3))  # every third link in file order: 17 groups
    count = [0]

    def link(name):
        k = count[0]
        count[0] += 1
        return t.link(name, n_spheres=(1 + k % 4) if k in with_spheres else 0)

    prev = link("base")
    for i in range(3):
        child = link(f"w{i}")
        t.moving(prev, child, prismatic=i == 1, limit=None if i == 1 else (-0.6, 0.6))
        prev = child
    wrist = prev
    for f in range(5):
        t.fixed(wrist, t.link(f"palm{f}", geom=False), seg=0.03)
        prev = f"palm{f}"
        for m in range(8):
            child = link(f"f{f}_{m}")
            t.moving(prev, child, prismatic=m == 3, limit=None if m == 3 else (-0.6, 0.6))
            prev = child
        t.fixed(prev, link(f"tip{f}"))
    return t.spec("comb43", root)


_ACTUATED12 = ["f0_j0", "f0_j1", "f1_j0", "f2_j0", "f3_j0"]
_COUPLING12 = {"f0_j2": ("f0_j1", 1.05851325, 0.05), "f1_j1": ("f1_j0", -0.8, 0.1), "f1_j2": ("f1_j0", 0.5, -0.07),
               "f2_j1": ("f2_j0", 1.0, 0.0), "f2_j2": ("f2_j0", -0.25, 0.002), "f3_j1": ("f3_j0", 0.9, 0.03),
               "f3_j2": ("f3_j0", 0.7, -0.02)}


def coupled12(root, seed=104):
    """Four fingers of three joints, 12 tree joints of which 5 are actuated: the others follow through build_hand_spec's
    joint_filter and coupling, with a negative multiplier and non-zero offsets.  f2_j2 is prismatic."""
    t = _Tree(seed)
    t.link("base", n_spheres=2)
    for f in range(4):
        t.fixed("base", t.link(f"palm{f}", geom=False), seg=0.03)
        prev = f"palm{f}"
        for m in range(3):
            child = t.link(f"f{f}_{m}", n_spheres=1 + (f + m) % 3)
            t.moving(prev, child, prismatic=(f, m) == (2, 2), limit=None if (f, m) == (2, 2) else (-0.6, 0.6), name=f"f{f}_j{m}")
            prev = child
    spec = t.spec("coupled12", root, joint_filter=_ACTUATED12, coupling=_COUPLING12)
    assert spec.n_nodes == 12 and spec.n_dofs == 5 and spec.is_coupled
    return spec


def coupled12_dense(root, seed=104):
    """coupled12 with spec.coupling overwritten by a general matrix: the rows of f0_j2, f1_j2 and f3_j1 take a second
    actuated joint (two non-zeros in a row).  The kernels and the oracle take any matrix; only the builder is single-source."""
    spec = copy.copy(coupled12(root, seed))
    C = np.array(spec.coupling, dtype=np.float32)
    row = spec.full_joint_names.index
    C[row("f0_j2"), 0] = 0.3
    C[row("f1_j2"), 1] = -0.4
    C[row("f3_j1"), 3] = 0.25
    assert ((C != 0).sum(1) == 2).sum() == 3
    spec.coupling = C
    spec.name = "coupled12_dense"
    return spec


def nospheres(root, seed=105):
    """Five joints in two branches below a root joint, one of them prismatic, and no penetration spheres at all."""
    t = _Tree(seed)
    t.link("base")
    t.moving("base", t.link("l0"), limit=(-0.6, 0.6))
    for f in range(2):
        prev = "l0"
        for m in range(2):
            child = t.link(f"b{f}_{m}")
            t.moving(prev, child, prismatic=(f, m) == (1, 0), limit=None if (f, m) == (1, 0) else (-0.6, 0.6))
            prev = child
    spec = t.spec("nospheres", root)
    assert spec.n_spheres == 0
    return spec


def layout(root, sizes, seed=106, radius=(0.005, 0.015), radii=None):
    """A flat hand with len(sizes) links -- one on the base, one on each of len(sizes) - 1 joints below it -- and sizes[i]
    spheres on link i, radii uniform in `radius` or given: the sphere groups of the self-penetration scan and nothing else."""
    t = _Tree(seed)
    t.link("base", n_spheres=sizes[0], n_contacts=1, radius=radius)
    for i in range(1, len(sizes)):
        t.moving("base", t.link(f"l{i}", n_spheres=sizes[i], n_contacts=1, radius=radius))
    if radii is not None:
        it = iter(np.asarray(radii, dtype=np.float64).tolist())
        for ln, _ in t.links:
            for s in t.spheres.get(ln, []):
                s[3] = next(it)
    spec = t.spec(f"layout_ng{len(sizes)}_s{sum(sizes)}", root)
    assert spec.n_spheres == sum(sizes) and np.array_equal(np.bincount(spec.sphere_link, minlength=len(sizes)), sizes)
    return spec


_BUILDERS = dict(chain64=chain64, star63=star63, comb43=comb43, coupled12=coupled12, coupled12_dense=coupled12_dense,
                 nospheres=nospheres)


def build(name, root):
    return _BUILDERS[name](root)


def joint_scale(spec):
    """Per actuated joint: the width of its limits relative to a +-0.3 rad joint.  Poses of the synthetic hands draw their
    joint noise in these units, so that a +-5 mm prismatic joint moves by millimetres, not by 0.3 m."""
    return ((np.asarray(spec.joints_upper, np.float64) - np.asarray(spec.joints_lower, np.float64)) / 0.6).astype(np.float32)


# ---- a plain numpy fp64 walk of the REDUCED tree (what the kernels walk) ---------------------------------------------------
def _rodrigues(a, q):
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3)[None] + np.sin(q)[:, None, None] * K + (1 - np.cos(q))[:, None, None] * (K @ K)


def reduced_forward_kinematics(spec, theta):
    """Actuated joint values (B, JA) -> link transforms (B, L, 4, 4) from node_pre / node_axis / node_type / node_parent /
    link_node / link_offset alone, in fp64."""
    theta = np.asarray(theta, np.float64)
    B = theta.shape[0]
    q = theta @ np.asarray(spec.coupling, np.float64).T + np.asarray(spec.coupling_offset, np.float64)
    W = []
    for j in range(spec.n_nodes):
        M = np.tile(np.eye(4), (B, 1, 1))
        a = np.asarray(spec.node_axis[j], np.float64)
        if int(spec.node_type[j]) == 1:
            M[:, :3, :3] = _rodrigues(a, q[:, j])
        else:
            M[:, :3, 3] = a[None] * q[:, j, None]
        A = np.asarray(spec.node_pre[j], np.float64)[None] @ M
        p = int(spec.node_parent[j])
        W.append(A if p < 0 else W[p] @ A)
    out = np.empty((B, spec.n_links, 4, 4))
    for l in range(spec.n_links):
        off = np.asarray(spec.link_offset[l], np.float64)
        n = int(spec.link_node[l])
        out[:, l] = off[None] if n < 0 else W[n] @ off
    return out
