"""The arm the hand sits on, as the reach term takes it (``ops.ArmSpec``; no GPU, no torch).

A serial chain of N <= 8 revolute or prismatic joints with limits:

    FK(q) = base_T  joint_T[0] m_0(q_0)  joint_T[1] m_1(q_1) ... joint_T[N-1] m_{N-1}(q_{N-1})  tool_T

``joint_T[j]`` is the fixed transform parent -> joint frame, ``m_j`` the rotation about (revolute) or the shift along (prismatic)
the unit ``joint_axis[j]`` given in the joint frame, ``tool_T`` flange -> hand root.  Link j is the frame after joint j has moved;
``spheres`` = (link (Ns), centre (Ns,3) in the link frame, radius (Ns)), at most 64, are the arm's collision spheres for the arm
clearance term (``ops.arm_terms``); the hand and a fixed base link carry none.  ``base_T`` is not part of the arm: it places
the arm in the frame of an object and belongs to the call (``ops.reach_terms``, ``GraspStepper(arm_base=...)``).  ``seeds`` (S, N),
1 <= S <= 8, are the joint vectors the IK iteration starts from; the default is the one mid-range configuration.
"""
import xml.etree.ElementTree as ET

import numpy as np

from .hands.spec import _origin, rpy_to_matrix

MAX_JOINTS, MAX_SEEDS, MAX_SPHERES = 8, 8, 64
REVOLUTE, PRISMATIC = 1, 2
_TYPES = {"revolute": REVOLUTE, "prismatic": PRISMATIC, REVOLUTE: REVOLUTE, PRISMATIC: PRISMATIC}


def _T34(T, who):
    T = np.asarray(T, dtype=np.float64)
    if T.shape[-2:] == (4, 4):
        T = T[..., :3, :]
    if T.shape[-2:] != (3, 4):
        raise ValueError(f"ArmSpec: {who} must be (3,4) or (4,4) transforms, got {T.shape}")
    if not np.isfinite(T).all():
        raise ValueError(f"ArmSpec: {who} is not finite")
    return np.ascontiguousarray(T)


def _T44(T34):
    T = np.eye(4)
    T[:3, :] = T34
    return T


class ArmSpec:
    """joint_types: N entries "revolute" / "prismatic" (or 1 / 2); joint_T (N,3,4) or (N,4,4); joint_axis (N,3), normalised here;
    lower / upper (N), finite with lower < upper; tool_T (3,4) or (4,4), default identity; seeds (S,N) inside the limits, default
    the mid-range configuration; spheres None or (link (Ns) integers in 0..N-1, centre (Ns,3) finite, radius (Ns) finite and > 0)
    with 1 <= Ns <= 64.  Anything else raises ValueError."""

    def __init__(self, joint_types, joint_T, joint_axis, lower, upper, tool_T=None, seeds=None, spheres=None):
        types = list(joint_types)
        N = len(types)
        if not 1 <= N <= MAX_JOINTS:
            raise ValueError(f"ArmSpec: the arm must have 1..{MAX_JOINTS} moving joints, got {N}")
        for t in types:
            if t not in _TYPES:
                raise ValueError(f"ArmSpec: joint type {t!r} is neither 'revolute' nor 'prismatic'")
        self.n_joints = N
        self.joint_type = np.array([_TYPES[t] for t in types], dtype=np.int32)
        self.joint_T = _T34(joint_T, "joint_T")
        if self.joint_T.shape != (N, 3, 4):
            raise ValueError(f"ArmSpec: joint_T must hold {N} transforms, got {self.joint_T.shape}")
        ax = np.asarray(joint_axis, dtype=np.float64)
        if ax.shape != (N, 3) or not np.isfinite(ax).all() or (np.linalg.norm(ax, axis=1) == 0).any():
            raise ValueError(f"ArmSpec: joint_axis must be ({N},3), finite and non-zero")
        self.joint_axis = ax / np.linalg.norm(ax, axis=1, keepdims=True)
        self.lower, self.upper = np.asarray(lower, dtype=np.float64), np.asarray(upper, dtype=np.float64)
        if self.lower.shape != (N,) or self.upper.shape != (N,):
            raise ValueError(f"ArmSpec: lower / upper must be ({N},)")
        if not (np.isfinite(self.lower).all() and np.isfinite(self.upper).all()):
            raise ValueError("ArmSpec: the joint limits must be finite (a continuous joint needs limits too)")
        if not (self.lower < self.upper).all():
            raise ValueError("ArmSpec: every joint needs lower < upper")
        self.tool_T = _T34(np.eye(4) if tool_T is None else tool_T, "tool_T")
        if self.tool_T.shape != (3, 4):
            raise ValueError(f"ArmSpec: tool_T must be one transform, got {self.tool_T.shape}")
        s = 0.5 * (self.lower + self.upper)[None] if seeds is None else np.asarray(seeds, dtype=np.float64)
        if s.ndim == 1:
            s = s[None]
        if s.ndim != 2 or s.shape[1] != N or not 1 <= s.shape[0] <= MAX_SEEDS:
            raise ValueError(f"ArmSpec: seeds must be (S,{N}) with 1 <= S <= {MAX_SEEDS}, got {s.shape}")
        if not np.isfinite(s).all() or (s < self.lower).any() or (s > self.upper).any():
            raise ValueError("ArmSpec: every seed must lie inside the joint limits")
        self.seeds = np.ascontiguousarray(s)
        self.n_seeds = int(s.shape[0])
        self.sphere_link = self.sphere_centre = self.sphere_radius = None
        self.n_spheres = 0
        if spheres is not None:
            if len(spheres) != 3:
                raise ValueError("ArmSpec: spheres must be (link, centre, radius)")
            link, centre, radius = (np.asarray(v, dtype=np.float64) for v in spheres)
            Ns = link.shape[0] if link.ndim == 1 else -1
            if not 1 <= Ns <= MAX_SPHERES:
                raise ValueError(f"ArmSpec: sphere link must be (Ns,) with 1 <= Ns <= {MAX_SPHERES}, got {link.shape}")
            if centre.shape != (Ns, 3) or radius.shape != (Ns,):
                raise ValueError(f"ArmSpec: sphere centre must be ({Ns},3) and sphere radius ({Ns},), got {centre.shape} and {radius.shape}")
            if not np.isfinite(link).all() or (link != np.floor(link)).any() or (link < 0).any() or (link > N - 1).any():
                raise ValueError(f"ArmSpec: every sphere link must be an integer in 0..{N - 1}")
            if not np.isfinite(centre).all():
                raise ValueError("ArmSpec: sphere centre is not finite")
            if not np.isfinite(radius).all() or not (radius > 0).all():
                raise ValueError("ArmSpec: every sphere radius must be finite and > 0")
            self.sphere_link, self.sphere_centre, self.sphere_radius = link.astype(np.int32), np.ascontiguousarray(centre), radius
            self.n_spheres = int(Ns)

    @property
    def spheres(self):
        """(link, centre, radius) or None."""
        return None if self.n_spheres == 0 else (self.sphere_link, self.sphere_centre, self.sphere_radius)

    def with_seeds(self, seeds):
        """The same arm with other seeds."""
        return ArmSpec(self.joint_type.tolist(), self.joint_T, self.joint_axis, self.lower, self.upper, self.tool_T, seeds, self.spheres)

    def with_spheres(self, link, centre, radius):
        """The same arm with the collision spheres (link (Ns), centre (Ns,3) in the link frame, radius (Ns) or one number)."""
        link = np.asarray(link)
        radius = np.full(link.shape, float(radius)) if np.ndim(radius) == 0 else radius
        return ArmSpec(self.joint_type.tolist(), self.joint_T, self.joint_axis, self.lower, self.upper, self.tool_T, self.seeds,
                       (link, centre, radius))

    def with_link_spheres(self, radius, spacing):
        """The same arm with spheres of ``radius`` along the segment of every link: from the link's origin to the fixed offset of
        the next joint (``joint_T[j+1]``'s translation; ``tool_T``'s for the last link), a sphere at the origin and then one every
        ``spacing`` metres, the far end included when the segment is longer than half a spacing.  Links are served in order until
        64 spheres are placed."""
        if not (np.isfinite(radius) and radius > 0 and np.isfinite(spacing) and spacing > 0):
            raise ValueError(f"ArmSpec.with_link_spheres: radius = {radius!r} and spacing = {spacing!r} must be finite and > 0")
        link, centre = [], []
        for j in range(self.n_joints):
            end = (self.joint_T[j + 1] if j + 1 < self.n_joints else self.tool_T)[:, 3]
            length = float(np.linalg.norm(end))
            n = int(np.floor(length / spacing + 0.5))  # pieces of the segment
            for i in range(n + 1):
                link.append(j)
                centre.append(end * (i / n) if n else np.zeros(3))
        link, centre = link[:MAX_SPHERES], centre[:MAX_SPHERES]
        return self.with_spheres(link, np.array(centre), float(radius))

    # ---- constructors ---------------------------------------------------------------------------------------------------
    @classmethod
    def from_dh(cls, a, alpha, d, theta, lower, upper, joint_types=None, tool_T=None, seeds=None):
        """Standard (distal) Denavit-Hartenberg rows: link i is ``Rz(theta_i + q_i) Tz(d_i) Tx(a_i) Rx(alpha_i)`` for a revolute joint
        and ``Rz(theta_i) Tz(d_i + q_i) Tx(a_i) Rx(alpha_i)`` for a prismatic one.  The joint moves about / along z at the start of
        its row, so joint_T[0] is the identity, joint_T[i] the fixed part of row i-1, and the fixed part of the last row is folded
        into the tool: FK ends with ``row_{N-1} tool_T``."""
        a, alpha, d, theta = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (a, alpha, d, theta))
        N = len(a)
        if not (len(alpha) == len(d) == len(theta) == N):
            raise ValueError("ArmSpec.from_dh: a, alpha, d, theta must have the same length")
        rows = []
        for i in range(N):
            F = np.eye(4)
            F[:3, :3] = rpy_to_matrix((0.0, 0.0, theta[i]))
            F[2, 3] = d[i]
            G = np.eye(4)
            G[:3, :3] = rpy_to_matrix((alpha[i], 0.0, 0.0))
            G[0, 3] = a[i]
            rows.append(F @ G)
        joint_T = np.stack([np.eye(4)] + rows[:-1]) if N else np.zeros((0, 4, 4))
        tool = rows[-1] @ _T44(_T34(np.eye(4) if tool_T is None else tool_T, "tool_T")) if N else np.eye(4)
        return cls(joint_types or ["revolute"] * N, joint_T, np.tile([0.0, 0.0, 1.0], (N, 1)), lower, upper, tool, seeds)

    @classmethod
    def from_urdf(cls, path, tip_link, base_link=None, tool_T=None, seeds=None):
        """The chain of a URDF file from ``base_link`` (default: the root reached from the tip) to ``tip_link``: the parent joints
        are walked from the tip, fixed joints are folded into the next moving joint's transform (those behind the last moving joint
        into the tool), ``continuous`` joints are refused (the term needs limits), ``<mimic>`` joints too, and so is a chain with more than 8 moving joints."""
        root = ET.parse(path).getroot()
        for j in root.findall("joint"):
            if j.find("child") is None or j.find("parent") is None or j.find("child").get("link") is None or \
                    j.find("parent").get("link") is None:
                raise ValueError(f"ArmSpec.from_urdf: joint {j.get('name')!r} lacks a <parent> or <child> link")
        by_child = {j.find("child").get("link"): j for j in root.findall("joint")}
        links = {l.get("name") for l in root.findall("link")}
        if tip_link not in links:
            raise ValueError(f"ArmSpec.from_urdf: no link {tip_link!r}")
        if base_link is not None and base_link not in links:
            raise ValueError(f"ArmSpec.from_urdf: no link {base_link!r}")
        chain, link = [], tip_link
        while link != base_link and link in by_child:
            chain.append(by_child[link])
            link = chain[-1].find("parent").get("link")
            if len(chain) > len(by_child):
                raise ValueError("ArmSpec.from_urdf: the joints form a loop")
        if base_link is not None and link != base_link:
            raise ValueError(f"ArmSpec.from_urdf: {base_link!r} is not an ancestor of {tip_link!r}")
        types, Ts, axes, lo, hi = [], [], [], [], []
        pending = np.eye(4)
        for j in reversed(chain):
            kind = j.get("type")
            pending = pending @ _origin(j)
            if kind == "fixed":
                continue
            if kind not in ("revolute", "prismatic"):
                raise ValueError(f"ArmSpec.from_urdf: joint {j.get('name')!r} is {kind!r}; only revolute, prismatic and fixed joints "
                                 "(with limits) are supported")
            if j.find("mimic") is not None:
                raise ValueError(f"ArmSpec.from_urdf: joint {j.get('name')!r} mimics another joint; coupled joints are not supported")
            lim = j.find("limit")
            if lim is None or lim.get("lower") is None or lim.get("upper") is None:
                raise ValueError(f"ArmSpec.from_urdf: joint {j.get('name')!r} has no limits")
            ax = j.find("axis")
            types.append(kind)
            Ts.append(pending)
            axes.append([float(v) for v in (ax.get("xyz") if ax is not None else "1 0 0").split()])
            lo.append(float(lim.get("lower")))
            hi.append(float(lim.get("upper")))
            pending = np.eye(4)
        if len(types) > MAX_JOINTS:
            raise ValueError(f"ArmSpec.from_urdf: the chain {link!r} -> {tip_link!r} has {len(types)} moving joints, at most "
                             f"{MAX_JOINTS} are supported")
        if not types:
            raise ValueError(f"ArmSpec.from_urdf: the chain {link!r} -> {tip_link!r} has no moving joint")
        tool = pending @ _T44(_T34(np.eye(4) if tool_T is None else tool_T, "tool_T"))
        return cls(types, np.stack(Ts), axes, lo, hi, tool, seeds)

    # ---- fp64 forward kinematics on the host (tools, tests) ----------------------------------------------------------------
    def fk(self, q, base_T=None):
        """q (N) -> the hand-root pose (4,4) in the base frame (or in the frame ``base_T`` places the base in), fp64 numpy."""
        q = np.asarray(q, dtype=np.float64)
        T = np.eye(4) if base_T is None else _T44(_T34(base_T, "base_T"))
        for j in range(self.n_joints):
            M = np.eye(4)
            a = self.joint_axis[j]
            if self.joint_type[j] == REVOLUTE:
                K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
                M[:3, :3] = np.eye(3) + np.sin(q[j]) * K + (1 - np.cos(q[j])) * (K @ K)
            else:
                M[:3, 3] = q[j] * a
            T = T @ _T44(self.joint_T[j]) @ M
        return T @ _T44(self.tool_T)


# ---- what the tools take on their command line --------------------------------------------------------------------------------
def _preset_arm7():
    """Seven revolute joints with the geometry and the limits of a common 7-axis research arm (joint origins as xyz / rpy), four
    seeds: mid-range and three spread configurations."""
    H = np.pi / 2
    org = [((0, 0, 0.333), (0, 0, 0)), ((0, 0, 0), (-H, 0, 0)), ((0, -0.316, 0), (H, 0, 0)), ((0.0825, 0, 0), (H, 0, 0)),
           ((-0.0825, 0.384, 0), (-H, 0, 0)), ((0, 0, 0), (H, 0, 0)), ((0.088, 0, 0), (H, 0, 0))]
    Ts = []
    for xyz, rpy in org:
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = rpy_to_matrix(rpy), xyz
        Ts.append(T)
    lo = np.array([-2.8973, -1.7628, -2.8973, -3.0718, -2.8973, -0.0175, -2.8973])
    hi = np.array([2.8973, 1.7628, 2.8973, -0.0698, 2.8973, 3.7525, 2.8973])
    tool = np.eye(4)
    tool[2, 3] = 0.107
    mid = 0.5 * (lo + hi)
    seeds = [mid, mid + 0.25 * (hi - lo) * [1, -1, 1, 1, -1, 1, -1], mid + 0.25 * (hi - lo) * [-1, 1, -1, -1, 1, -1, 1],
             mid + 0.25 * (hi - lo) * [1, 1, -1, 1, 1, -1, -1]]
    return ArmSpec(["revolute"] * 7, np.stack(Ts), np.tile([0.0, 0.0, 1.0], (7, 1)), lo, hi, tool, np.array(seeds))


PRESETS = {"arm7": _preset_arm7}


def arm_from_arg(text, tip_link=None, base_link=None):
    """``--arm`` of the tools: the name of a preset (``arm7``) or the path of a URDF file, which needs ``tip_link``."""
    if text in PRESETS:
        return PRESETS[text]()
    if tip_link is None:
        raise ValueError(f"--arm {text!r} is no preset ({', '.join(PRESETS)}); a URDF file needs --arm_tip")
    return ArmSpec.from_urdf(text, tip_link, base_link)


def base_from_arg(xyz_yaw):
    """``--arm_base x y z yaw``: the arm base in the object's frame, turned about z; (3,4)."""
    x, y, z, yaw = (float(v) for v in xyz_yaw)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = rpy_to_matrix((0.0, 0.0, yaw)), (x, y, z)
    return T[:3]
