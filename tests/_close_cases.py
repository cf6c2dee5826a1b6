"""Inputs of the finger-closing tests, shared by tests/test_close_oracle.py, tests/test_close_body_host.py (CPU) and
tests/test_gpu_close.py.  Nothing here needs a GPU; the fp64 oracle's results are computed once per case and shared.

A case is 8 rows = 4 objects x 2 rows on one hand with Ns samples and S steps.  The grids are a stack of four, 32^3 nodes at 5 mm
about the origin; grid g holds a sphere of radius 3 / 3.5 / 4 / 4.5 cm, so reading another row's grid fails.  The sphere's phi is
computed at the nodes and rounded once; the reference everywhere is the grid's own trilinear interpolant.

The rows populate every regime (``assert_populated``, on the fp64 oracle):
  rows 0, 2, 4, 6  a hand around the sphere, closing: at least two links touch after at least one step ("closing")
  row 1            the closed state of row 0's long run: links touch at step 0 ("touching")
  row 3            joints within a step of a limit, commanded away from the object: ends on the joint limits ("limits")
  row 5            a zero command ("zero")
  row 7            a hand one metre outside the volume ("outside")
The closing rows are built from ONE long run per object (200 steps from the opened hand): every joint starts ``lead`` steps before
the step at which that run stopped it, so that its links touch ``lead`` steps into the case whatever S is (lead = 1 for S = 1).
Guards (tests/_close_oracle.undecidable): a row with an evaluated |m_l - touch| < NEAR before that link's touch is left out of the
exact comparisons; at most one row per case, and no regime may be empty after that.  ``SEEDS`` are the committed seeds for which the
oracle alone meets it; what ``build`` gave at them is kept in tests/golden/close_cases.npz (a case takes ``build`` seconds, its
reference a fraction of one), and tests/test_close_oracle.py checks the guards on those inputs."""
import functools
import os

import numpy as np
import torch

import _close_oracle as co
import _pregrasp_cases as pc
import _scene_oracle as so
from graspqp_amd import ops
from graspqp_amd.hands import get_hand_spec

B, BE = 8, 2
G_SHAPE, G_H = (32, 32, 32), 0.005
G_ORIGIN = (-0.0775, -0.0775, -0.0775)
RADII = (0.030, 0.035, 0.040, 0.045)
TOUCH = 5e-4
HANDS = ("allegro", "ability_hand", "panda")
NS = (96, 512)
STEPS = (1, 8, 32)
LONG = 200  # steps of the oracle's long run (the oracle has no limit of 64)
CLOSING, TOUCHING, LIMITS, ZERO, OUTSIDE = (0, 2, 4, 6), (1,), (3,), (5,), (7,)
# the closing sense of each hand's actuated joints, and the share of the way from the lower to the upper limits at which the
# fingertips meet: the centre of the spheres is put there
SENSE = {"allegro": 1.0, "ability_hand": 1.0, "panda": -1.0}
SEEDS = {}  # (hand, Ns, S) -> seed; filled below


def cases():
    return [(h, ns, s) for h in HANDS for ns in NS for s in STEPS]


@functools.lru_cache(maxsize=None)
def fields():
    out = []
    for r in RADII:
        out.append(so.Field(G_SHAPE, G_ORIGIN, G_H, analytic=lambda x, r=r: x.norm(dim=-1) - r))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def samples(name, Ns):
    """The samples of tests/_pregrasp_cases.samples in the order ops.SurfaceSamples keeps them (stable sort by link), so that the
    sample indices of the oracle and of the launch mean the same."""
    pts, lnk = pc.samples(name, Ns)
    order = np.argsort(np.asarray(lnk), kind="stable")
    return np.ascontiguousarray(np.asarray(pts)[order], np.float32), np.ascontiguousarray(np.asarray(lnk)[order], np.int32)


def lead(S):
    return 1 if S == 1 else 3 if S == 8 else 5


def _rot6(gen):
    return torch.randn(6, generator=gen)


def _opened(spec, name):
    """The joints the long run starts from: a tenth of the range in from the limit the hand opens towards"""
    lo, hi = np.asarray(spec.joints_lower, np.float64), np.asarray(spec.joints_upper, np.float64)
    return (lo + 0.1 * (hi - lo)) if SENSE[name] > 0 else (hi - 0.1 * (hi - lo))


def _centre(spec, name, pts, lnk, six, share):
    """Where the fingers close to, in the world frame of a hand at the origin with rotation ``six``: the mean over the outermost links
    of the middle of the link's samples, with the joints ``share`` of the way along the closing sense; and the unit vector from the
    hand's base towards it."""
    lo, hi = np.asarray(spec.joints_lower, np.float64), np.asarray(spec.joints_upper, np.float64)
    th = lo + share * (hi - lo) if SENSE[name] > 0 else hi - share * (hi - lo)
    oh = so.hand_oracle(spec, pts, lnk)
    hp = torch.cat([torch.zeros(3, dtype=torch.float64), six.double(), torch.as_tensor(th)])[None]
    oh.set_parameters(hp, torch.zeros(1, 1, dtype=torch.long))
    x = oh.get_surface_points()[0]
    parents = set(int(p) for p in spec.node_parent)
    tips = [l for l, n in enumerate(spec.link_node) if int(n) >= 0 and int(n) not in parents and (np.asarray(lnk) == l).any()]
    mid = lambda p: 0.5 * (p.min(0).values + p.max(0).values)  # the middle of the link's box: every outermost link counts the same
    c = torch.stack([mid(x[torch.as_tensor(np.asarray(lnk) == l)]) for l in tips]).mean(0)
    fixed = np.asarray(spec.link_node)[np.asarray(lnk)] < 0
    out = c - mid(x[torch.as_tensor(fixed)]) if fixed.any() else c  # from the hand's base towards the fingertips
    return c, out / out.norm()


def _row_ok(name, kind, ref):
    """Is the one-row reference what its regime asks for, with nothing near the touch tolerance?"""
    if co.undecidable(ref, TOUCH)[0]:
        return False
    return len(regimes(name, ref, rows={kind: (0,)})[kind]) == 1


TRIES = 80
DEBUG = False
PUSH = {"allegro": 0.0, "ability_hand": 0.0, "panda": 0.004}  # panda opens to 8 cm: it pinches a cap of the sphere, not its equator
JITTER = {"allegro": 0.004, "ability_hand": 0.004, "panda": 0.0001}  # panda's one joint stops at the first touch: both fingers must
# touch at the same step, which a draw in a few gives


@functools.lru_cache(maxsize=None)
def build(name, Ns, S, seed):
    """-> (hand_pose (8,D) float32, direction (8,JA) float32, step (JA) float32) of a case.  Per object, seeded draws of the hand's
    rotation and of the sphere's place are tried (at most TRIES) until both rows of the object are in their regime on the fp64
    oracle with no evaluated m_l within NEAR of the tolerance."""
    spec = get_hand_spec(name)
    pts, lnk = samples(name, Ns)
    gen = torch.Generator().manual_seed(seed)
    JA = spec.n_dofs
    step = ops.close_default_step(spec)
    st = torch.as_tensor(step)
    th0 = torch.as_tensor(_opened(spec, name), dtype=torch.float32)
    lo, hi = torch.as_tensor(np.asarray(spec.joints_lower, np.float32)), torch.as_tensor(np.asarray(spec.joints_upper, np.float32))
    hp, dirs = torch.zeros(B, 9 + JA), torch.zeros(B, JA)
    K = lead(S)
    run = lambda obj, p, d, steps: co.close(spec, pts, lnk, p[None], d[None], (fields()[obj],), steps, step, TOUCH)
    for obj in range(B // BE):
        r0, r1 = BE * obj, BE * obj + 1
        kind = "touching" if r1 in TOUCHING else "limits" if r1 in LIMITS else "zero" if r1 in ZERO else "outside"
        for _ in range(TRIES):
            v = torch.full((JA,), SENSE[name]) * (0.5 + 0.5 * torch.rand(JA, generator=gen))  # every joint closes, at its own speed
            six = _rot6(gen)
            share = 0.35 + 0.3 * float(torch.rand(1, generator=gen))
            c, out = _centre(spec, name, pts, lnk, six, share)
            c, out = c.float(), out.float()
            if PUSH[name]:  # move the sphere out along the fingers until the opened hand clears it by PUSH, then sideways until the
                moving = np.nonzero(np.asarray(spec.link_node) >= 0)[0]  # two fingers are equally far from it (bisection)
                m0 = lambda cc_, th=th0: run(obj, torch.cat([-cc_, six, th]), v, 0)["M"][0, 0][moving]
                for d in np.arange(0.0, RADII[obj] + 0.04, 0.002):
                    if m0(c + float(d) * out).min() >= PUSH[name]:
                        break
                c = c + float(d) * out
                x = so.hand_oracle(spec, pts, lnk)
                x.set_parameters(torch.cat([torch.zeros(3), six, th0]).double()[None], torch.zeros(1, 1, dtype=torch.long))
                xs = x.get_surface_points()[0].float()
                side = xs[torch.as_tensor(lnk == moving[1])].mean(0) - xs[torch.as_tensor(lnk == moving[0])].mean(0)
                side = side / side.norm()
                for th in (th0, None):  # balance the opened hand, then the hand closed to its first touch
                    if th is None:
                        th = torch.as_tensor(run(obj, torch.cat([-c, six, th0]), v, LONG)["theta"][0]).float()
                    a_, b_ = -0.008, 0.008
                    for _i in range(24):
                        mid_ = 0.5 * (a_ + b_)
                        mm = m0(c + mid_ * side, th)
                        a_, b_ = (a_, mid_) if mm[1] < mm[0] else (mid_, b_)  # moving towards the second finger shrinks its distance
                    c = c + 0.5 * (a_ + b_) * side
            c = c + JITTER[name] * torch.randn(3, generator=gen)
            long = run(obj, torch.cat([-c, six, th0]), v, LONG)  # the sphere's centre is the origin of the grid
            tr, js = torch.as_tensor(long["thetas"][:, 0]).float(), long["joint_stop"][0]
            start = torch.stack([tr[max(int(js[a]) - K, 0) if js[a] >= 0 else max(LONG - K, 0), a] for a in range(JA)])
            p0, d0 = torch.cat([-c, six, start]), v
            if kind == "touching":
                p1, d1 = torch.cat([-c, six, torch.as_tensor(long["theta"][0]).float()]), v
            elif kind == "limits":  # 4 cm further from the sphere, within 0.3 steps of the limit the hand opens towards, sent there
                away = -SENSE[name]
                near = (lo + 0.3 * st) if away < 0 else (hi - 0.3 * st)
                p1, d1 = torch.cat([-c - 0.04 * c / c.norm(), six, near]), away * st * 100.0
            elif kind == "zero":
                p1, d1 = p0.clone(), torch.zeros(JA)
            else:
                p1, d1 = torch.cat([-c + torch.tensor([1.0, 0.0, 0.0]), six, start]), v
            ra, rb = run(obj, p0, d0, S), run(obj, p1, d1, S)
            if DEBUG:
                print(obj, "long ts", long["touch_step"][0].tolist(), "short ts", ra["touch_step"][0].tolist(), "M", np.round(ra["M"][:, 0] * 1e3, 2).tolist(),
                      _row_ok(name, "closing", ra), kind, _row_ok(name, kind, rb))
            if _row_ok(name, "closing", ra) and _row_ok(name, kind, rb):
                break
        else:
            raise AssertionError(f"no draw in {TRIES} puts object {obj} of {(name, Ns, S, seed)} in its regimes")
        hp[r0], dirs[r0], hp[r1], dirs[r1] = p0, d0, p1, d1
    return hp.contiguous(), dirs.contiguous(), step


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "close_cases.npz")


@functools.lru_cache(maxsize=None)
def inputs(name, Ns, S):
    """The committed inputs of a case (tests/golden/close_cases.npz, what ``build`` gave at ``SEEDS``; ``python tests/_close_cases.py``
    writes the file again): hand_pose (8,D), direction (8,JA), step (JA), float32."""
    with np.load(GOLDEN) as z:
        k = f"{name}_{Ns}_{S}"
        return torch.from_numpy(z[k + "_pose"]), torch.from_numpy(z[k + "_dir"]), z[k + "_step"]


@functools.lru_cache(maxsize=None)
def reference(name, Ns, S, dtype=torch.float64):
    hp, dirs, step = inputs(name, Ns, S)
    pts, lnk = samples(name, Ns)
    return co.close(get_hand_spec(name), pts, lnk, hp, dirs, fields(), S, step, TOUCH, dtype)


def regimes(name, ref, keep=None, rows=None):
    """rows per regime on a reference.  ``keep`` (B) bool: the rows that count; ``rows``: regime -> the rows it is looked for in"""
    spec = get_hand_spec(name)
    n = ref["theta"].shape[0]
    keep = np.ones(n, bool) if keep is None else keep
    where = dict(closing=CLOSING, touching=TOUCHING, limits=LIMITS, zero=ZERO, outside=OUTSIDE) if rows is None else rows
    ts, js, th, d = ref["touch_step"], ref["joint_stop"], ref["theta"], ref["delta"]
    lo, hi = np.asarray(spec.joints_lower, np.float32).astype(np.float64), np.asarray(spec.joints_upper, np.float32).astype(np.float64)
    on_limit = (th == lo) | (th == hi)
    test = dict(
        closing=lambda b: (ts[b] >= 1).sum() >= 2,  # at least two links touch after at least one step
        touching=lambda b: (ts[b] == 0).any() and (js[b] == 0).any(),  # touching, and stopped by it, before the first step
        limits=lambda b: (js[b] < 0).all() and (d[b] != 0).all() and on_limit[b].all(),  # no touch stopped a joint: the limits did
        zero=lambda b: (d[b] == 0).all() and (th[b] == ref["thetas"][0, b]).all(),
        outside=lambda b: np.isinf(ref["phi"][b]).all() and (ref["sample"][b] < 0).all() and (ts[b] < 0).all())
    return {k: [b for b in where[k] if keep[b] and test[k](b)] for k in where}


def assert_populated(name, ref, tag):
    und = co.undecidable(ref, TOUCH)
    reg = regimes(name, ref, ~und)
    print(f"[{tag}] undecidable rows {np.nonzero(und)[0].tolist()}, regimes {reg}, touched links per row "
          f"{(ref['touch_step'] >= 0).sum(1).tolist()}, touch steps of row 0 {ref['touch_step'][0].tolist()}")
    assert und.sum() <= 1, (tag, und)
    assert all(len(v) > 0 for v in reg.values()), (tag, reg)
    return und


def compare_masks(ref):
    """Which (row, link) pairs the sample / point and the normal are compared at -> (exact (B,L) bool, normal (B,L) bool)"""
    has = ref["sample"] >= 0
    with np.errstate(invalid="ignore"):
        exact = has & ~(ref["second"] - ref["phi"] <= co.NEAR)
    return exact, exact & (ref["face"] > co.FACE)


SEEDS.update({c: 1 for c in cases()})

if __name__ == "__main__":  # python tests/_close_cases.py (with the repository root and oracle/ on the path, as tests/conftest.py puts them)
    out = {}
    for c in cases():
        hp_, dirs_, step_ = build(*c, SEEDS[c])
        k_ = "%s_%d_%d" % c
        out[k_ + "_pose"], out[k_ + "_dir"], out[k_ + "_step"] = hp_.numpy(), dirs_.numpy(), np.asarray(step_, np.float32)
        print(k_, flush=True)
    np.savez(GOLDEN, **out)
