"""The MALA* step on the GPU -- proposal, per-object z-score, Metropolis accept and state merge (csrc/loop_dev.h, csrc/loop.hip,
the head of gq_fk_forward and the tail of gq_fk_backward in csrc/kin.hip) -- against oracle/ref_cpu/mala.py in fp64 on the same
fp32 inputs, at the sizes where the kernels take another path: the three routes of the column means, the second pose slot of
a lane (D > 64), contacts beyond lane 63, strided z-score sums, the decay exponents at their period boundaries, overflow,
underflow and NaN in the accept test, the 64-slot ring of draws, and every carrier of the fused head and tail.

Cases, oracle wrappers and bounds: tests/_mala_cases.py (tests/test_mala_cases.py proves on the CPU that the float32 oracle
itself stays inside every bound and that the decisive draws decide the same way in float32 and fp64 on all rows).  Bounds, U =
2^-24, none taken from the kernels: column means (chain + 4) U relative with chain = ceil(B / 16) + 16 (units and inline route)
or ceil(B / 256) + 8 (256-thread kernel); ema that + 4 U; step size and temperature the larger of 4 x the float32 oracle's
error on the case and 16 U; pose 4 U |pose| + |move| (tol_s + tol_ema / 2 + 8 U); z 16 U (1 + |z|) max|e| / sd; integers,
flags and copies exact.

Measured on the MI355X, largest over all cases of this module: kernel error / float32-oracle error 1.00 for the step size
(powf gives torch's float32 bits on every case, error 5.2e-8) and 1.55 for the temperature (powf and erff; B = 17 with z), both
under the factor 4.  Column means 2.4e-7 relative (bounds 7.7e-7 .. 3.1e-6), ema 3.2e-7, pose at most 0.25 of its bound, z at
most 0.12 of its bound.  Every test prints its figures."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _fk_backward_case as fkb  # noqa: E402
import _mala_cases as mc  # noqa: E402
import _synthetic_hand as sh  # noqa: E402
from graspqp_amd.hands import get_hand_spec  # noqa: E402
from graspqp_amd.utils import meshes  # noqa: E402

HP = mc.HP
GUARD = 64
_SENT = {torch.float32: 1.5e30, torch.int64: -77, torch.uint8: 0xA5, torch.int32: -77}


@pytest.fixture(scope="module")
def gq():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from graspqp_amd import _C, ops, stepper

    _C.lib()
    return type("gq", (), {"ops": ops, "C": _C, "stepper": stepper})


@pytest.fixture(scope="module")
def hands(gq, tmp_path_factory):
    """name -> (spec, HandHandle): the shipped hands and chain64 of tests/_synthetic_hand.py (D = 73)."""
    root = tmp_path_factory.mktemp("mala_hands")
    cache = {}

    def get(name):
        if name not in cache:
            spec = sh.build(name, root) if name == "chain64" else get_hand_spec(name)
            cache[name] = (spec, gq.ops.HandHandle(spec))
        return cache[name]

    yield get
    for _, h in cache.values():
        h.close()


@pytest.fixture(scope="module")
def sphere():
    fv = meshes.icosphere(2, 0.05)
    return fv, meshes.surface_points(fv, 128, oversample=4)


class Dev:
    """Device buffers between guard words: inputs must come back untouched, outputs start as sentinels so that an unwritten
    element shows, and nothing next to a buffer may change."""

    def __init__(self):
        self.bufs, self.inputs = [], []

    def _alloc(self, host):
        sent = _SENT[host.dtype]
        buf = torch.full((host.numel() + 2 * GUARD,), sent, dtype=host.dtype)
        buf[GUARD:GUARD + host.numel()] = host.reshape(-1)
        buf = buf.cuda()
        self.bufs.append((buf, host.numel(), sent))
        return buf[GUARD:GUARD + host.numel()].view(host.shape)

    def put(self, a, frozen=False):
        host = torch.tensor(np.ascontiguousarray(a))
        v = self._alloc(host)
        if frozen:
            self.inputs.append((v, host))
        return v

    def out(self, shape, dtype=torch.float32):
        return self._alloc(torch.full(tuple(shape), _SENT[dtype], dtype=dtype))

    def check(self, label=""):
        for buf, n, sent in self.bufs:
            g = torch.cat([buf[:GUARD], buf[GUARD + n:]]).cpu()
            assert bool((g == sent).all()), f"{label}: a guard word next to a buffer changed"
        for v, host in self.inputs:
            assert _same_bits(v.cpu().numpy(), host.numpy()), f"{label}: an input buffer changed"


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _written(t, label):
    assert not bool((t == _SENT[t.dtype]).any()), f"{label}: unwritten elements"
    return t.cpu().numpy()


def run_propose(C, c, label=""):
    """gq_mala_propose on the case -> numpy outputs (g2 = g2_scratch)."""
    B, D, n = c["B"], c["D"], c["n"]
    d = Dev()
    i = {k: d.put(c[k], frozen=True) for k in ("hand_pose", "grad", "idx", "u_switch", "new_idx", "energy")}
    ema, step = d.put(c["ema"]), d.put(c["step"])
    pose, idx, s, z, g2 = d.out((B, D)), d.out((B, n), torch.int64), d.out((B,)), d.out((B,)), d.out((D,))
    C.call("gq_mala_propose", C.f32(i["hand_pose"]), C.f32(i["grad"]), C.i64(i["idx"]), C.f32(i["u_switch"]), C.i64(i["new_idx"]),
           B, D, n, HP["step_size"], HP["stepsize_period"], HP["decay"], HP["mu"], HP["switch_possibility"], int(c["clip"]),
           C.f32(ema), C.i64(step), C.f32(pose), C.i64(idx), C.f32(s), C.f32(g2), C.f32(i["energy"]), c["batch_each"], C.f32(z),
           C.stream_ptr())
    torch.cuda.synchronize()
    d.check(label)
    return dict(pose=_written(pose, label + " pose_out"), idx=_written(idx, label + " idx_out"), ema=ema.cpu().numpy(),
                step=step.cpu().numpy(), s=_written(s, label + " s_out"), z=_written(z, label + " z_out"),
                g2=_written(g2, label + " g2_scratch"))


def _fmt(fig):
    return ", ".join(f"{k} {v:.3g}" for k, v in fig.items())


# ---- (a) column means, stand-alone routes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("B,D", mc.MEAN_SIZES)
def test_column_means_against_the_fp64_mean(gq, B, D, clip):
    """g2_scratch after gq_mala_propose: gq_colsq_units_kernel up to 512 rows and D <= 64 (fewer rows than units, one row per
    unit, its last size), gq_colsq_mean_kernel beyond (its first size, four strides plus one row, D > 64 at any B).  With the
    clip on the gradient holds NaN, +-inf and +-1e3."""
    c = mc.proposal_case(B, D, 4, clip=clip, special=clip, seed=B + D)
    got = run_propose(gq.C, c, f"B={B} D={D} clip={clip}")
    o64, o32 = mc.oracle_propose(c), mc.oracle_propose(c, torch.float32)
    tol = mc.tol_mean(B, mc.colsq_route(B, D))
    assert mc.same_nonfinite(got["g2"], o32["g2"]) and np.isfinite(o64["g2"]).all()
    fin = np.isfinite(o64["g2"])
    e = mc.rel(got["g2"], o64["g2"])[fin].max()
    print(f"B={B} D={D} clip={clip} {mc.colsq_route(B, D)}: column means {e:.3g} relative (bound {tol:.3g}), float32 oracle "
          f"{mc.rel(o32['g2'], o64['g2'])[fin].max():.3g}")
    assert e <= tol
    if clip:
        assert (got["g2"][c["planted"]["zero_col"]] == 0) and np.isfinite(got["g2"]).all()


# ---- (b) proposal and z-score ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,D,n", mc.PROPOSAL_SIZES)
def test_proposal_against_the_oracle(gq, B, D, n):
    """pose_out, ema, step + 1, s_out, idx_out and the zeroed rows: plain gradient, the special gradient with the clip (every
    entry ends finite) and without it (NaN and inf columns, zeroed rows)."""
    worst = {}
    for clip, special in ((False, False), (True, True), (False, True)):
        c = mc.proposal_case(B, D, n, clip=clip, special=special, seed=B + D + n)
        label = f"B={B} D={D} n={n} clip={clip} special={special}"
        fig = mc.check_proposal(c, run_propose(gq.C, c, label), mc.colsq_route(B, D), label)
        if special and not clip:
            assert fig["zeroed_rows"] >= 1
        for k, v in fig.items():
            worst[k] = max(worst.get(k, 0), v)
    print(f"B={B} D={D} n={n}: {_fmt(worst)}")


@pytest.mark.parametrize("n_obj,be,kind", mc.ZSCORE_CASES)
def test_z_score_against_the_oracle(gq, n_obj, be, kind):
    """Strided sums (batch_each no multiple of 64), the object offset, one-row objects (z = NaN), a tight cluster at 1e4 and an
    object of equal energies (std = 0: z = 0 / 0 = NaN, the float32 oracle's pattern)."""
    c = mc.proposal_case(n_obj * be, 25, 4, batch_each=be, seed=be + n_obj, energy=kind)
    label = f"z n_obj={n_obj} batch_each={be} {kind}"
    got = run_propose(gq.C, c, label)
    fig = mc.check_proposal(c, got, mc.colsq_route(c["B"], 25), label)
    if be == 1 or kind == "equal":
        assert np.isnan(got["z"][:be]).all()
    print(f"{label}: {_fmt(fig)}")


# ---- (c) accept and merge --------------------------------------------------------------------------------------------------
def run_accept(C, c, label=""):
    B, D, n, nt = c["B"], c["D"], c["n"], c["n_terms"]
    d = Dev()
    i = {k: d.put(c[k], frozen=True) for k in ("energy_new", "u_accept", "step", "pose_new", "idx_new", "grad_new")}
    z = d.put(c["z"], frozen=True) if c["z"] is not None else None
    rm = d.put(c["reset_mask"], frozen=True) if c["reset_mask"] is not None else None
    tn = d.put(c["terms_new"], frozen=True) if nt else None
    st = {k: d.put(c[k + "_old"]) for k in ("energy", "pose", "idx", "grad")}
    terms = d.put(c["terms_old"]) if nt else None
    acc, temp = d.out((B,), torch.uint8), d.out((B,))
    C.call("gq_mala_accept", C.f32(i["energy_new"]), C.f32(i["u_accept"]), C.f32(z), C.u8(rm), C.i64(i["step"]), C.f32(i["pose_new"]),
           C.i64(i["idx_new"]), C.f32(i["grad_new"]), B, D, n, HP["starting_temperature"], HP["decay"], HP["annealing_period"],
           C.f32(st["energy"]), C.f32(st["pose"]), C.i64(st["idx"]), C.f32(st["grad"]), C.u8(acc), C.f32(temp), nt, C.f32(tn),
           C.f32(terms), C.stream_ptr())
    torch.cuda.synchronize()
    d.check(label)
    got = {k: v.cpu().numpy() for k, v in st.items()}
    got["terms"] = terms.cpu().numpy() if nt else np.zeros((0, B), np.float32)
    return acc.cpu().numpy(), temp.cpu().numpy(), got


@pytest.mark.parametrize("with_reset", [False, True])
@pytest.mark.parametrize("with_z", [False, True])
@pytest.mark.parametrize("B", mc.ACCEPT_B)
def test_accept_and_merge_against_the_oracle(gq, B, with_z, with_reset):
    """gq_mala_accept on decisive draws: the accept vector exactly (no row excluded), the temperature, and the merged state --
    accepted rows hold the bits of the new state, rejected rows the bits of the old one, nothing else changes -- for every
    (D, n) pair of D in {10 .. 128} and n in {1 .. 130} with n_terms in {0, 5, 11, 64}."""
    worst = 0.0
    for (D, n, nt) in mc.accept_shapes():
        c = mc.accept_case(B, D, n, nt, with_z, seed=B + D + n, with_reset=with_reset)
        label = f"accept B={B} D={D} n={n} n_terms={nt} z={with_z} reset={with_reset}"
        acc, temp, got = run_accept(gq.C, c, label)
        fig = mc.check_accept(c, acc, temp, label)
        mc.check_merge(c, acc, got, label=label)
        worst = max(worst, fig["T_ratio"])
    print(f"B={B} z={with_z} reset={with_reset}: temperature error / float32-oracle error at most {worst:.3g}")


# ---- (d) the fused head of gq_fk_forward ------------------------------------------------------------------------------------
def _fk_forward(C, hand, pose, idx, sdf=None, propose=None):
    """One gq_fk_forward launch -> (Rg, link_T, contact points, contact normals) as numpy."""
    B, n = idx.shape
    Rg, LT = torch.zeros(B, 9, device="cuda"), torch.zeros(B, hand.L, 12, device="cuda")
    cp, cn = torch.zeros(B, n, 3, device="cuda"), torch.zeros(B, n, 3, device="cuda")
    ws, nb = hand.fk_ws(B, pose.device)
    C.call("gq_fk_forward", hand.handle, C.f32(pose), C.i64(idx), B, n, C.f32(Rg), C.f32(LT), C.f32(cp), C.f32(cn), None, 0.0,
           None, None, ctypes.byref(propose) if propose is not None else None, ctypes.byref(sdf) if sdf is not None else None,
           C.ptr(ws), nb, C.stream_ptr())
    torch.cuda.synchronize()
    return dict(Rg=Rg.cpu().numpy(), link_T=LT.cpu().numpy(), cp=cp.cpu().numpy(), cn=cn.cpu().numpy())


def _sdf_desc(C, ms, B, n, be):
    out = dict(d2=torch.zeros(B * n, device="cuda"), sgn=torch.zeros(B * n, dtype=torch.int32, device="cuda"),
               onrm=torch.zeros(B * n, 3, device="cuda"), closest=torch.zeros(B * n, 3, device="cuda"))
    sd = C.SdfDesc()
    sd.meshes, sd.queries_per_mesh = ms.handle, be * n
    sd.dist_sq, sd.sign, sd.obj_dir, sd.closest = (out[k].data_ptr() for k in ("d2", "sgn", "onrm", "closest"))
    return sd, out


def _head_case(spec, B, n, be, clip, seed):
    """A proposal case on a real pose of the hand (fkb.make_inputs) with indices among the hand's candidates."""
    D = 9 + spec.n_dofs
    c = mc.proposal_case(B, D, n, batch_each=be, clip=clip, special=clip, seed=seed, n_cand=spec.n_contact_candidates)
    c["hand_pose"] = fkb.make_inputs(spec, max(B, 3), n, seed, sh.joint_scale(spec) if spec.name == "chain64" else None)["hand_pose"][:B]
    c["grad"] = (c["grad"] * np.float32(1e-2)).astype(np.float32)  # moves of a few centimetres / hundredths of a radian
    return c


def _check_fused_head(gq, hands, sphere, name, B, n, attach, ctr, be=None, clip=False, seed=0):
    C = gq.C
    spec, hand = hands(name)
    be = B if be is None else be
    c = _head_case(spec, B, n, be, clip, seed + B + n)
    D = c["D"]
    label = f"{name} B={B} n={n} D={D} sdf={attach} ctr={ctr} batch_each={be} clip={clip}"
    ref = run_propose(C, c, label)
    ms = gq.ops.MeshSet([sphere[0]] * (B // be)) if attach else None
    sd0, q0 = _sdf_desc(C, ms, B, n, be) if attach else (None, {})
    plain = _fk_forward(C, hand, torch.tensor(ref["pose"]).cuda(), torch.tensor(ref["idx"]).cuda(), sdf=sd0)
    plain.update({k: v.cpu().numpy() for k, v in q0.items()})
    # the fused launch: a ring of 64 slots of draws, all but the current one poisoned (u = 0 switches every contact to index 0)
    slots, slot = 64, ctr % 64
    u_ring, ix_ring = np.zeros((slots, B, n), np.float32), np.zeros((slots, B, n), np.int64)
    u_ring[slot], ix_ring[slot] = c["u_switch"], c["new_idx"]
    d = Dev()
    i = {k: d.put(c[k], frozen=True) for k in ("hand_pose", "grad", "idx", "energy")}
    u_ring, ix_ring = d.put(u_ring, frozen=True), d.put(ix_ring, frozen=True)
    ema, step = d.put(c["ema"]), d.put(c["step"])
    pose, idx, s, z, g2 = d.out((B, D)), d.out((B, n), torch.int64), d.out((B,)), d.out((B,)), d.out((D,))
    slot_ctr = d.put(np.array([ctr, -5], np.int32))
    pr = C.ProposeDesc()
    pr.hand_pose, pr.grad, pr.contact_idx = i["hand_pose"].data_ptr(), i["grad"].data_ptr(), i["idx"].data_ptr()
    pr.u_switch, pr.new_idx, pr.ema, pr.step = u_ring.data_ptr(), ix_ring.data_ptr(), ema.data_ptr(), step.data_ptr()
    pr.step_size_out, pr.g2_scratch, pr.energy, pr.batch_each, pr.z_out = s.data_ptr(), g2.data_ptr(), i["energy"].data_ptr(), be, z.data_ptr()
    pr.step_size, pr.stepsize_period, pr.decay, pr.mu = HP["step_size"], HP["stepsize_period"], HP["decay"], HP["mu"]
    pr.switch_possibility, pr.clip_grad, pr.slot_ctr, pr.slots = HP["switch_possibility"], int(clip), slot_ctr.data_ptr(), slots
    sd1, q1 = _sdf_desc(C, ms, B, n, be) if attach else (None, {})
    fused = _fk_forward(C, hand, pose, idx, sdf=sd1, propose=pr)
    fused.update({k: v.cpu().numpy() for k, v in q1.items()})
    d.check(label)
    got = dict(pose=_written(pose, label + " pose"), idx=_written(idx, label + " idx"), ema=ema.cpu().numpy(), step=step.cpu().numpy(),
               s=_written(s, label + " s"), z=_written(z, label + " z"), g2=_written(g2, label + " g2"))
    for k in got:
        assert _same_bits(got[k], ref[k]), f"{label}: {k} of the fused head differs from gq_mala_propose"
    assert slot_ctr.cpu().tolist() == [ctr, ctr + 1], f"{label}: slot_ctr {slot_ctr.cpu().tolist()}"
    for k in plain:
        assert _same_bits(fused[k], plain[k]), f"{label}: {k} differs from a plain gq_fk_forward on the stand-alone proposal"
    assert np.isfinite(fused["cp"]).all()
    return c, got


# (hand, B, n, ring counter, batch_each): the row kernel (no gqSdfDesc)
ROW_HEAD = [("allegro", 4, 4, 0, None), ("allegro", 513, 4, 63, None), ("chain64", 4, 4, 64, None), ("allegro", 3, 4, 197, 1)]


@pytest.mark.parametrize("name,B,n,ctr,be", ROW_HEAD)
def test_fused_head_row_kernel_equals_the_stand_alone_launch(gq, hands, sphere, name, B, n, ctr, be):
    """gq_fk_forward_row_kernel with a gqProposeDesc: pose (in place), idx, ema, step, step_size_out, z_out, g2_scratch and
    slot_ctr[1] bit for bit those of gq_mala_propose; the kinematics those of a plain launch on that proposal.  The last case
    has one row per object: z = NaN on both routes."""
    for clip in (False, True):
        c, got = _check_fused_head(gq, hands, sphere, name, B, n, False, ctr, be=be, clip=clip)
        mc.check_proposal(c, got, mc.colsq_route(B, c["D"]), f"row kernel {name} B={B}")
        if be == 1:
            assert np.isnan(got["z"]).all()


# (hand, B, n, ring counter, batch_each): the block kernel with the sphere attached.  n = 3: the smallest inline case (three
# wavefronts; D = 25 gives two lane groups); n = 12: twelve; n = 13: two rounds, seven wavefronts; n = 2: not inline; panda:
# smallest D, most lane groups; shadow hand D = 31; chain64: D > 64, not inline; B = 513: beyond the inline limit.
BLOCK_HEAD = [("allegro", 17, 3, c, None) for c in (0, 63, 64, 64 * 3 + 5)] + [
    ("allegro", 17, 12, 63, None), ("allegro", 17, 13, 64, None), ("allegro", 17, 2, 0, None), ("panda", 17, 12, 197, None),
    ("shadow_hand", 17, 12, 0, None), ("chain64", 4, 12, 63, None), ("allegro", 1, 12, 64, None), ("allegro", 512, 12, 197, None),
    ("allegro", 513, 12, 0, None), ("allegro", 3, 12, 63, 1)]


@pytest.mark.parametrize("name,B,n,ctr,be", BLOCK_HEAD)
def test_fused_head_block_kernel_equals_the_stand_alone_launch(gq, hands, sphere, name, B, n, ctr, be):
    """gq_fk_forward_kernel with gqProposeDesc and gqSdfDesc: the column means reduced by the query wavefronts where n >= 3
    wavefronts, D <= 64 and B <= 512 (gq_colsq_partial), by a launch of their own otherwise -- the same bits either way, and
    inside the bound of the fp64 mean.  The last case has one row per object."""
    spec, _ = hands(name)
    D = 9 + spec.n_dofs
    nw = -(-n // (-(-n // 12)))
    inline = nw >= 3 and D <= 64 and B <= 512
    c, got = _check_fused_head(gq, hands, sphere, name, B, n, True, ctr, be=be, clip=(ctr % 2 == 1))
    fig = mc.check_proposal(c, got, "inline" if inline else mc.colsq_route(B, D), f"block kernel {name} B={B} n={n}")
    print(f"{name} B={B} n={n} D={D} nw={nw} inline={inline}: {_fmt(fig)}")
    if be == 1:
        assert np.isnan(got["z"]).all()


# ---- (e) the fused tail of gq_fk_backward -----------------------------------------------------------------------------------
def _check_fused_tail(gq, hands, name, B, n, seed, tile=1, ctr=0):
    C = gq.C
    spec, hand = hands(name)
    inp = fkb.make_inputs(spec, B, n, seed, sh.joint_scale(spec) if name == "chain64" else None)
    inp.update(fkb.forward_state(C, hand, inp))
    if tile > 1:
        inp = {k: (np.tile(v, (1, tile)) if k == "terms_old" else np.tile(v, (tile,) + (1,) * (v.ndim - 1))) for k, v in inp.items()}
        B = B * tile
    label = f"fused tail {name} B={B} n={n}"
    r = np.random.RandomState(seed)
    inp["step"] = np.asarray(mc.ACCEPT_STEPS, np.int64)[(np.arange(B) + r.randint(5)) % 5] if B > 4 else np.array([29, 30, 31, 95], np.int64)[:B]
    inp["z"] = r.standard_normal(B).astype(np.float32)
    inp["z"][B - 1] = np.nan
    if tile > 1:  # rows of the same total against different old energies
        inp["energy_old"] = (inp["energy_old"] * (0.9 + 0.2 * r.rand(B))).astype(np.float32)
    # pass 1: the new totals, reproducible to the bit
    first = fkb.run_backward(C, hand, inp)
    again = fkb.run_backward(C, hand, inp)
    for k in ("total", "grad_pose", "terms_new"):
        assert _same_bits(first[k], again[k]), f"{label}: {k} is not bit-reproducible"
    total = first["total"]
    assert np.isfinite(total).all()
    # pass 2: decisive draws from those totals, in slot (ctr % 64) of a ring whose other slots are poisoned
    u = mc.decisive_draws(inp["energy_old"], total, inp["step"], inp["z"], seed)
    case = dict(energy_old=inp["energy_old"], energy_new=total, step=inp["step"], z=inp["z"], u_accept=u, reset_mask=None)
    a0, _ = mc.oracle_accept(case)
    rej = np.nonzero(~a0)[0]
    assert rej.size and a0.any(), f"{label}: the case must accept and reject"
    reset = np.zeros(B, np.uint8)
    reset[rej[0]] = 1  # a row that the test itself rejects
    case["reset_mask"] = reset
    slots = 64
    ring = np.where(np.arange(slots)[:, None] % 2 == 0, np.float32(2.0), np.float32(0.0)) * np.ones((1, B), np.float32)
    ring[ctr % slots] = u
    inp2 = dict(inp, u_accept=ring.astype(np.float32))
    out = fkb.run_backward(C, hand, inp2, reset_mask=reset, slots=slots, slot_ctr=(ctr, ctr + 1))
    assert _same_bits(out["total"], total), f"{label}: total changed with the draws"
    fig = mc.check_accept(case, out["accept"], out["temperature"], label)
    assert out["accept"][rej[0]] == 1 and (rej.size < 2 or out["accept"][rej[1]] == 0)
    pseudo = dict(pose_old=inp["pose_old"], grad_old=inp["grad_old"], idx_old=inp["idx_old"], terms_old=inp["terms_old"],
                  energy_old=inp["energy_old"])
    new = dict(energy=total, pose=inp["hand_pose"], idx=inp["idx"], grad=out["grad_pose"], terms=out["terms_new"])
    mc.check_merge(pseudo, out["accept"], out, label=label, new=new)
    assert out["slot_ctr"].tolist() == [ctr + 1, ctr + 1], f"{label}: slot_ctr {out['slot_ctr']}"
    print(f"{label}: accepted {fig['accepted']} of {B}, temperature error / float32-oracle error {fig['T_ratio']:.3g}")


@pytest.mark.parametrize("name,B,n,ctr", [("allegro", 4, 12, 0), ("allegro", 17, 12, 63), ("chain64", 4, 64, 64 * 3 + 5)])
def test_fused_tail_block_kernel_against_the_oracle(gq, hands, name, B, n, ctr):
    """gq_fk_backward_kernel with energy and accept tail, two passes: the totals of a first run (bit-reproducible) give the
    decisive draws of the second; accept exactly, temperature, merged energy / pose / grad / idx / terms, slot_ctr[0]."""
    _check_fused_tail(gq, hands, name, B, n, 300 + B, ctr=ctr)


def test_fused_tail_wave_kernel_against_the_oracle(gq, hands):
    """gq_fk_backward_wave_kernel (more than 512 rows): the B = 4 inputs of chain64 with n = 64 tiled to 516 rows, every row
    with its own old energy, counter, z and draw."""
    _check_fused_tail(gq, hands, "chain64", 4, 64, 310, tile=129, ctr=64)


# ---- (f) one whole iteration through the stepper ------------------------------------------------------------------------------
def _stepper_iteration(gq, hands, sphere, n_obj, be, n, fuse_loop, seed=7):
    spec, hand = hands("allegro")
    fv, sp = sphere
    B, D = n_obj * be, 9 + spec.n_dofs
    st = gq.stepper.GraspStepper(hand, gq.ops.MeshSet([fv] * n_obj), torch.tensor(np.stack([sp] * n_obj)), be, n)
    for k, v in (("step_size", "step_size"), ("temperature_decay", "decay"), ("mu", "mu"), ("switch_possibility", "switch_possibility")):
        assert np.float32(st.mala[k]) == np.float32(HP[v])
    assert not st.mala["clip_grad"] and st._fuse_loop
    c = mc.proposal_case(B, D, n, batch_each=be, seed=seed, n_cand=spec.n_contact_candidates)
    c["hand_pose"] = fkb.make_inputs(spec, B, n, seed)["hand_pose"]
    c["grad"] = (c["grad"] * np.float32(1e-2)).astype(np.float32)
    st.reset(torch.tensor(c["hand_pose"]).cuda(), torch.tensor(c["idx"]).cuda())
    torch.cuda.synchronize()
    c["energy"] = st.energy.cpu().numpy().copy()  # the accepted energies of the real scene: operands of the z-score
    st.grad.copy_(torch.tensor(c["grad"]).cuda())
    st.ema.copy_(torch.tensor(c["ema"]).cuda())
    st.step_count.copy_(torch.tensor(c["step"]).cuda())
    u_acc = torch.tensor(np.random.RandomState(seed).rand(B).astype(np.float32)).cuda()
    draws = (torch.tensor(c["u_switch"]).cuda(), torch.tensor(c["new_idx"]).cuda(), u_acc)
    st._fuse_loop = fuse_loop
    if fuse_loop:
        st.draw(draws)
        st._iteration(gq.C.stream_ptr(), fused=True)  # the FK forward block carries the query: the column means run inline
    else:
        st.step(draws=draws)
    torch.cuda.synchronize()
    g = lambda t: t.cpu().numpy().copy()
    prop = dict(pose=g(st.pose_new), idx=g(st.idx_new), ema=g(st.ema), step=g(st.step_count), s=g(st.s_out), z=g(st.z), g2=g(st.g2))
    state = dict(energy=g(st.energy), hand_pose=g(st.hand_pose), grad=g(st.grad), contact_idx=g(st.contact_idx), terms=g(st.terms),
                 accept=g(st.accept), temperature=g(st.temperature), total_new=g(st.total_new))
    return c, prop, state


@pytest.mark.parametrize("n_obj,be", [(3, 5), (3, 1)])
def test_stepper_iteration_both_routes(gq, hands, sphere, n_obj, be):
    """GraspStepper on Allegro and three spheres, n = 12, state and draws injected: stand-alone launches (_fuse_loop False) and
    the fused loop with the column means inline.  The proposal of both against the oracle; the state after the iteration bit for
    bit the same on both routes.  batch_each = 1: z and the temperature are NaN and no row is accepted, on both routes."""
    res = {}
    for fuse in (False, True):
        c, prop, state = _stepper_iteration(gq, hands, sphere, n_obj, be, 12, fuse)
        fig = mc.check_proposal(c, prop, "inline" if fuse else "units", f"stepper fuse_loop={fuse}")
        print(f"stepper {n_obj} x {be}, fuse_loop={fuse}: {_fmt(fig)}; accepted {int(state['accept'].sum())} of {n_obj * be}")
        res[fuse] = (prop, state)
        if be == 1:
            assert np.isnan(prop["z"]).all() and np.isnan(state["temperature"]).all() and not state["accept"].any()
            assert _same_bits(state["hand_pose"], c["hand_pose"]) and _same_bits(state["energy"], c["energy"])
    for k in res[False][0]:
        assert _same_bits(res[False][0][k], res[True][0][k]), f"proposal {k} differs between the routes"
    for k in res[False][1]:
        assert _same_bits(res[False][1][k], res[True][1][k]), f"{k} after the iteration differs between the routes"
