"""gq_pen_bwd_body (csrc/pen_dev.h) -- the backward of the hand-penetration query, which every pose gradient of E_pen (and of
E_wall, E_scene, E_approach, which accumulate onto its outputs) goes through -- against the fp64 oracle of
tests/_pen_backward_oracle.py, on synthetic inputs (the function is a pure map of plain arrays) and on two real scenes.

Every call pre-fills wrench, gRt and e_pen with a sentinel and must leave none; every synthetic case runs in both forms
(grad_dis given; grad_dis = NULL with dis, w_pen = 100, e_pen) unless it needs signed or NaN weights.  The tolerance is the
derived one of the oracle module, per accumulator; every check prints max |hip - ref| / tol, which must stay below 1.

Path of the kernel                                            -> case that reaches it (its precondition is asserted by the
                                                                 case itself, with GQ_PENB_K / GQ_PENB_LIST read from the source)
  second and later rounds of the point loop (P > 4096)        -> test_several_rounds (4097: a last round of ONE point; 9000)
  the K = 16 instantiation (P > 2560)                         -> test_k16_single_round, test_several_rounds, test_list_overflow[9000]
  `first ? 0 : *dst` read-modify-write across rounds          -> test_several_rounds, test_list_overflow (sentinel pre-fill: a
                                                                 first round that read *dst would keep 12345)
  kfit < K: the LDS list fills up, slices wait for the next   -> test_list_overflow: 2500 (kfit = 4 exactly; a slice that does not
  round                                                          fit behind a partly filled list), 9000 (every round cut at 4),
                                                                 test_fused_roles_equal_the_stand_alone_kernel (a real scene)
  fold loop with more than four groups, sums not riding       -> test_link_groups (L = 16, 19, 20, 160; riding: 1, 2, 5, 17)
  rows with no contributing point                             -> test_list_overflow[2500] row 2, test_ragged_single_round[1]
  a NaN weight                                                -> test_nan_weight
  refusal of bad sizes                                        -> test_refusals

Further: bitwise determinism, bitwise independence of the instantiation K, the row stride of hand_pose, objects
(row / batch_each), exact zeros on links without points, -0.0 / 1e-30 weights; the fused roles of gq_stage_b_kernel and
gq_stage_b_alt_kernel against the stand-alone kernel bit for bit; and the forward's (dis, link, gvec) per point against the
fp64 oracle (test_forward_offsets_and_links_against_the_oracle)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _pen_backward_oracle as pbo  # noqa: E402
import _pen_scene as psc  # noqa: E402
from graspqp_amd.hands import get_hand_spec  # noqa: E402
from graspqp_amd.utils import meshes  # noqa: E402

W_PEN = 100.0
FORMS = [False, True]  # fused: grad_dis = NULL


@pytest.fixture(scope="module")
def gq():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from graspqp_amd import _C, ops, stepper

    _C.lib()
    return type("gq", (), {"ops": ops, "C": _C, "stepper": stepper})


@pytest.fixture(scope="module")
def consts():
    return pbo.kernel_constants()


_worst = {"ratio": 0.0}


def _dev(a):
    return None if a is None else torch.as_tensor(a).cuda().contiguous()


def _launch(gq, case, L=None, e_pen=True):
    """One call of gq_hand_pen_backward on sentinel-filled outputs -> (wrench, gRt, e_pen or None) as device tensors,
    and the call's exception (or None)."""
    C = gq.C
    B, P, L = case["B"], case["P"], case["L"] if L is None else L
    surf, hp, Rg, w, link, gvec, dis = (_dev(case[k]) for k in ("surf", "hand_pose", "Rg", "w", "link", "gvec", "dis"))
    assert surf.shape == (case["n_obj"], P, 3) and hp.shape[0] == B and Rg.shape == (B, 9) and link.shape == (B, P)
    assert gvec.shape == (B, P, 3) and (w if w is not None else dis).shape == (B, P) and B <= 8 and P <= 9000
    assert int(link.min()) >= 0 and int(link.max()) < max(L, 1)
    fill = lambda *s: torch.full(s, pbo.SENTINEL, device="cuda")
    wrench, gRt = fill(B, max(L, 1), 6), fill(B, 12)
    e = fill(B) if (w is None and e_pen) else None
    err = None
    try:
        C.call("gq_hand_pen_backward", int(L), C.f32(surf), case["n_obj"], P, case["batch_each"], C.f32(hp), hp.shape[1], C.f32(Rg),
               C.f32(w), C.i32(link), C.f32(gvec), C.f32(wrench), C.f32(gRt), C.f32(dis), W_PEN, C.f32(e), None, None,
               C.stream_ptr())
    except RuntimeError as ex:
        err = ex
    torch.cuda.synchronize()
    return (wrench, gRt, e), err


def _run(gq, case):
    (wrench, gRt, e), err = _launch(gq, case)
    assert err is None, err
    out = [t.cpu().numpy() for t in (wrench, gRt)] + [None if e is None else e.cpu().numpy()]
    for name, a in zip(("wrench", "gRt", "e_pen"), out):
        assert a is None or not (a == np.float32(pbo.SENTINEL)).any(), f"{name}: the sentinel is left in {int((a == pbo.SENTINEL).sum())} places"
    assert (out[2] is None) == (case["w"] is not None)
    return out


def _ratio(got, ref, tol, where=None):
    r = np.abs(got.astype(np.float64) - ref) / tol
    return float(r.max() if where is None else r[where].max())


def _check(gq, case, tag):
    """Run, compare with the oracle, print the ratio -> the kernel's outputs."""
    out = _run(gq, case)
    wr, g, e, bd = pbo.oracle_of(case, W_PEN)
    assert np.isfinite(out[0]).all() and np.isfinite(out[1]).all()
    rs = {"wrench": _ratio(out[0], wr, bd["wrench"]), "gRt": _ratio(out[1], g, bd["gRt"])}
    if e is not None:
        assert np.isfinite(out[2]).all()
        rs["e_pen"] = _ratio(out[2], e, bd["e_pen"])
    _worst["ratio"] = max(_worst["ratio"], *rs.values())
    print(f"{tag} [{'fused' if case['w'] is None else 'grad_dis'}] n_max={bd['n_max']}: max |hip - ref| / tol = "
          + ", ".join(f"{k} {v:.3f}" for k, v in rs.items()) + f"   (all cases so far: {_worst['ratio']:.3f})")
    assert all(v < 1.0 for v in rs.values()), rs
    return out


def _same_bits(a, b):
    return all((x is None and y is None) or np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------------------
# synthetic cases against the oracle
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", FORMS)
@pytest.mark.parametrize("P", pbo.RAGGED_P)
def test_ragged_single_round(gq, consts, P, fused):
    """The K = 10 kernel: P below one slice, at and around a slice boundary, the reference's 2500, the largest P it takes."""
    case = pbo.case_ragged(P, fused)
    pbo.require_single_round(case, consts, "K_small")
    if P == 1:
        n = pbo.contributing(case).sum(1)
        assert n[0] == 1 and (n == 0).any(), "P = 1: a row with its one point and a row without"
    _check(gq, case, f"ragged P={P}")


@pytest.mark.parametrize("fused", FORMS)
@pytest.mark.parametrize("P", pbo.K16_P)
def test_k16_single_round(gq, consts, P, fused):
    case = pbo.case_k16(P, fused)
    pbo.require_single_round(case, consts, "K")
    _check(gq, case, f"K=16 P={P}")


@pytest.mark.parametrize("fused", FORMS)
@pytest.mark.parametrize("P", pbo.ROUNDS_P)
def test_several_rounds(gq, consts, P, fused):
    """first == false: the later rounds add onto what the first one stored; the last round is ragged."""
    case = pbo.case_rounds(P, fused)
    pbo.require_several_rounds(case, consts)
    _check(gq, case, f"rounds P={P}")


@pytest.mark.parametrize("fused", FORMS)
@pytest.mark.parametrize("P", [2500, 9000])
def test_list_overflow(gq, consts, P, fused):
    """kfit < K: a round's LDS list fills up and the remaining slices are taken up again by the next round."""
    case = pbo.case_overflow(P, fused)
    (pbo.require_overflow_2500 if P == 2500 else pbo.require_overflow_9000)(case, consts)
    out = _check(gq, case, f"overflow P={P}")
    if P == 2500:  # the empty row beside the full ones: zeros, written
        assert (out[0][2] == 0).all() and (out[1][2] == 0).all() and (out[2] is None or out[2][2] == 0)
    assert _same_bits(out, _run(gq, case)), "two runs of one case differ in their bits"


@pytest.mark.parametrize("fused", FORMS)
def test_order_of_sums_is_independent_of_K(gq, consts, fused):
    """pen_dev.h: "The order of all sums is independent of K."  The P = 2500 overflow case again with every per-point array
    padded to P = 2816 by points that do not contribute: the K = 10 kernel, then the K = 16 kernel, same bits."""
    case = pbo.case_overflow(2500, fused)
    pbo.require_overflow_2500(case, consts)
    P2, B = 2816, case["B"]
    assert pbo.launcher_K(2500, consts) == consts["K_small"] < pbo.launcher_K(P2, consts) == consts["K"]
    pad = lambda a, v: np.concatenate([a, np.full((a.shape[0], P2 - 2500) + a.shape[2:], v, a.dtype)], 1)
    big = dict(case, P=P2, surf=pad(case["surf"], 0.05), link=pad(case["link"], 0), gvec=pad(case["gvec"], 0.0),
               w=None if fused else pad(case["w"], 0.0), dis=pad(case["dis"], -1.0) if fused else None)
    assert np.array_equal(pbo.contributing(big)[:, :2500], pbo.contributing(case)) and not pbo.contributing(big)[:, 2500:].any()
    assert _same_bits(_run(gq, case), _check(gq, big, "padded to P=2816"))


@pytest.mark.parametrize("fused", FORMS)
@pytest.mark.parametrize("L", pbo.GROUP_L)
def test_link_groups(gq, consts, L, fused):
    """The fold: a wavefront takes a group of four links or the group of the 12 global sums, which ride in the last link group
    when that holds at most two links; with more than four groups a wavefront folds two or more; link id 159 as a byte."""
    case = pbo.case_groups(L, fused)
    pbo.require_groups(case, consts)
    _check(gq, case, f"groups L={L}")


@pytest.mark.parametrize("fused", FORMS)
@pytest.mark.parametrize("only", [13, 0])
def test_all_points_on_one_link(gq, only, fused):
    case = pbo.make_case(3, 600, 14, seed=600 + only, density=0.5, fused=fused)
    on = pbo.contributing(case)
    case["link"] = np.where(on, only, 0).astype(np.int32)
    out = _check(gq, case, f"all on link {only}")
    others = np.delete(out[0], only, axis=1)
    assert (others == 0.0).all(), "links without a point must come out exactly 0.0"
    assert (np.abs(out[0][:, only]) > 0).all()
    np.testing.assert_array_equal(out[0][:, only, :3], -out[1][:, :3])  # one link: f = -gsum, the same chains, bit for bit


@pytest.mark.parametrize("fused", FORMS)
def test_objects(gq, fused):
    """obj = row / batch_each picks the object's surface points."""
    case = pbo.make_case(6, 300, 14, n_obj=2, seed=700, density=0.5, fused=fused)
    assert case["batch_each"] == 3 and not np.array_equal(case["surf"][0], case["surf"][1])
    out = _check(gq, case, "objects 2 x 3")
    swapped = pbo.oracle_of(dict(case, surf=case["surf"][::-1].copy()), W_PEN)
    assert _ratio(out[0], swapped[0], swapped[3]["wrench"]) > 100, "the case must tell the objects apart"


@pytest.mark.parametrize("fused", FORMS)
def test_pose_dim(gq, fused):
    """The row stride of hand_pose: D = 9 and D = 25 with the same first nine columns give the same bits."""
    case = pbo.make_case(5, 300, 14, seed=800, density=0.5, fused=fused, D=9)
    wide = dict(case, hand_pose=np.concatenate([case["hand_pose"], np.random.default_rng(1).normal(size=(5, 16)).astype(np.float32)], 1))
    assert wide["hand_pose"].shape == (5, 25)
    assert _same_bits(_check(gq, case, "D=9"), _check(gq, wide, "D=25"))


def test_signed_and_tiny_weights(gq):
    """w of both signs; w = 1e-30 contributes (its link holds nothing else: the wrench there is 1e-30 G, not 0); w = -0.0
    and w = +0.0 do not -- a NaN gradient at those points would show.  In the fused form dis = 0.0, -1e30 and NaN do not."""
    case = pbo.make_case(3, 600, 15, seed=900, density=0.5, fused=False)
    on = pbo.contributing(case)
    assert (case["w"] < 0).any() and (case["w"] > 0).any()
    case["link"][case["link"] == 14] = 3  # link 14 is kept for the tiny weight alone
    tiny = np.nonzero(on[0])[0][0]
    pbo.force_on(case, 0, tiny, 14, np.float32(1e-30))
    z0, z1 = np.nonzero(~on[0])[0][:2]
    case["w"][0, z1] = -0.0
    assert np.signbit(case["w"][0, z1]) and not np.signbit(case["w"][0, z0]) and case["w"][0, z0] == 0
    case["gvec"][0, [z0, z1]] = np.nan
    case["link"][0, [z0, z1]] = 5
    out = _check(gq, case, "signed, 1e-30, -0.0")
    g = case["gvec"][0, tiny].astype(np.float64)
    assert (np.abs(out[0][0, 14, :3]) > 0).all()
    np.testing.assert_allclose(out[0][0, 14, :3], -1e-30 * g, rtol=1e-6, atol=0)
    fz = pbo.make_case(3, 600, 14, seed=901, density=0.5, fused=True)
    off = np.nonzero(~pbo.contributing(fz)[1])[0]
    kinds = {float(v): off[fz["dis"][1, off] == v][0] for v in (0.0, -1e30)}
    nan_pt = off[(fz["dis"][1, off] < 0) & (fz["dis"][1, off] > -1)][0]
    fz["dis"][1, nan_pt] = np.nan
    for p in list(kinds.values()) + [nan_pt]:
        fz["gvec"][1, p], fz["link"][1, p] = np.nan, 7
    _check(gq, fz, "dis = 0.0, -1e30, NaN")


def test_nan_weight(gq):
    """__ballot(w != 0) takes a NaN weight up: in its row the accumulators its point feeds -- the six of its link and gRt --
    are NaN; every other row is finite and within the tolerance.  (The fold selects a link's entries by a 0 / 1 factor, so
    the row's other links turn NaN as well; the row's pose gradient is NaN either way and that is not asserted.)"""
    case = pbo.make_case(4, 600, 14, seed=950, density=0.5, fused=False)
    p = np.nonzero(pbo.contributing(case)[0])[0][7]
    l = int(case["link"][0, p])
    case["w"][0, p] = np.nan
    out = _run(gq, case)
    wr, g, _, bd = pbo.oracle_of(case)
    assert np.isnan(wr[0, l]).all() and np.isnan(g[0]).all() and np.isfinite(wr[1:]).all() and np.isfinite(g[1:]).all()
    assert np.isnan(out[0][0, l]).all() and np.isnan(out[1][0]).all()
    assert np.isfinite(out[0][1:]).all() and np.isfinite(out[1][1:]).all()
    rs = (_ratio(out[0][1:], wr[1:], bd["wrench"][1:]), _ratio(out[1][1:], g[1:], bd["gRt"][1:]))
    print(f"NaN weight, rows 1..3: max |hip - ref| / tol = {rs[0]:.3f}, {rs[1]:.3f}")
    assert max(rs) < 1.0


def test_refusals(gq):
    """Bad sizes and a missing e_pen are refused before anything is launched: RuntimeError, outputs untouched."""
    for fused, kw in ((False, {"L": 0}), (True, {"L": 0}), (False, {"L": 161}), (True, {"L": 161}), (True, {"e_pen": False})):
        case = pbo.make_case(3, 300, 14, seed=990, density=0.5, fused=fused)
        case["link"][:] = 0
        outs, err = _launch(gq, case, **kw)
        assert isinstance(err, RuntimeError), (fused, kw)
        for t in outs:
            assert t is None or bool((t == pbo.SENTINEL).all()), "a refused call must not write"
    outs, err = _launch(gq, pbo.make_case(3, 300, 160, seed=991, density=0.5), L=160)
    assert err is None  # the documented limit itself is accepted (test_link_groups checks its values)


# ---------------------------------------------------------------------------------------------------------------
# the fused roles (gq_stage_b_kernel / gq_stage_b_alt_kernel) on a scene that overflows the list
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("energy_type", ["graspqp", "dexgrasp"])
def test_fused_roles_equal_the_stand_alone_kernel(gq, consts, energy_type):
    """The "deep" scene of tests/test_gpu_large_batch.py (Allegro inside superquadric 0, 2500 surface points), eight rows,
    penetration_only = 1 and no point grid: the per-role launches (gq_hand_pen_forward + gq_hand_pen_backward) and the fused
    launches (gq_fc_pen_step, gq_alt_pen_step for "dexgrasp") give the same dis bit for bit, hence the same wrench, gRt and
    e_pen bit for bit, and both lie within the derived tolerance of the fp64 oracle fed with the GPU's own (dis, link, gvec).

    The translation factor: that scene's 0.15 leaves at most 343 of a row's 2500 points inside the hand, and 0.0 (the hand's
    origin -- its wrist -- at the object's centre) at most 738; the fingers fill the object only once the origin is past the
    centre.  With -0.2 every one of the eight rows has 1155 .. 1521 penetrating points (OracleHand.cal_distance on the CPU,
    fp64, 8 x 2500 points).  The precondition itself -- a row with more than GQ_PENB_LIST penetrating points among its first
    2560, so that the backward's list overflows -- is asserted on the dis > 0 of the penetration_only = 1 query that the
    backward consumes."""
    from bench import make_initial_state

    spec = get_hand_spec("allegro")
    be, n, P = 8, 12, 2500
    fv = meshes.superquadric(0)
    sp = meshes.surface_points(fv, P, oversample=4, seed=42)
    hp, idx = make_initial_state(spec, fv, be, n, 1000)
    hp[:, :3] *= -0.2
    hand = gq.ops.HandHandle(spec)
    st = gq.stepper.GraspStepper(hand, gq.ops.MeshSet([fv]), torch.tensor(sp[None]), be, n, seed=5, energy_type=energy_type)
    assert st._can_fuse and st.penetration_only == 1 and st.grid is None
    assert (st._alt_desc is not None) == (energy_type == "dexgrasp")
    st.pose_new.copy_(hp.cuda())
    st.idx_new.copy_(idx.cuda())
    outs = []
    for fused in (False, True):
        st.wrench.fill_(pbo.SENTINEL), st.gRt.fill_(pbo.SENTINEL), st.terms_new[2].fill_(pbo.SENTINEL)
        st._evaluate(st.pose_new, st.idx_new, gq.C.stream_ptr(), fused=fused)
        torch.cuda.synchronize()
        outs.append([t.clone().cpu().numpy() for t in (st.pen_dis, st.pen_link, st.pen_gvec, st.wrench, st.gRt, st.terms_new[2])])
    (dis, link, gvec, wrench, gRt, e_pen), fz = outs
    cnt = (dis[:, : consts["K_small"] * 256] > 0).sum(1)
    print(f"{energy_type}: penetrating points among the first {consts['K_small'] * 256}: {cnt.tolist()}")
    assert cnt.max() > consts["LIST"], "no row overflows the backward's list: shrink the translation factor"
    for name, a, b in zip(("dis", "link", "gvec", "wrench", "gRt", "e_pen"), outs[0], fz):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{name}: the fused role differs from the separate launches"
    for a in (wrench, gRt, e_pen):
        assert not (a == np.float32(pbo.SENTINEL)).any() and np.isfinite(a).all()
    wr, g, e, bd = pbo.oracle(sp[None].astype(np.float32), st.pose_new.cpu().numpy(), st.Rg.cpu().numpy(), link, gvec, hand.L, be,
                              dis=dis, w_pen=float(st.w["E_pen"]))
    rs = (_ratio(wrench, wr, bd["wrench"]), _ratio(gRt, g, bd["gRt"]), _ratio(e_pen, e, bd["e_pen"]))
    _worst["ratio"] = max(_worst["ratio"], *rs)
    print(f"{energy_type}: n_max={bd['n_max']}  max |hip - ref| / tol = wrench {rs[0]:.3f}, gRt {rs[1]:.3f}, e_pen {rs[2]:.3f}"
          f"   (all cases so far: {_worst['ratio']:.3f})")
    assert max(rs) < 1.0


# ---------------------------------------------------------------------------------------------------------------
# the forward's (dis, link, gvec) per point against the fp64 oracle
# ---------------------------------------------------------------------------------------------------------------
# python tests/_pen_scene.py, three nudge seeds, max(wrench, gRt) norm-wise: 1.53e-4, 1.16e-4, 1.90e-4 -> their median
NUDGE_BASELINE = 1.53e-4
BACKWARD_BOUND = 4 * NUDGE_BASELINE  # 6.1e-4


@pytest.fixture(scope="module")
def pen_scene(gq):
    spec, fvs, sps, hp, idx = psc.scene()
    o = psc.point_oracle(spec, hp, idx, np.repeat(sps.astype(np.float64), psc.BE, 0))
    hand = gq.ops.HandHandle(spec)
    pose, surf = hp.cuda().contiguous(), torch.tensor(sps).cuda().contiguous()
    B = pose.shape[0]
    Rg, LT, *_ = gq.ops.fk_contacts(pose, idx.cuda(), hand)
    return {"spec": spec, "hand": hand, "pose": pose, "surf": surf, "oracle": o, "B": B, "sps": sps,
            "Rg": Rg.reshape(B, 9).contiguous(), "LT": LT.reshape(B, hand.L, 12).contiguous(), "grid": gq.ops.PointGrid(surf, 8)}


@pytest.mark.parametrize("mode", [1, 0, "cells"])
def test_forward_offsets_and_links_against_the_oracle(gq, pen_scene, mode):
    """gq_hand_pen_forward with penetration_only = 1 and 0, and gq_hand_pen_forward_cells, per point against the fp64 oracle
    (tests/_pen_scene.py: the per-link stack of OracleHand.cal_distance, its arg-max, autograd's gradient rotated into the
    hand frame), on the scene of test_hand_penetration_and_self_penetration with P = 1024.

    Not the gradient direction: at shallow penetration a position noise of 3e-6 m turns it by more than 2e-3 without any tie.
    Compared is the offset vector dis gvec = x_h - c_h in metres: at every point with dis_o > 1e-5, |dis gvec - dis_o g_o|_inf
    <= 1e-5 m (the project's near-tie bound) and link == the oracle's winner.  At most 2e-3 of those points are excused (the
    project's disagreement cap), and every excused point must be a near-tie by the oracle's own numbers: the second-best
    link within 1e-5 m of the best, or |dis - dis_o| > 3e-6 already (a face swap).

    Then the oracle's triple, cast to fp32, and the GPU's own go through gq_hand_pen_backward: wrench and gRt agree norm-wise
    to BACKWARD_BOUND = 4 x the nudge baseline (python tests/_pen_scene.py: two fp32 casts of the oracle, the second at points
    moved by 3e-6 m, through the fp64 backward oracle; 4 x because the nudge models one kernel's noise and here two sources
    differ)."""
    s, C = pen_scene, gq.C
    o, B, P, hand = s["oracle"], s["B"], psc.P, s["hand"]
    dis = torch.empty(B, P, device="cuda")
    link = torch.zeros(B, P, dtype=torch.int32, device="cuda")
    gvec = torch.zeros(B, P, 3, device="cuda")
    if mode == "cells":
        C.call("gq_hand_pen_forward_cells", hand.links.handle, s["grid"].handle, C.f32(s["surf"]), psc.N_OBJ, P, psc.BE, C.f32(s["pose"]),
               s["pose"].shape[1], C.f32(s["Rg"]), C.f32(s["LT"]), C.f32(dis), C.i32(link), C.f32(gvec), None, None, C.stream_ptr())
    else:
        C.call("gq_hand_pen_forward", hand.links.handle, C.f32(s["surf"]), psc.N_OBJ, P, psc.BE, C.f32(s["pose"]), s["pose"].shape[1],
               C.f32(s["Rg"]), C.f32(s["LT"]), int(mode), C.f32(dis), C.i32(link), C.f32(gvec), None, 0, None, None, None, C.stream_ptr())
    torch.cuda.synchronize()
    d, l, g = dis.cpu().numpy(), link.cpu().numpy(), gvec.cpu().numpy()
    assert o["n_links"] == hand.L
    deep = o["dis"] > 1e-5
    assert deep.sum() > 1500, f"the scene must hold about 2000 penetrating points, has {deep.sum()}"
    off = np.abs(d.astype(np.float64)[..., None] * g - o["dis"][..., None] * o["g_h"]).max(-1)
    bad = deep & ((off > 1e-5) | (l != o["winner"]))
    near_tie = (o["dis"] - o["second"] < 1e-5) | (np.abs(d - o["dis"]) > 3e-6)
    print(f"mode {mode}: {deep.sum()} points with dis_o > 1e-5, excused {bad.sum()} (offset {int((deep & (off > 1e-5)).sum())}, "
          f"link {int((deep & (l != o['winner'])).sum())}), max offset error elsewhere {off[deep & ~bad].max():.3g} m")
    assert bad.sum() <= 2e-3 * deep.sum(), f"{bad.sum()} of {deep.sum()} points disagree with the oracle"
    assert near_tie[bad].all(), "a point disagrees with the oracle without being a near-tie"
    if mode != 0:  # the penetration-only queries write link / gvec only where dis > 0: the caller's zeros stay
        out = d <= 0
        assert out.any() and (l[out] == 0).all() and (g[out] == 0).all()
    # both triples through the backward kernel
    case = {"surf": s["sps"], "hand_pose": s["pose"].cpu().numpy(), "Rg": s["Rg"].cpu().numpy(), "w": None, "L": hand.L,
            "batch_each": psc.BE, "n_obj": psc.N_OBJ, "B": B, "P": P}
    do, lo, go = psc.fp32_triple(o)
    a = _run(gq, dict(case, dis=d, link=np.where(d > 0, l, 0).astype(np.int32), gvec=np.where((d > 0)[..., None], g, 0).astype(np.float32)))
    b = _run(gq, dict(case, dis=do, link=lo, gvec=go))
    rw, rg = psc.normwise(a[0], b[0].astype(np.float64)), psc.normwise(a[1], b[1].astype(np.float64))
    print(f"mode {mode}: backward of the GPU's triple against the oracle's: norm-wise wrench {rw:.3g}, gRt {rg:.3g} (bound {BACKWARD_BOUND:.3g})")
    assert max(rw, rg) <= BACKWARD_BOUND
