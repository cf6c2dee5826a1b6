"""GPU tests of the scene-aware initialisation (screened hull candidates; include/graspqp_hip.h): the selection kernel against the
numpy oracle of tests/_init_select_oracle.py, the candidate poses against the fp64 oracle of the initialisation and against the
unscreened route bit for bit, the scores against the stepper's own terms bit for bit, feasibility against the fp64 scene and
approach oracles, and the properties of the screened poses on the public surfaces (convex_hull_poses_screened, GraspStepper,
initialize_convex_hull).

Shared set-up: Allegro and Panda, 2 objects x 16 rows from 128 candidates per object on the hull of superquadric(40, 32, 16); 80^3
grids of 5 mm voxels centred on the object holding a half-space wall, free for x < c; margin 5 mm; approach over 0.10 m with 4
stations; 128 samples of the hand's surface.

Bounds: candidate poses 3e-5 abs, joint angles 2e-4 (tests/test_gpu_init.py); everything else is exact (bit for bit, or a
comparison of a penalty with 0).  In the feasibility test a candidate with a sample, or a station of a sample, whose phi lies
within _scene_oracle.NEAR of the margin is left out: there an fp32 kernel cannot be asked for the fp64 oracle's side; at most 5 %
of the candidates may be left out, asserted."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ref_cpu import init as oinit  # noqa: E402

import _approach_oracle as ao  # noqa: E402
import _init_select_oracle as oracle  # noqa: E402
import _scene_oracle as so  # noqa: E402
from graspqp_amd.hands import get_hand_spec  # noqa: E402
from graspqp_amd.utils import meshes  # noqa: E402

HANDS = ["allegro", "panda"]
N_OBJ, BE, M = 2, 16, 128
SHAPE, H = (80, 80, 80), 0.005
ORIGIN = (-0.5 * 79 * H,) * 3
MARGIN, AP_D, AP_K = 0.005, 0.10, 4
SELECT_CASES = oracle.cases()


@pytest.fixture(scope="module")
def gq():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from graspqp_amd import _C, ops, stepper
    from graspqp_amd.core import initializations as ini

    _C.lib()
    return type("gq", (), {"ops": ops, "C": _C, "stepper": stepper, "ini": ini})


@functools.lru_cache(maxsize=None)
def _object():
    fv = meshes.superquadric(40, 32, 16)
    return fv, oinit.convex_hull_faces(fv.reshape(-1, 3))


@functools.lru_cache(maxsize=None)
def _hulls(n_obj=N_OBJ):
    hull = _object()[1]
    fv = torch.tensor(np.concatenate([hull] * n_obj), dtype=torch.float32).cuda().contiguous()
    cdf = torch.tensor(np.concatenate([oinit.area_cdf(hull)] * n_obj), dtype=torch.float32).cuda().contiguous()
    off = torch.tensor(np.cumsum([0] + [len(hull)] * n_obj), dtype=torch.int32).cuda()
    return fv, cdf, off


@functools.lru_cache(maxsize=None)
def _hand(name):
    from graspqp_amd import ops

    hand = ops.HandHandle(get_hand_spec(name))
    pts, lnk = meshes.hand_surface_samples(hand.spec, 128)
    return hand, ops.SurfaceSamples(hand, pts, lnk), (pts, lnk)


@functools.lru_cache(maxsize=None)
def _wall(c):
    """Free for x < c: phi = c - x, reproduced exactly by every cell."""
    return so.Field(SHAPE, ORIGIN, H, analytic=lambda x: c - x[..., 0])


def _free():
    return so.Field(SHAPE, ORIGIN, H, values=torch.ones(SHAPE))


def _scene(gq, *fields):
    if len(fields) == 1:
        return fields[0].scene(gq)
    f = fields[0]
    return gq.ops.SceneSDFSet(torch.stack([g.values for g in fields]).cuda(), [float(o) for o in f.origin], float(f.voxel))


def _draws(spec, n_obj=N_OBJ, m=M, seed=1):
    """The generator order of convex_hull_poses_screened."""
    g = torch.Generator().manual_seed(seed)
    return {"u_face": torch.rand(n_obj, m, generator=g), "u_len": torch.rand(n_obj, m, 2, generator=g),
            "u_pose": torch.rand(n_obj * m, 4, generator=g), "u_joint": torch.rand(n_obj * m, spec.n_dofs, generator=g)}


def _approach(hand, weight=1.0):
    return dict(distance=AP_D, stations=AP_K, margin=MARGIN, axis=hand.spec.grasp_axis, weight=weight)


def _terms(gq, hand, samples, pose, scene):
    """E_scene and E_approach of rows through the class-surface ops (the routes that exist without this feature)."""
    hp = pose.detach().contiguous()
    idx = torch.zeros(hp.shape[0], 1, dtype=torch.long, device="cuda")
    Rg, LT, _, _, _, ws = gq.ops.fk_contacts(hp, idx, hand)
    es = gq.ops.scene_terms(hp, hand, samples, idx, Rg, LT, ws, scene, MARGIN)
    ea = gq.ops.approach_terms(hp, hand, samples, idx, Rg, LT, ws, scene, hand.spec.grasp_axis, AP_D, AP_K, MARGIN)
    return es, ea


# ---- 3. the selection kernel ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SELECT_CASES) + ["ten_points"])
def test_select_kernel_equals_the_oracle(gq, name):
    c = oracle.ten_point_case() if name == "ten_points" else SELECT_CASES[name]
    want, want_nf = oracle.select_all(c["points"], c["penalty"], c["K"], c["tol"])
    P, pen = torch.tensor(c["points"]).cuda(), torch.tensor(c["penalty"]).cuda()
    sel, nf = gq.ini.init_select(P, pen, c["K"], c["tol"])
    sel2, nf2 = gq.ini.init_select(P, pen, c["K"], c["tol"])
    torch.cuda.synchronize()
    assert nf.cpu().numpy().tolist() == want_nf.tolist(), name
    assert np.array_equal(sel.cpu().numpy(), want), name
    assert torch.equal(sel, sel2) and torch.equal(nf, nf2)
    if name == "ten_points":
        assert sel[0].tolist() == oracle.TEN_SEL


def test_select_with_everything_feasible_is_the_farthest_point_pass(gq):
    """Distinct points, penalty 0 everywhere: sel is what gq_init_convex_hull's farthest-point pass picks -- seen through the
    shell points of convex_hull_poses on the same samples."""
    spec = get_hand_spec("allegro")
    d = _draws(spec)
    _, cand_p, _ = gq.ini.hull_candidates(spec, _hulls(), N_OBJ, M, draws=d)
    sel, nf = gq.ini.init_select(cand_p.view(N_OBJ, M, 3), torch.zeros(N_OBJ, M, device="cuda"), BE)
    pick = lambda t: torch.gather(t.view(N_OBJ, M, -1).cuda(), 1, sel.long()[..., None].expand(-1, -1, t.shape[-1])).reshape(N_OBJ * BE, -1)
    _, sp, _ = gq.ini.convex_hull_poses(spec, _hulls(), N_OBJ, BE, draws={**d, "u_pose": pick(d["u_pose"]), "u_joint": pick(d["u_joint"])},
                                        samples_per_object=M, return_shell=True)
    assert nf.tolist() == [M] * N_OBJ and (sel[:, 0] == 0).all()
    assert torch.equal(sp, pick(cand_p))


# ---- 4. candidates against the fp64 oracle ----------------------------------------------------------------------------
@pytest.mark.parametrize("hand_name", HANDS)
def test_candidates_match_the_fp64_oracle(gq, hand_name):
    spec = get_hand_spec(hand_name)
    d = _draws(spec)
    pose, p, n = gq.ini.hull_candidates(spec, _hulls(), N_OBJ, M, draws=d)
    torch.cuda.synchronize()
    hull32 = _object()[1].astype(np.float32).astype(np.float64)  # the float32 hull the device sees
    ps, ns = [], []
    for i in range(N_OBJ):
        pts, f = oinit.sample_surface(hull32, d["u_face"][i].double(), d["u_len"][i].double())
        nrm = oinit.face_normals(hull32)[f]
        ps.append(pts + 0.01 * nrm)
        ns.append(-nrm)
    p_o, n_o = torch.cat(ps), torch.cat(ns)
    pose_o = oinit.poses_from_samples(spec, p_o, n_o, d["u_pose"].double(), d["u_joint"].double())
    assert pose.shape == (N_OBJ * M, 9 + spec.n_dofs)
    np.testing.assert_allclose(p.cpu().numpy(), p_o.numpy(), atol=2e-6)
    np.testing.assert_allclose(n.cpu().numpy(), n_o.numpy(), atol=2e-5)
    np.testing.assert_allclose(pose[:, :9].cpu().numpy(), pose_o[:, :9].numpy(), atol=3e-5)
    np.testing.assert_allclose(pose[:, 9:].cpu().numpy(), pose_o[:, 9:].numpy(), atol=2e-4)


# ---- 5. a free scene is the parent ------------------------------------------------------------------------------------
@pytest.mark.parametrize("hand_name", HANDS)
def test_free_scene_gives_the_unscreened_poses_bit_for_bit(gq, hand_name):
    hand, samples, _ = _hand(hand_name)
    spec = hand.spec
    d = _draws(spec)
    pose, info = gq.ini.convex_hull_poses_screened(hand, _hulls(), N_OBJ, BE, samples, _scene(gq, _free()), MARGIN, 1.0, _approach(hand),
                                                   draws=d, samples_per_object=M, return_info=True)
    assert info["n_feasible"].tolist() == [M] * N_OBJ
    assert float(info["penalty"].abs().max()) == 0.0
    sel = info["sel"].long()
    pick = lambda t: torch.gather(t.view(N_OBJ, M, -1).cuda(), 1, sel[..., None].expand(-1, -1, t.shape[-1])).reshape(N_OBJ * BE, -1)
    parent = gq.ini.convex_hull_poses(spec, _hulls(), N_OBJ, BE, draws={**d, "u_pose": pick(d["u_pose"]), "u_joint": pick(d["u_joint"])},
                                      samples_per_object=M)
    assert torch.equal(pose, parent)
    assert torch.equal(pose, pick(info["cand_pose"]))


# ---- 6. the scores are the stepper's ----------------------------------------------------------------------------------
def _stepper(gq, hand, raw, scene, weights, be=BE, seed=11, **kw):
    fv = _object()[0]
    sp = meshes.surface_points(fv, 300, oversample=4)
    st = gq.stepper.GraspStepper(hand, gq.ops.MeshSet([fv] * N_OBJ), torch.tensor(np.stack([sp] * N_OBJ)), be, 4, weights=weights,
                                 seed=seed, scene=scene, scene_margin=MARGIN, approach_distance=AP_D, approach_stations=AP_K,
                                 surface_samples=raw, **kw)
    st.set_hulls(_hulls())
    return st


@pytest.mark.parametrize("stack", [False, True], ids=["SceneSDF", "SceneSDFSet"])
@pytest.mark.parametrize("hand_name", HANDS)
def test_scores_are_the_steppers_terms_bit_for_bit(gq, hand_name, stack):
    hand, _, raw = _hand(hand_name)
    scene = _scene(gq, _wall(0.08), _wall(0.12)) if stack else _scene(gq, _wall(0.08))
    w = {"E_scene": 50.0, "E_approach": 20.0}
    st = _stepper(gq, hand, raw, scene, w)
    pose, info = gq.ini.convex_hull_poses_screened(hand, _hulls(), N_OBJ, BE, st.samples, scene, MARGIN, w["E_scene"],
                                                   _approach(hand, w["E_approach"]), draws=_draws(hand.spec), samples_per_object=M,
                                                   return_info=True)
    idx = torch.randint(hand.spec.n_contact_candidates, (N_OBJ * BE, 4), device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
    st.reset(pose, idx)
    sel = info["sel"].long()
    es, ea = info["e_scene"].gather(1, sel).reshape(-1), info["e_approach"].gather(1, sel).reshape(-1)
    assert torch.equal(st.terms[st.term_row("E_scene")], es) and torch.equal(st.terms[st.term_row("E_approach")], ea)
    assert float(info["e_scene"].max()) > 0 and float(info["e_approach"].max()) > 0  # the walls are met
    pen = w["E_scene"] * info["e_scene"].double() + w["E_approach"] * info["e_approach"].double()
    assert torch.equal(info["penalty"] <= 0, pen <= 0) and torch.allclose(info["penalty"].double(), pen, rtol=1e-6, atol=0)
    if stack:  # the nearer wall leaves fewer candidates
        assert int(info["n_feasible"][0]) < int(info["n_feasible"][1])


# ---- 7. feasibility against fp64 --------------------------------------------------------------------------------------
@pytest.mark.parametrize("hand_name", HANDS)
def test_feasibility_agrees_with_the_fp64_oracles(gq, hand_name):
    hand, samples, _ = _hand(hand_name)
    F = _wall(0.08)
    _, info = gq.ini.convex_hull_poses_screened(hand, _hulls(), N_OBJ, BE, samples, _scene(gq, F), MARGIN, 1.0, _approach(hand),
                                                draws=_draws(hand.spec), samples_per_object=M, return_info=True)
    hp = info["cand_pose"].cpu().double()  # the GPU's fp32 candidates
    pts, lnk = samples.points.cpu().numpy(), samples.link.cpu().numpy()
    rs = so.e_scene(hand.spec, pts, lnk, hp, F, MARGIN)
    ra = ao.e_approach(hand.spec, pts, lnk, hp, F, MARGIN, AP_D, AP_K)
    near_s = (rs["inside"] & (np.abs(rs["phi"] - MARGIN) < so.NEAR)).any(-1)
    near_a = (ra["inside"] & (np.abs(ra["phi"] - MARGIN) < so.NEAR)).any((-1, -2))
    keep = ~(near_s | near_a)
    ins = rs["inside"]
    print(f"[{hand_name}] {(~keep).sum()} of {keep.size} candidates left out; closest sample to the margin "
          f"{np.abs(rs['phi'][ins] - MARGIN).min():.2e} m; oracle feasible {int(((rs['E'] == 0) & (ra['E'] == 0)).sum())}, scene alone "
          f"{int((rs['E'] == 0).sum())}; kernel feasible {info['n_feasible'].tolist()}")
    assert (~keep).mean() <= 0.05
    want = (rs["E"] == 0) & (ra["E"] == 0)
    got = (info["penalty"] <= 0).reshape(-1).cpu().numpy()
    assert np.array_equal(got[keep], want[keep])
    assert np.array_equal((info["e_scene"] <= 0).reshape(-1).cpu().numpy()[~near_s], (rs["E"] == 0)[~near_s])
    assert 0 < want.sum() < want.size


# ---- 8. screened initial poses are collision-free, and the case is not empty -------------------------------------------
@pytest.mark.parametrize("hand_name", HANDS)
def test_screened_poses_are_collision_free_where_the_unscreened_are_not(gq, hand_name):
    hand, samples, _ = _hand(hand_name)
    scene = _scene(gq, _wall(0.08))
    gen = lambda: torch.Generator(device="cuda").manual_seed(1)
    plain = gq.ini.convex_hull_poses(hand.spec, _hulls(), N_OBJ, BE, generator=gen(), samples_per_object=M)
    es, _ = _terms(gq, hand, samples, plain, scene)
    assert float((es > 0).float().mean()) >= 0.25, "the unscreened route must start rows inside the wall"
    pose, info = gq.ini.convex_hull_poses_screened(hand, _hulls(), N_OBJ, BE, samples, scene, MARGIN, 1.0, _approach(hand), generator=gen(),
                                                   samples_per_object=M, return_info=True)
    print(f"[{hand_name}] unscreened rows with E_scene > 0: {int((es > 0).sum())} of {es.numel()}; n_feasible {info['n_feasible'].tolist()}")
    assert (info["n_feasible"] >= BE).all()
    es, ea = _terms(gq, hand, samples, pose, scene)
    assert pose.shape == (N_OBJ * BE, 9 + hand.spec.n_dofs)
    assert float(es.abs().max()) == 0.0 and float(ea.abs().max()) == 0.0
    again = gq.ini.convex_hull_poses_screened(hand, _hulls(), N_OBJ, BE, samples, scene, MARGIN, 1.0, _approach(hand), generator=gen(),
                                              samples_per_object=M, chunk_rows=50)
    assert torch.equal(again, pose), "the chunk size changes nothing"


# ---- 9. the fill order -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hand_name", HANDS)
def test_rows_beyond_the_feasible_ones_are_the_least_penalised(gq, hand_name):
    hand, samples, _ = _hand(hand_name)
    be = 48
    pose, info = gq.ini.convex_hull_poses_screened(hand, _hulls(), N_OBJ, be, samples, _scene(gq, _wall(0.04)), MARGIN, 1.0, None,
                                                   draws=_draws(hand.spec), samples_per_object=M, return_info=True)
    assert info["e_approach"] is None
    assert torch.equal(info["penalty"], info["e_scene"])  # weight 1, the approach term off: exactly the scene term
    pen, sel, nf = info["penalty"].cpu().numpy(), info["sel"].cpu().numpy(), info["n_feasible"].cpu().numpy()
    print(f"[{hand_name}] n_feasible {nf.tolist()} of {M}, be = {be}")
    for g in range(N_OBJ):
        assert 0 < nf[g] < be, "the case must need fills"
        picked = pen[g][sel[g]]
        assert len(set(sel[g].tolist())) == be
        assert (picked[:nf[g]] == 0).all()
        fills = picked[nf[g]:]
        assert (fills > 0).all() and (np.diff(fills) >= 0).all()
        rest = np.delete(pen[g], sel[g])
        assert picked.max() <= rest.min()


# ---- 10. the stepper ---------------------------------------------------------------------------------------------------
def test_stepper_initialises_and_resets_outside_the_obstacles(gq):
    """``initialize`` and the reset of ``run(7, reset_epochs=2)`` (at step 2, the only one: step < 7 - 4) take the screened route.
    The terms of the re-initialised rows are read in the callback of step 2: that is the iteration whose accept step takes the new
    poses unconditionally; the MALA* iterations that follow move them again."""
    hand, _, raw = _hand("allegro")
    w = {"E_scene": 50.0, "E_approach": 20.0}
    outs = []
    for _ in range(2):
        st = _stepper(gq, hand, raw, _scene(gq, _wall(0.08)), w, init_avoid_scene=True)
        st.initialize()
        assert st.init_feasible.dtype == torch.int32 and st.init_feasible.shape == (N_OBJ,) and st.init_feasible.is_cuda
        ok = (st.init_feasible >= BE).repeat_interleave(BE)
        assert ok.all(), "1600 candidates per object: every object has enough collision-free ones"
        assert float(st.terms[st.term_row("E_scene")][ok].abs().max()) == 0.0 and float(st.terms[st.term_row("E_approach")][ok].abs().max()) == 0.0
        seen = {}

        def at(step):
            if step == 2:
                seen["mask"] = st.reset_mask.clone()
                seen["terms"] = st.terms.clone()
                seen["ok"] = (st.init_feasible >= BE).repeat_interleave(BE)

        st.run(7, reset_epochs=2, callback=at)
        torch.cuda.synchronize()
        assert torch.isfinite(st.energy).all() and torch.isfinite(st.hand_pose).all() and torch.isfinite(st.terms).all()
        m = seen["mask"] & seen["ok"]
        assert int(m.sum()) > 0, "the schedule must actually reset rows"
        assert float(seen["terms"][st.term_row("E_scene")][m].abs().max()) == 0.0 and float(seen["terms"][st.term_row("E_approach")][m].abs().max()) == 0.0
        outs.append((st.hand_pose.clone(), st.energy.clone(), st.contact_idx.clone(), st.init_feasible.clone(), seen["mask"]))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_stepper_without_the_switch_is_the_parent_route(gq):
    hand, _, raw = _hand("allegro")
    scene = _scene(gq, _wall(0.08))
    st = _stepper(gq, hand, raw, scene, {"E_scene": 50.0}, seed=11)
    assert st.init_avoid_scene is False
    pose, idx = st.fresh_state()
    gen = torch.Generator(device="cuda").manual_seed(11)
    want = gq.ini.convex_hull_poses(hand.spec, _hulls(), N_OBJ, BE, None, gen, "cuda")
    want_idx = torch.randint(hand.spec.n_contact_candidates, (N_OBJ * BE, 4), device="cuda", generator=gen)
    assert torch.equal(pose, want) and torch.equal(idx, want_idx)
    assert int(st.init_feasible.abs().max()) == 0
    with pytest.raises(ValueError, match="init_avoid_scene"):
        _stepper(gq, hand, raw, scene, {}, init_avoid_scene=True)
    with pytest.raises(ValueError, match="init_avoid_scene"):
        _stepper(gq, hand, raw, None, None, init_avoid_scene=True)
    # the approach term alone is enough
    st = _stepper(gq, hand, raw, scene, {"E_approach": 20.0}, init_avoid_scene=True)
    st.initialize()
    assert (st.init_feasible >= BE).all() and float(st.terms[st.term_row("E_approach")].abs().max()) == 0.0


# ---- the class surface -------------------------------------------------------------------------------------------------
def test_initialize_convex_hull_with_the_flag(gq):
    from graspqp_amd.core.hand_model import HandModel
    from graspqp_amd.core.initializations import initialize_convex_hull
    from graspqp_amd.core.object_model import ObjectModel

    spec = get_hand_spec("allegro")
    fv = _object()[0]
    om = ObjectModel(batch_size_each=BE, num_samples=300)
    om.initialize_from_meshes([fv, fv], surface_points_list=[meshes.surface_points(fv, 300, oversample=4)] * 2)
    hm = HandModel(spec, "cuda")
    args = SimpleNamespace(n_contact=4, init_avoid_scene=True)
    with pytest.raises(ValueError, match="set_scene"):
        initialize_convex_hull(hm, om, args, generator=torch.Generator(device="cuda").manual_seed(3))
    scene = _scene(gq, _wall(0.08))
    hm.set_scene(scene, MARGIN)
    hm.set_approach(AP_D, AP_K)
    pose, idx = initialize_convex_hull(hm, om, args, generator=torch.Generator(device="cuda").manual_seed(3))
    assert pose.shape == (N_OBJ * BE, 9 + spec.n_dofs) and idx.shape == (N_OBJ * BE, 4) and hm.hand_pose.requires_grad
    _, pts, lnk = hm._surface_handle()
    es, ea = _terms(gq, hm._hand, gq.ops.SurfaceSamples(spec, pts, lnk), pose, scene)
    assert float(es.abs().max()) == 0.0 and float(ea.abs().max()) == 0.0
    # without the flag: the parent's poses on the same generator
    plain, _ = initialize_convex_hull(hm, om, SimpleNamespace(n_contact=4), generator=torch.Generator(device="cuda").manual_seed(3))
    want = gq.ini.convex_hull_poses(spec, om.convex_hulls(), N_OBJ, BE, None, torch.Generator(device="cuda").manual_seed(3), "cuda")
    assert torch.equal(plain.detach(), want)
