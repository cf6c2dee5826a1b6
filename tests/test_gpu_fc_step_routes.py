"""gq_fc_step, the fused force-closure step of GraspStepper: every dispatch route against the fp64 oracle.

csrc/fcstep.hip picks one of eight kernel instantiations:

  columns per lane NC   1 | 2                       nz = n_contact * n_cone <= 64 | > 64
  stop rule             TAIL    replayed per row by the tail, gq_fc_tail_kernel<NC, 4>          max_iter <= 16, B <= 256
                        HEAD    epilogue of the head block that finishes last,
                                gq_fc_head_stop_kernel<NC> + gq_fc_tail_kernel<NC, 0>           max_iter <= 16, B > 256
                        LAUNCH  gq_qp_stop_launch_ between gq_fc_head_kernel<NC> and
                                gq_fc_tail_kernel<NC, 0>                                        max_iter > 16

Section 1 holds NC x {TAIL, HEAD} to the oracle at a FIXED iteration count (eps = 0, max_iter = 1 and 3: the stop rule
cannot fire), where fp32 and fp64 agree to a few ulps times the conditioning, with contact-term inputs in general position
(tests/_fc_step_case.py::general_contact_inputs) and three weightings: E_fc alone, E_dis alone, both -- the tail ADDS its
gradient to the head's.  HEAD runs 259 rows: 65 head blocks, one more than a wavefront has lanes, the last with 3 rows.

Section 2 holds the batch-global stop rule where it runs in each route: a batch of copies of an early row E with ONE late
row H at the positions where the rule's folds change hands (first, last, either side of the 64-record lane wrap of the
epilogue's fold, its second trip, a partial last block).  The rule sees max / any / min over the rows, so n_iter has to
be that of the two-row batch [E, H] wherever H sits; tests/test_fc_step_scenes.py keeps the scene's teeth (E alone stops
>= 3 iterations earlier).  LAUNCH and both sides of max_iter = 16 | 17 are here.

Every launch goes through tests/_fc_step_case.py::run: one guard row behind every output, sentinels in front of it.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ref_cpu import span as ospan  # noqa: E402

import _fc_step_case as fsc  # noqa: E402
from _parity import assert_tail_within_fp32_noise, rel_err  # noqa: E402
from _scenes import hetero_contacts  # noqa: E402
from test_gpu_fc_tail_slot import _qp_stop  # noqa: E402
from test_gpu_qp_variants import FC_CFGS, FC_TOL_E, FC_TOL_G, FWD_CEIL, FWD_FLOOR, NOISE_MULT  # noqa: E402

# Measured on the MI355X (batch maxima over all cases of section 1), beside the bounds they are held to:
#   FC_TOL_E = 1e-5   E_fc rel err       NC = 1: TAIL 1.6e-6  HEAD 2.4e-6   NC = 2: TAIL 2.6e-6  HEAD 2.6e-6
#   FC_TOL_G = 1e-5   d E_fc / d pts     NC = 1: TAIL 1.6e-6  HEAD 1.6e-6   NC = 2: TAIL 4.9e-7  HEAD 1.1e-6
#   forward rule (NOISE_MULT = 16 x oracle fp32 noise within [FWD_FLOOR, FWD_CEIL]); error, and error / oracle fp32 noise:
#     x_sum  NC = 1: TAIL 2.7e-7 (1.1 x)  HEAD 3.7e-7 (1.1 x)   NC = 2: TAIL 1.6e-7 (0.9 x)  HEAD 2.6e-7 (0.9 x)
#     F x    NC = 1: TAIL 3.8e-6 (0.5 x)  HEAD 3.8e-6 (0.7 x)   NC = 2: TAIL 1.2e-6 (0.4 x)  HEAD 2.1e-6 (0.6 x)
#     val    NC = 1: TAIL 1.7e-6 (1.3 x)  HEAD 3.1e-6 (1.4 x)   NC = 2: TAIL 3.2e-6 (0.8 x)  HEAD 3.2e-6 (1.1 x)
#     svd    NC = 1: TAIL 1.5e-7 (1.0 x)  HEAD 1.8e-7 (1.3 x)   NC = 2: TAIL 1.3e-7 (0.7 x)  HEAD 1.8e-7 (1.2 x)
#   (HEAD runs all 16 base rows, TAIL the first five.)
CONTACT_MULT = NOISE_MULT  # contact terms: 16 x the error of the closed form in torch fp32 on the CPU, per vector,
CONTACT_FLOOR = FWD_FLOOR  # floor 2e-6; measured, relative to the vector's norm: g_cpts <= 2.2e-7, g_cnrm <= 2.4e-7 on
#                            every route (the fp32 closed form itself: <= 2.8e-7 and <= 2.5e-7)
# Section 2 (converged, default eps), every route, measured: E_fc rel err <= 1.1e-7 at NC = 1 and 5.6e-7 at NC = 2 (oracle
# fp32: 1.9e-7 and 4.0e-5), x bit-identical to the box QP's best iterate, gradient <= 1.8e-7 of its norm.

W_DIS = 100.0  # the stepper's E_dis weight


@pytest.fixture(scope="module")
def gq():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from graspqp_amd import _C, ops

    _C.lib()
    return ops


def _rowerr(a, ref):
    """per-row inf-norm error relative to the inf norm of the fp64 reference row"""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    a, ref = a.reshape(a.shape[0], -1), ref.reshape(ref.shape[0], -1)
    return np.abs(a - ref).max(-1) / np.maximum(np.abs(ref).max(-1), 1e-30)


def _vecerr(a, ref):
    """per-vector (last axis) 2-norm error relative to the norm of the fp64 reference vector"""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return np.linalg.norm(a - ref, axis=-1) / np.linalg.norm(ref, axis=-1)


def _rows_identical(out, groups, what):
    """every output of the rows of a group carries the same bits"""
    for name in ("e_fc", "val", "svd", "x", "x_sum", "obj_normal", "g_cpts", "g_cnrm", "F"):
        a = out[name].cpu().numpy() if name == "F" else out[name]
        a = np.ascontiguousarray(a).reshape(a.shape[0], -1).view(np.uint32)
        for rows in groups:
            bad = np.nonzero((a[rows] != a[rows[0]]).any(1))[0]
            assert bad.size == 0, f"{what}: {name} of rows {[int(rows[b]) for b in bad[:6]]} differs from row {int(rows[0])}, a copy of the same input"


def _same_launch(a, b, what):
    for name in fsc.OUTPUTS:
        assert fsc.same_bits(a[name], b[name]), f"{what}: {name} differs between two launches on the same workspace"
    assert torch.equal(a["F"], b["F"]), f"{what}: F differs between two launches on the same workspace"


# ---------------------------------------------------------------------------------------------------------------
# 1: fixed iteration count, NC x {TAIL, HEAD}
# ---------------------------------------------------------------------------------------------------------------
SHAPES = ((5, 3), (12, 4), (16, 4), (13, 5), (11, 6), (8, 8), (16, 8))  # nz = 15, 48, 64, 65, 66, 64, 128
CFGS = {"cfg0": FC_CFGS[0], "cfg1": FC_CFGS[1], "default": fsc.FC_DEFAULT}
FIXED = [(n, k, c) for n, k in SHAPES for c in ("cfg0", "cfg1")] + [(12, 4, "default")]
ROUTE_ROWS = {"TAIL": 5, "HEAD": 259}  # 259 = 64 * 4 + 3: 65 head blocks, the last one partial
N_BASE = 16
_fixed_ref = {}


class _Ref:
    pass


def _span(r, k, cfg, k_it, dtype):
    c = lambda t: t.to(dtype)
    with torch.no_grad():
        val, svd, x, F = ospan.span_metric(c(r.pts), c(r.nrm), c(r.cog), mu=cfg["friction"], k=k, max_limit=cfg["max_limit"],
                                           torque_weight=cfg["torque_weight"], eps=0.0, maxIter=k_it, box_form=True)
    Fx = (F @ x.unsqueeze(-1)).squeeze(-1)
    return tuple(t.double().numpy() for t in (val, svd, Fx))


def _reference(n, k, cfg_name, k_it):
    """the 16 base rows, the oracle in fp64 and in fp32 and the closed form of the contact terms, once per case"""
    key = (n, k, cfg_name, k_it)
    if key not in _fixed_ref:
        cfg = CFGS[cfg_name]
        r = _Ref()
        r.pts, r.nrm, r.cog = (t.float().double() for t in hetero_contacts(N_BASE, n, seed=9000 + n * k))
        r.c = fsc.general_contact_inputs(r.pts, r.nrm, seed=77 + n * k)
        assert torch.equal(r.c["sign"].double().unsqueeze(-1) * r.c["obj_dir"], r.nrm)  # the oracle's object normals
        for dtype, tag in ((torch.float64, "64"), (torch.float32, "32")):
            e, g, xs, n_it = fsc.oracle_fc(r.pts, r.nrm, r.cog, k, 0.0, k_it, dtype, cfg)
            assert n_it == k_it
            setattr(r, "o" + tag, dict(e=e, g=g, xs=xs, **dict(zip(("val", "svd", "Fx"), _span(r, k, cfg, k_it, dtype)))))
        r.ct64 = [t.numpy() for t in fsc.contact_term_closed_form(r.c, r.pts, W_DIS, torch.float64)]
        r.ct32 = [t.double().numpy() for t in fsc.contact_term_closed_form(r.c, r.pts, W_DIS, torch.float32)]
        _fixed_ref[key] = r
    return _fixed_ref[key]


def _fwd_rule(what, err, noise):
    """the forward rule of tests/test_gpu_qp_variants.py on batch maxima"""
    e, e32 = float(np.max(err)), float(np.max(noise))
    tol = min(max(NOISE_MULT * e32, FWD_FLOOR), FWD_CEIL)
    assert e <= tol, f"{what}: err {e:.3g} > tol {tol:.3g} (oracle fp32 noise {e32:.3g})"
    return f"{e:.2e}|{e / max(e32, 1e-30):.2g}x"


@pytest.mark.parametrize("route", list(ROUTE_ROWS))
@pytest.mark.parametrize("k_it", [1, 3])
@pytest.mark.parametrize("n,k,cfg_name", FIXED)
def test_fixed_iterations_against_the_oracle(gq, n, k, cfg_name, k_it, route):
    cfg, B = CFGS[cfg_name], ROUTE_ROWS[route]
    assert (B <= 256) == (route == "TAIL") and k_it <= 16  # the dispatch of csrc/fcstep_dev.h::gq_fc_step_fill
    r = _reference(n, k, cfg_name, k_it)
    idx = torch.arange(B) % N_BASE
    ins = [r.c[name][idx] for name in ("dist_sq", "sign", "obj_dir", "closest")] + [r.pts[idx], r.c["hand_normals"][idx], r.cog[idx]]
    what = f"fc_step {route} n={n} k={k} NC={1 + (n * k > 64)} it={k_it} {cfg_name}"
    groups = [np.arange(b, B, N_BASE) for b in range(N_BASE) if b + N_BASE < B]
    ws, outs = None, {}
    for tag, w_dis, w_fc in (("A", 0.0, 1.0), ("B", W_DIS, 0.0), ("C", W_DIS, 1.0)):
        o = fsc.run(gq, n, k, cfg, 0.0, k_it, w_dis, w_fc, *ins, ws=ws)
        ws = o["ws"]
        again = fsc.run(gq, n, k, cfg, 0.0, k_it, w_dis, w_fc, *ins, ws=ws)  # not re-zeroed: the head's block counter is back at zero
        _same_launch(o, again, f"{what} launch {tag}")
        assert int(o["n_iter"][0]) == k_it, f"{what} launch {tag}: n_iter {int(o['n_iter'][0])}"
        _rows_identical(o, groups, f"{what} launch {tag}")
        assert fsc.same_bits(o["obj_normal"], (r.c["sign"].unsqueeze(-1) * r.c["obj_dir"])[idx].float().numpy()), \
            f"{what} launch {tag}: obj_normal is not sign * obj_dir"
        for name in ("e_fc", "val", "svd", "x", "x_sum"):  # the forward knows no weight
            assert fsc.same_bits(o[name], outs.get("A", o)[name]), f"{what}: {name} of launch {tag} differs from launch A"
        outs[tag] = o
    A, Bo, C = outs["A"], outs["B"], outs["C"]
    ix = idx.numpy()

    # A: E_fc alone, against the oracle
    er = rel_err(A["e_fc"], r.o64["e"][ix])
    gr = np.linalg.norm((A["g_cpts"] - r.o64["g"][ix]).reshape(B, -1), axis=1) / np.linalg.norm(r.o64["g"][ix].reshape(B, -1), axis=1)
    assert not A["g_cnrm"].any(), f"{what}: g_cnrm != 0 at w_dis = 0"
    Fx = (A["F"].cpu().double() @ torch.from_numpy(A["x"]).double().unsqueeze(-1)).squeeze(-1).numpy()
    fwd = []
    for name, hip in (("x_sum", A["x_sum"]), ("Fx", Fx), ("val", A["val"]), ("svd", A["svd"])):
        ref = r.o64["xs" if name == "x_sum" else name]
        fwd.append(name + " " + _fwd_rule(f"{what} {name}", _rowerr(hip, ref[ix]), _rowerr(r.o32["xs" if name == "x_sum" else name], ref)))

    # B: E_dis alone, against the closed form of gq_contact_term
    cp, cn = _vecerr(Bo["g_cpts"], r.ct64[0][ix]), _vecerr(Bo["g_cnrm"], r.ct64[1][ix])
    cp32, cn32 = _vecerr(r.ct32[0], r.ct64[0])[ix], _vecerr(r.ct32[1], r.ct64[1])[ix]
    print(f"MEASURED {what}: E_fc {er.max():.2e} g_cpts {gr.max():.2e} | {' '.join(fwd)} | contact g_cpts {cp.max():.2e} "
          f"(fp32 closed form {cp32.max():.2e}) g_cnrm {cn.max():.2e} (fp32 closed form {cn32.max():.2e})")
    assert er.max() <= FC_TOL_E, f"{what}: E_fc rel err {er.max():.3g} (row {int(er.argmax())})"
    assert gr.max() <= FC_TOL_G, f"{what}: d E_fc / d contact points err {gr.max():.3g} (row {int(gr.argmax())})"
    for name, e, e32 in (("g_cpts", cp, cp32), ("g_cnrm", cn, cn32)):
        bad = np.argwhere(e > np.maximum(CONTACT_MULT * e32, CONTACT_FLOOR))
        assert bad.size == 0, f"{what} E_dis {name}: (row, contact) {bad[:4].tolist()} err {e[tuple(bad[0])]:.3g}, fp32 closed form {e32[tuple(bad[0])]:.3g}"

    # C: both; the tail adds its part to the head's
    assert fsc.same_bits(C["g_cnrm"], Bo["g_cnrm"]), f"{what}: g_cnrm of launch C differs from launch B"
    a, b = A["g_cpts"].astype(np.float64), Bo["g_cpts"].astype(np.float64)
    assert (np.linalg.norm(a, axis=-1) > 0).all() and (np.linalg.norm(b, axis=-1) > 0).all(), f"{what}: a contact without E_fc or E_dis gradient"
    ulp = np.spacing(np.maximum(np.abs(A["g_cpts"]), np.abs(Bo["g_cpts"]))).astype(np.float64)  # fp32 ulp of the larger term
    d = np.abs(C["g_cpts"].astype(np.float64) - (a + b))
    bad = np.argwhere(d > ulp)
    assert bad.size == 0, (f"{what}: g_cpts(w_dis, w_fc) != g_cpts(w_dis, 0) + g_cpts(0, w_fc) at (row, contact, axis) {bad[:4].tolist()}: "
                           f"{d[tuple(bad[0])]:.3g} > one ulp {ulp[tuple(bad[0])]:.3g}")


# ---------------------------------------------------------------------------------------------------------------
# 2: the batch-global stop rule in every route, the deciding row at every position
# ---------------------------------------------------------------------------------------------------------------
def _stop_cases():
    out = []
    for route, Bs, mis in (("TAIL", (1, 6, 256), (12, 16)), ("HEAD", (257, 259, 515), (12, 16)), ("LAUNCH", (6, 259), (17,))):
        for B in Bs:
            pos = {0, B - 1}
            if route == "HEAD":
                pos |= {255, 256}  # head blocks 63 and 64: either side of the lane wrap of the epilogue's fold
                if B == 515:
                    pos |= {512}  # block 128: the fold's second trip, whose partner record is the clamped duplicate
            for mi in mis:
                out += [pytest.param(route, B, mi, p, id=f"{route}-B{B}-mi{mi}-H{p}") for p in sorted(pos)]
    return out


_stop_ref, _all_e = {}, {}
POISON_ROWS = 2048  # 512 head blocks on 256 compute units


def _stop_oracle(n, k, rows, max_iter):
    """fp64 and fp32 oracle on the rows ``rows`` of the scene [E, H] -> ((e, g, n_iter) in fp64, (e, g, n_iter) in fp32)"""
    key = (n, k, tuple(rows), max_iter)
    if key not in _stop_ref:
        pts, nrm, cog = (t[list(rows)] for t in fsc.stop_scene(n, k)[:3])
        res = []
        for dtype in (torch.float64, torch.float32):
            e, g, _, n_it = fsc.oracle_fc(pts, nrm, cog, k, fsc.STOP_EPS, max_iter, dtype)
            res.append((e, g, n_it))
        _stop_ref[key] = tuple(res)
    return _stop_ref[key]


def _stop_launch(gq, n, k, idx, max_iter):
    pts, nrm, cog = (t[idx] for t in fsc.stop_scene(n, k)[:3])
    d2, sg, od, cl, hn = fsc.plain_contact_inputs(pts, nrm)
    return fsc.run(gq, n, k, fsc.FC_DEFAULT, fsc.STOP_EPS, max_iter, 0.0, 1.0, d2, sg, od, cl, pts, hn, cog)


@pytest.mark.parametrize("route,B,max_iter,pos", _stop_cases())
@pytest.mark.parametrize("n,k", fsc.STOP_SHAPES)
def test_stop_rule_with_the_deciding_row_at(gq, n, k, route, B, max_iter, pos):
    assert route == ("LAUNCH" if max_iter > 16 else "TAIL" if B <= 256 else "HEAD")  # csrc/fcstep_dev.h::gq_fc_step_fill
    what = f"fc_step {route} n={n} k={k} NC={1 + (n * k > 64)} B={B} max_iter={max_iter} H at {pos}"
    # without H the batch stops with E: a step that always runs to the end, or to H's count, fails here
    if (n, k, B, max_iter) not in _all_e:
        if route == "HEAD":
            # first a batch of H only, large enough to leave H's per-row record in the LDS of every compute unit: the
            # last head block of the launch that follows is partial, and a fold over the records of wavefronts that
            # never ran would pick up what the LDS still holds -- H's record, which holds the batch back
            n_h = int(_stop_launch(gq, n, k, torch.ones(POISON_ROWS, dtype=torch.long), max_iter)["n_iter"][0])
            assert n_h == _stop_oracle(n, k, (1,), max_iter)[0][2], f"{what}: n_iter of {POISON_ROWS} copies of H {n_h}"
        _all_e[(n, k, B, max_iter)] = int(_stop_launch(gq, n, k, torch.zeros(B, dtype=torch.long), max_iter)["n_iter"][0])
    n_e = _stop_oracle(n, k, (0,), max_iter)[0][2]
    assert _all_e[(n, k, B, max_iter)] == n_e, f"{what}: n_iter of {B} copies of E {_all_e[(n, k, B, max_iter)]}, oracle {n_e}"

    idx = torch.zeros(B, dtype=torch.long)
    idx[pos] = 1
    present = sorted(set(idx.tolist()))  # B = 1: H alone
    (e64, g64, n64), (e32, _, n32) = _stop_oracle(n, k, present, max_iter)
    assert n64 == n32 and (len(present) == 1 or n_e + 3 <= n64 < max_iter)
    o = _stop_launch(gq, n, k, idx, max_iter)
    n_iter = int(o["n_iter"][0])
    assert n_iter == n64, f"{what}: n_iter {n_iter}, oracle on [E, H] {n64} (E alone {n_e})"
    e_rows = np.nonzero(idx.numpy() == 0)[0]
    if e_rows.size > 1:
        _rows_identical(o, [e_rows], what)
    rows = [int(e_rows[0]), pos] if len(present) == 2 else [pos]  # one E row and H, in the oracle's order
    # E_fc of E and of H under the rule of _parity.py
    re_, ne = rel_err(o["e_fc"][rows], e64), rel_err(e32, e64)
    assert_tail_within_fp32_noise(re_, ne, f"{what} E_fc")
    # x, sharp: the best iterate among 0..k* that the library's box QP selects on the step's F at the same eps
    n_qp, _ = _qp_stop(gq, o["F"][rows].contiguous(), fsc.STOP_EPS, 3, max_iter)
    x_qp = _qp_stop.x.cpu().double().numpy()
    assert n_qp == n_iter, f"{what}: the box QP on the step's F stops after {n_qp}"
    dx = np.abs(o["x"][rows] - x_qp).max(-1) / np.abs(x_qp).max(-1)
    assert dx.max() <= 1e-6, f"{what}: x of {'EH'[int(dx.argmax())] if len(rows) == 2 else 'H'} is not the best iterate among 0..k* ({dx.max():.3g})"
    # the converged gradient: 2e-2 norm-wise as everywhere in the suite
    ge = np.linalg.norm(o["g_cpts"][rows] - g64) / np.linalg.norm(g64)
    print(f"MEASURED {what}: n_iter {n_iter} (E alone {n_e}) E_fc rel err {re_.max():.2e} (oracle fp32 {ne.max():.2e}) x {dx.max():.2e} gradient {ge:.2e}")
    assert ge < 2e-2, f"{what}: gradient err {ge:.3g}"
