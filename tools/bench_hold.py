"""Timing of the payload-holding launch.  Evidence run, not a test: one JSON record is printed and written to --out.

  launch   gq_hold_terms with every output (E, resid, x, force, torque, g_contact_pts) replayed from a captured graph at 256 and 2 048
           rows, L in {1, 3, 8} loads, nz in {48, 96} columns (12 contacts x 4 / 8 cone edges), T = 16, Allegro.  Beside it the same
           quantity composed from existing ops in the same call: the cone matrix and p assembled in torch, the low-rank box QP
           ``graspqp_amd::lsq_box_qp`` with T iterations on the B L problems, V, r and the forces in torch, gq_contact_jacobian and an
           einsum for J' R' f (no gradient on that side: it is the cheaper half of the comparison).  The composed route is replayed
           from a captured graph too when it captures, else launched eagerly (``composed_mode`` says which).  HIP events around
           --calls replays per window, the two routes alternating, medians of --rounds windows.
  stepper  GraspStepper.hold() end to end (flush, FK forward, object query, the launch) at 1 x 256 and 8 x 256 rows on the bench
           scene, host clock around calls that end in a synchronise.

usage: python tools/bench_hold.py [--calls 100] [--rounds 3] [--out file.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=100)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--rows", default="256,2048")
ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "hold_bench.json"))
args = ap.parse_args()

from graspqp_amd import ops
from graspqp_amd.hands import get_hand_spec
from graspqp_amd.stepper import GraspStepper
from graspqp_amd.utils import meshes

assert torch.cuda.is_available(), "this tool runs on the GPU"
spec = get_hand_spec("allegro")
hand = ops.HandHandle(spec)
MU, TW, RIDGE, T, U, N = 0.5, 5.0, 1e-4, 16, 10.0, 12
ACC = ((0, 0, 0), (3, 0, 0), (0, -3, 2), (0, 0, 6), (-4, 1, 0), (2, 2, -2), (0, 5, 0), (-1, -1, -5))


def cone_matrix(cp, nrm_out, cog, k):
    """F (B,6,n k) in torch: the cone column of csrc/fc_dev.h on the inward normals."""
    n = -nrm_out
    b1 = torch.full_like(n, 0.57735026918962576)
    dot = (b1 * n).sum(-1) / (n.norm(dim=-1) + 1e-6)
    b1[..., 1] = torch.where(dot > 0.9, b1[..., 1] - 2.0, b1[..., 1])
    t1 = torch.linalg.cross(n, b1, dim=-1)
    t2 = torch.linalg.cross(n, t1, dim=-1)
    cc = float(np.sqrt(1.0 - MU * MU))
    cols = []
    for e in range(k):
        if k == 4:
            s = MU if e < 2 else -MU
            dr = s * t2 if e & 1 else s * t1
        else:
            ang = 6.283185307179586 / k * e
            dr = MU * (float(np.cos(ang)) * t1 + float(np.sin(ang)) * t2)
        f = (dr + cc * n) / k
        cols.append(torch.cat([f, TW * torch.linalg.cross(cp - cog[:, None], f, dim=-1)], -1))
    F = torch.stack(cols, 2)
    return F.reshape(F.shape[0], -1, 6).transpose(1, 2).contiguous()


def window(fn, n_calls):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    ev0.record()
    for _ in range(n_calls):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    return 1e3 * ev0.elapsed_time(ev1) / n_calls  # us


def captured(fn):
    """fn replayed from a graph; None if it does not capture."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(g):
            fn()
    except Exception as ex:  # noqa: BLE001 -- recorded, the eager route is timed instead
        print(f"[bench_hold] the composed route does not capture ({type(ex).__name__}); timed eagerly", flush=True)
        torch.cuda.synchronize()
        return None
    return g.replay


rec = {"hold_bench": True, "hand": "allegro", "n_contact": N, "iterations": T, "friction": MU, "max_force": U, "rounds": args.rounds,
       "calls_per_window": args.calls, "device": torch.cuda.get_device_name(0), "e_fc_head_us_per_row": 27.7, "launch": {}}
gen = torch.Generator().manual_seed(0)
for B in map(int, args.rows.split(",")):
    hp = torch.cat([0.12 * torch.nn.functional.normalize(torch.randn(B, 3, generator=gen), dim=-1), torch.randn(B, 6, generator=gen),
                    torch.tensor(spec.default_state)[None] + 0.1 * torch.randn(B, spec.n_dofs, generator=gen)], 1).float().cuda()
    idx = torch.randint(spec.n_contact_candidates, (B, N), generator=gen).cuda()
    d = torch.nn.functional.normalize(torch.randn(B, N, 3, generator=gen), dim=-1)
    cog = (0.01 * torch.randn(B, 3, generator=gen)).cuda()
    nrm = d.cuda().contiguous()
    cp = (cog[:, None] + 0.05 * nrm).contiguous()
    Rg, LT, _, _, _, ws = ops.fk_contacts(hp, idx, hand)
    Rg, LT = Rg.contiguous(), LT.contiguous()
    for k in (4, 8):
        nz = N * k
        for L in (1, 3, 8):
            lw = ops.hold_check(hand, N, k, ops.hold_loads(0.5, accelerations=ACC[:L]), U, RIDGE, T, MU, TW).cuda()
            z = lambda *s: torch.zeros(*s, device="cuda")
            e, resid, x, force, torque, g = z(B), z(B, L), z(B, L, nz), z(B, L, N, 3), z(B, L, hand.J), z(B, N, 3)

            def fused():
                ops._hold_call(hand, idx, Rg, LT, ws, nrm, cp, cog, lw, B, k, MU, TW, U, RIDGE, T, None, None, 1.0, e, resid, x, force,
                               torque, None, 0, g)

            w = torch.cat([lw[0, :, :3], TW * lw[0, :, 3:]], -1)  # (L,6)

            def composed():
                F = cone_matrix(cp, nrm, cog, k)  # (B,6,nz)
                A = F[:, None].expand(B, L, 6, nz).reshape(B * L, 6, nz)
                b = -w[None].expand(B, L, 6).reshape(B * L, 6)
                xs = ops.lsq_box_qp(A, b, 0.0, U, RIDGE, eps=0.0, max_iter=T).view(B, L, nz)
                r = torch.einsum("bin,bln->bli", F, xs) + w[None]
                ww = (w * w).sum(-1)
                V = (r * r).sum(-1) + RIDGE * (xs * xs).sum(-1)
                fo = (F[:, None, :3].transpose(-1, -2) * xs.unsqueeze(-1)).view(B, L, N, k, 3).sum(3)
                jc = ops.contact_jacobian(hand, idx, LT, ws)  # (B,n,3,JA)
                fh = torch.einsum("bji,blcj->blci", Rg, fo)
                return (V / ww).mean(-1), torch.sqrt((r * r).sum(-1) / ww), fo, torch.einsum("bcia,blci->bla", jc, fh)

            fused()
            e_c, resid_c, fo_c, tq_c = composed()
            torch.cuda.synchronize()
            agree = {"E_max_abs": float((e - e_c).abs().max()), "resid_max_abs": float((resid - resid_c).abs().max()),
                     "force_max_abs_N": float((force - fo_c).abs().max()), "torque_max_abs_Nm": float((torque - tq_c).abs().max())}
            fns = {"gq_hold_terms": captured(fused)}
            cg = captured(composed)
            fns["composed_route"] = cg or composed
            for fn in fns.values():
                for _ in range(10):
                    fn()
            t = {key: [] for key in fns}
            for _ in range(args.rounds):
                for key, fn in fns.items():
                    t[key].append(window(fn, args.calls))
            r_ = {key: {"median_us": float(np.median(v)), "min_us": min(v), "max_us": max(v)} for key, v in t.items()}
            r_.update({"rows": B, "loads": L, "nz": nz, "composed_mode": "graph" if cg else "eager", "agreement": agree,
                       "us_per_problem": r_["gq_hold_terms"]["median_us"] / (B * L),
                       "us_per_row": r_["gq_hold_terms"]["median_us"] / B,
                       "launch_over_composed": r_["gq_hold_terms"]["median_us"] / r_["composed_route"]["median_us"]})
            rec["launch"][f"{B}x{L}x{nz}"] = r_
            print(json.dumps({f"{B}x{L}x{nz}": r_}), flush=True)

# ---- GraspStepper.hold() end to end --------------------------------------------------------------------------------------------
rec["stepper_hold"] = {}
for n_obj in (1, 8):
    fvs = [meshes.superquadric(o) for o in range(n_obj)]
    sps = [meshes.surface_points(f, 2500, oversample=4, seed=42) for f in fvs]
    st = GraspStepper(hand, ops.MeshSet(fvs), torch.tensor(np.stack(sps)), 256, N, seed=3)
    g2 = torch.Generator().manual_seed(1)
    B = st.B
    hp = torch.cat([0.12 * torch.nn.functional.normalize(torch.randn(B, 3, generator=g2), dim=-1), torch.randn(B, 6, generator=g2),
                    torch.tensor(spec.default_state)[None] + 0.1 * torch.randn(B, spec.n_dofs, generator=g2)], 1).float().cuda()
    st.reset(hp, torch.randint(spec.n_contact_candidates, (B, N), generator=g2).cuda())
    lw = ops.hold_loads(0.5, accelerations=ACC[:3])
    for _ in range(5):
        st.hold(lw, U)
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        for _ in range(20):
            h = st.hold(lw, U)
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0) / 20)
    rec["stepper_hold"][f"{n_obj}x256"] = {"rows": B, "loads": 3, "nz": N * int(st.fc["n_cone_vecs"]), "ms_per_call_median": float(np.median(ts)),
                                           "ms_per_call_min": min(ts), "ms_per_call_max": max(ts), "E_hold_mean": float(h.e.mean()),
                                           "rows_with_resid_below_5_percent": int((h.resid.amax(1) <= 0.05).sum())}
    print(json.dumps({"stepper_hold": rec["stepper_hold"]}), flush=True)
    del st
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
print(json.dumps(rec), flush=True)
