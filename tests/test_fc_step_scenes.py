"""The scenes of tests/test_gpu_fc_step_routes.py keep their teeth (CPU, oracle only).

Section 2 of that module puts ONE late row H into a batch of copies of an early row E and asks the fused step for the
n_iter of the two-row batch [E, H].  That only tests the batch-global stop rule if H really holds the batch back: a step
that drops H's record stops with E, at least three iterations earlier -- more than anything the fp32 arithmetic can move
n_iter by -- and a step that never stops early reports max_iter.  Both have to stay distinguishable if _scenes.py changes.
Section 1 relies on the contact-term inputs being in general position."""
import numpy as np
import pytest
import torch

import _fc_step_case as fsc
from _scenes import hetero_contacts


@pytest.mark.parametrize("n,k", fsc.STOP_SHAPES)
def test_late_row_holds_the_batch_back(n, k):
    pts, nrm, cog, n_e, n_h = fsc.stop_scene(n, k)
    got = {}
    for dtype in (torch.float64, torch.float32):
        both = fsc.oracle_fc(pts, nrm, cog, k, fsc.STOP_EPS, fsc.STOP_MAX_ITER, dtype)[3]
        e_only = fsc.oracle_fc(pts[:1], nrm[:1], cog[:1], k, fsc.STOP_EPS, fsc.STOP_MAX_ITER, dtype)[3]
        h_only = fsc.oracle_fc(pts[1:], nrm[1:], cog[1:], k, fsc.STOP_EPS, fsc.STOP_MAX_ITER, dtype)[3]
        # H first or last: the rule folds the rows with max / any / min
        swapped = fsc.oracle_fc(pts.flip(0), nrm.flip(0), cog.flip(0), k, fsc.STOP_EPS, fsc.STOP_MAX_ITER, dtype)[3]
        got[dtype] = (e_only, both, h_only)
        assert swapped == both
        assert e_only + 3 <= both < fsc.STOP_MAX_ITER, (n, k, dtype, e_only, both)
    print(f"n={n} k={k}: n_iter of E alone {got[torch.float64][0]}, of [E, H] {got[torch.float64][1]}, of H alone {got[torch.float64][2]}")
    assert got[torch.float64] == got[torch.float32], got
    assert got[torch.float64][0] == n_e and got[torch.float64][2] == n_h
    # a larger iteration budget (the max_iter = 16 and 17 cases) changes nothing: the rule has fired before
    for mi in (16, 17):
        assert fsc.oracle_fc(pts, nrm, cog, k, fsc.STOP_EPS, mi, torch.float64)[3] == got[torch.float64][1]


@pytest.mark.parametrize("n", [5, 13])
def test_general_contact_inputs_are_general(n):
    pts, nrm, _ = (t.float().double() for t in hetero_contacts(16, n, seed=9000 + 3 * n))
    c = fsc.general_contact_inputs(pts, nrm, seed=n)
    for v in c.values():
        assert torch.equal(v.float().to(v.dtype), v), "inputs must be exact in fp32"
    sg = c["sign"]
    assert ((sg == 1) | (sg == -1)).all() and (sg == 1).any(1).all() and (sg == -1).any(1).all()
    d2 = c["dist_sq"]
    assert (d2 == 0).any(1).all() and d2.max() <= 1e-3 and d2[d2 > 0].min() >= 0.99e-10
    assert torch.allclose(sg.double().unsqueeze(-1) * c["obj_dir"], nrm)
    cos = (c["hand_normals"] * c["obj_dir"]).sum(-1)
    assert cos.abs().max() < 0.9999 and np.isclose(torch.linalg.norm(c["hand_normals"], dim=-1).numpy(), 1.0, atol=1e-6).all()
    off = torch.linalg.norm(pts - c["closest"], dim=-1)
    assert off.min() >= 0.9e-4, "p - closest must not vanish: the E_dis gradient of every contact is non-zero"
    gp, gn = fsc.contact_term_closed_form(c, pts, 100.0, torch.float64)
    assert torch.linalg.norm(gp, dim=-1).min() > 0 and torch.linalg.norm(gn, dim=-1).min() > 0
