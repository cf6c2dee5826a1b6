"""The contact queries inside the FK forward launch with sized box slots (csrc/sdf_dev.h: KC; csrc/kin.hip:
gq_fk_forward_slots_kernel<KC>, three clusters per round; csrc/fk_slots.h: which kernel serves a mesh set).

What can go wrong here are slot boundaries, not the batch size: B = 4 rows, n = 12 contacts, Allegro, meshes whose cluster counts
sit on the dispatch edges (1, 64 | 65, 128 | 129, 192 | 193 -> the four-slot kernel, 300 -> its second pass), the last cluster of
each five faces short, two-mesh sets in which the larger mesh decides KC whichever position it has, the Allegro palm (sliver
faces) and the zoo's mesh with zero-area faces.  The search is exact whatever KC and the clusters per round are, so the four
outputs must be the BITS of the stand-alone query (gq_sdf_forward_meshset: four slots, four clusters per round) on the same
contact points -- hands a decimetre away and hands whose fingers reach through the surface -- and every query must have been
answered with at least one and at most all clusters visited (gq_debug_set_pen_counters, words 0 and 1)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _sdf_set_oracle as so  # noqa: E402
from graspqp_amd.hands import get_hand_spec  # noqa: E402
from graspqp_amd.utils import meshes  # noqa: E402

B, N_CONTACT = 4, 12


@functools.lru_cache(maxsize=None)
def _sphere5():
    return meshes.icosphere(5)


def _open_sphere(n_clusters):
    """The first 64 nC - 5 faces of the 20480-face icosphere: nC clusters, the last one partly filled."""
    return np.ascontiguousarray(_sphere5()[: 64 * n_clusters - 5])


# name -> (meshes, kernel that must serve the set: box slots KC, or 0 = gq_fk_forward_kernel with four slots)
SETS = {f"nC{c}": ((c,), kc) for c, kc in ((1, 1), (64, 1), (65, 2), (128, 2), (129, 3), (192, 3), (193, 0), (300, 0))}
SETS["two_meshes_1_and_129"] = ((1, 129), 3)   # the larger mesh decides
SETS["two_meshes_65_and_64"] = ((65, 64), 2)   # ... whichever position it has
SETS["allegro_palm"] = (("palm",), 1)          # sliver faces (fillet strips), 324 faces
SETS["degenerate_sliver"] = (("degenerate_sliver",), 1)  # zero-area faces and needles among 1350 faces


def _set(name):
    def one(m):
        if m == "palm":
            return np.ascontiguousarray(get_hand_spec("allegro").link_faces(0), dtype=np.float32)
        return so.mesh(m) if isinstance(m, str) else _open_sphere(m)

    return [one(m) for m in SETS[name][0]], SETS[name][1]


@pytest.fixture(scope="module")
def gq():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from graspqp_amd import _C, ops

    _C.lib()
    return type("gq", (), {"ops": ops, "C": _C, "hand": ops.HandHandle(get_hand_spec("allegro"))})


def _n_clusters(fv):
    return (len(fv) + 63) // 64


def _poses(spec, fvs, seed, radius):
    """Row r grasps at mesh r // (B / n_mesh): the hand ``radius`` from the centre of the mesh's box."""
    g = torch.Generator().manual_seed(seed)
    be = B // len(fvs)
    ctr = np.repeat(np.stack([0.5 * (f.reshape(-1, 3).min(0) + f.reshape(-1, 3).max(0)) for f in fvs]), be, 0)
    t = torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=-1) * radius + torch.tensor(ctr, dtype=torch.float32)
    th = torch.tensor(spec.default_state, dtype=torch.float32)[None] + 0.3 * torch.randn(B, spec.n_dofs, generator=g)
    return torch.cat([t, torch.randn(B, 6, generator=g), th], 1)


@pytest.mark.parametrize("name", list(SETS))
def test_slot_kernels_give_the_bits_of_the_stand_alone_query(gq, name):
    fvs, kc = _set(name)
    C, hand = gq.C, gq.hand
    n_max = max(_n_clusters(f) for f in fvs)
    assert (64 * (kc - 1) < n_max <= 64 * kc) if kc else n_max > 192  # the table above says what fk_slots.h says
    ms, be, dev = gq.ops.MeshSet(fvs), B // len(fvs), "cuda"
    idx = torch.randint(hand.spec.n_contact_candidates, (B, N_CONTACT), generator=torch.Generator().manual_seed(2)).to(dev)
    Rg, LT = torch.empty(B, 9, device=dev), torch.empty(B, hand.L, 12, device=dev)
    cp, cn = torch.empty(B, N_CONTACT, 3, device=dev), torch.empty(B, N_CONTACT, 3, device=dev)
    ws, nb = hand.fk_ws(B, dev)
    out = [torch.empty(B * N_CONTACT, device=dev), torch.empty(B * N_CONTACT, dtype=torch.int32, device=dev),
           torch.empty(B * N_CONTACT, 3, device=dev), torch.empty(B * N_CONTACT, 3, device=dev)]
    sd = C.SdfDesc()
    sd.meshes, sd.queries_per_mesh = ms.handle, be * N_CONTACT
    sd.dist_sq, sd.sign, sd.obj_dir, sd.closest = (t.data_ptr() for t in out)
    cnt = torch.zeros(12, dtype=torch.int64, device=dev)
    for radius in (0.1, 0.0):  # a decimetre off, as the fit starts; and the palm at the centre: fingers through the surface
        pose = _poses(hand.spec, fvs, 31, radius).to(dev)
        out[0].fill_(float("nan"))  # a query nobody answers shows
        out[1].fill_(-77)
        cnt.zero_()
        C.call("gq_debug_set_pen_counters", ctypes.c_void_p(cnt.data_ptr()))
        try:
            C.call("gq_fk_forward", hand.handle, C.f32(pose), C.i64(idx), B, N_CONTACT, C.f32(Rg), C.f32(LT), C.f32(cp), C.f32(cn),
                   None, 0.0, None, None, None, ctypes.byref(sd), C.ptr(ws), nb, C.stream_ptr())
            torch.cuda.synchronize()
        finally:
            C.call("gq_debug_set_pen_counters", None)
        visits, queries = int(cnt[0]), int(cnt[1])
        alone = gq.ops.sdf_meshset(cp.reshape(-1, 3), ms, be * N_CONTACT)
        for got, ref, what in zip(out, alone, ("dist_sq", "sign", "obj_dir", "closest")):
            assert torch.equal(got.view(torch.int32).reshape(-1), ref.contiguous().view(torch.int32).reshape(-1)), (name, radius, what)
        assert torch.isfinite(out[0]).all() and ((out[1] == 1) | (out[1] == -1)).all(), (name, radius)
        assert queries == B * N_CONTACT and queries <= visits <= sum(_n_clusters(f) for f in fvs) * be * N_CONTACT, (name, visits, queries)
