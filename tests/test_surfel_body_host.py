"""The device body of the TSDF surfel extraction (csrc/surfel_dev.h: tile fill, crossing test, stencil normal) compiled for the
HOST with AddressSanitizer and UBSan, run as a program of its own and compared with the fp64 oracle (tests/_surfel_oracle.py)
under the bounds and conditions of the GPU test: the count and the order exactly, positions at rtol 1e-5 / atol 1e-6, normals by
angle within 4 x the oracle's own float32-to-float64 angle (at least 1e-5 rad) on the non-ambiguous edges.  The volume, the
weight, the tile and the outputs are allocations of exactly their size, so a node or slot touched outside one ends the program
with a non-zero status.  No GPU involved."""
import subprocess

import numpy as np
import pytest

import _host_program
import _surfel_oracle as so

SENTINEL = np.float32(-7777.0)


@pytest.fixture(scope="module")
def body(tmp_path_factory):
    d = tmp_path_factory.mktemp("surfel_body")
    exe = _host_program.build("surfel_body_host", d)

    def run(D, W, origin, voxel, trunc, min_weight=1.0, region=None, capacity=0):
        """-> (points (G,capacity,3), normals (G,capacity,3), count (G,2)); capacity 0 is the counting call.  A sanitizer report
        or any other failure of the program raises (check_call)."""
        D = np.asarray(D, dtype=np.float32)
        G = D.shape[0]
        f4, i4 = (lambda a: np.asarray(a, dtype=np.float32).tobytes()), (lambda a: np.asarray(a, dtype=np.int32).tobytes())
        with open(d / "in.bin", "wb") as f:
            f.write(i4(D.shape) + f4(list(origin) + [voxel]) + i4([W is not None, region is not None, capacity]) + f4([min_weight, trunc]))
            if region is not None:
                f.write(i4(region))
            f.write(f4(D))
            if W is not None:
                f.write(f4(W))
        subprocess.check_call([exe, str(d / "in.bin"), str(d / "out.bin")])  # a sanitizer report is a non-zero exit
        raw = np.fromfile(d / "out.bin", dtype=np.float32)
        n = G * capacity * 3
        assert raw.size == 2 * G + 2 * n
        return raw[2 * G:2 * G + n].reshape(G, capacity, 3), raw[2 * G + n:].reshape(G, capacity, 3), raw[:2 * G].view(np.int32).reshape(G, 2)

    return run


def _exact(body, D, W, origin, voxel, trunc, min_weight=1.0, region=None):
    """The counting call, then the call of exactly that size (what extract_clouds does)."""
    _, _, count = body(D, W, origin, voxel, trunc, min_weight, region, 0)
    assert (count[:, 1] == 0).all()
    cap = max(int(count[:, 0].max()), 1)
    P, N, count2 = body(D, W, origin, voxel, trunc, min_weight, region, cap)
    assert np.array_equal(count2[:, 0], count[:, 0]) and np.array_equal(count2[:, 1], count[:, 0])
    for g in range(D.shape[0]):  # slots beyond the count are not touched
        assert (P[g, count[g, 0]:] == SENTINEL).all() and (N[g, count[g, 0]:] == SENTINEL).all()
    return P, N, count2


def test_one_cell(body):
    D, W, origin, voxel, trunc, mw, region, _ = so.tiny()
    P, N, count = _exact(body, D, W, origin, voxel, trunc, mw, region)
    ref = so.assert_parity(P, N, count, D, W, origin, voxel, trunc, mw, region, "(2,2,2)")
    assert len(ref[0]["edges"]) >= 4 and set(ref[0]["edges"][:, 3]) == {2}  # the four z edges of the cell


@pytest.mark.parametrize("name,min_weight", [("A", 1.0), ("B", 1.0), ("sphere", 1.0), ("sphere", 2.0)])
def test_body_matches_the_oracle_on_fused_volumes(body, name, min_weight):
    D, W, origin, voxel, trunc = so.fused(name)
    P, N, count = _exact(body, D, W, origin, voxel, trunc, min_weight)
    so.assert_parity(P, N, count, D, W, origin, voxel, trunc, min_weight, None, f"{name} min_weight {min_weight}")
    assert int(count[:, 0].sum()) >= 50 and (count[:, 0] > 0).all(), count  # the case does not pass empty
    if name == "A":  # crossings whose b lies in the next tile along x and y (along z: the hand-made volume "seam_z")
        e = so.extract(D, W, origin, voxel, trunc, min_weight)[0]["edges"]
        for c in range(2):
            assert ((e[:, 3] == c) & (e[:, c] % so.TILE[c] == so.TILE[c] - 1)).any(), c


@pytest.mark.parametrize("name", sorted(so.hand_made()))
def test_hand_made_volumes(body, name):
    D, W, origin, voxel, trunc, mw, region, want = so.hand_made()[name]
    P, N, count = _exact(body, D, W, origin, voxel, trunc, mw, region)
    ref = so.assert_parity(P, N, count, D, W, origin, voxel, trunc, mw, region, name)[0]
    if want is not None:
        assert int(count[0, 0]) == want
    if name == "lonely_pairs":
        assert int(ref["fallback"].sum()) == 1
        got = {tuple(e): tuple(n) for e, n in zip(ref["edges"].tolist(), N[0].tolist())}
        assert got[(4, 3, 4, 2)] == (0.0, 0.0, -1.0) and got[(4, 1, 12, 0)] == (1.0, 0.0, 0.0)
        assert np.allclose(got[(2, 2, 4, 1)], (0.0, -1.0, 0.0), atol=1e-6)
    if name == "seam_z":
        assert ((ref["edges"][:, 3] == 2) & (ref["edges"][:, 2] == 15)).sum() >= 20
    if name == "one_pair":
        assert ref["edges"].tolist() == [[2, 1, 8, 2]]
    if name in ("zero", "non_finite", "min_weight_2"):  # the rule changes the result: not the plain volume's
        base = so.hand_made()["no_weight"]
        assert int(count[0, 0]) != len(so.extract(base[0], None, origin, voxel, trunc)[0]["edges"]) or name == "zero"
    if name == "zero":  # the exact zero is a crossing's free end: t = 0 puts the surfel on the node
        e = ref["edges"]
        hit = [r for r in range(len(e)) if tuple(e[r, :3]) == (2, 2, 8)]
        assert hit and all(np.allclose(P[0, r], np.float32(origin) + np.float32(voxel) * np.array([2, 2, 8]), atol=1e-7) for r in hit)


def test_a_region_is_the_whole_extraction_filtered(body):
    D, W, origin, voxel, trunc = so.fused("A")
    region = (1, 8, 2, 7, 3, 17)
    P, N, count = _exact(body, D, W, origin, voxel, trunc, 1.0, region)
    so.assert_parity(P, N, count, D, W, origin, voxel, trunc, 1.0, region, "region")
    Pa, Na, ca = _exact(body, D, W, origin, voxel, trunc)
    e = so.extract(D, W, origin, voxel, trunc)[0]["edges"]
    b = e[:, :3] + np.eye(3, dtype=np.int64)[e[:, 3]]
    lo, hi = np.array(region[0::2]), np.array(region[1::2])
    keep = ((e[:, :3] >= lo) & (e[:, :3] < hi) & (b >= lo) & (b < hi)).all(1)
    assert 0 < keep.sum() < len(e) and count[0, 0] == keep.sum()
    assert np.array_equal(P[0].view(np.int32), Pa[0][keep].view(np.int32)) and np.array_equal(N[0].view(np.int32), Na[0][keep].view(np.int32))


@pytest.mark.parametrize("name", ["A", "B"])
def test_capacity_below_the_total(body, name):
    D, W, origin, voxel, trunc = so.fused(name)
    full_P, full_N, full = _exact(body, D, W, origin, voxel, trunc)
    cap = int(full[:, 0].min()) - 9  # below every grid's total, inside a tile's run of crossings
    assert cap >= 10
    P2, N2, count2 = body(D, W, origin, voxel, trunc, 1.0, None, cap)  # buffers of exactly (G,cap,3): ASan guards their end
    assert np.array_equal(count2[:, 0], full[:, 0]) and (count2[:, 1] == cap).all()
    assert np.array_equal(P2.view(np.int32), full_P[:, :cap].view(np.int32)) and np.array_equal(N2.view(np.int32), full_N[:, :cap].view(np.int32))
    so.assert_parity(P2, N2, count2, D, W, origin, voxel, trunc, 1.0, None, f"{name} capacity {cap}", capacity=cap)
