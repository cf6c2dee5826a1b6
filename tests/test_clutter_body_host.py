"""The device body of the compose kernel (csrc/clutter_dev.h: one output node and the tile's conservative cull, on top of
scene_dev.h's interpolant) compiled for the HOST with AddressSanitizer and UBSan, run as a program and compared with the fp64
oracle (tests/_clutter_oracle.py) at the bound of the GPU tests (rtol 1e-5 / atol 1e-6).  Every grid is held in a
buffer of exactly its size, so a node read outside it, or a float -> int conversion of an out-of-range value, ends the program;
the program itself fails if the cull changes a single bit.  No GPU involved."""
import subprocess

import numpy as np
import pytest
import torch

import _host_program
import _clutter_oracle as co
import _scene_oracle as so



@pytest.fixture(scope="module")
def body(tmp_path_factory):
    d = tmp_path_factory.mktemp("clutter_body")
    exe = _host_program.build("clutter_body_host", d)

    def grid_bytes(F):
        return (np.array(F.shape, dtype=np.int32).tobytes() + np.array(list(F.origin) + [F.voxel], dtype=np.float32).tobytes()
                + F.values.numpy().tobytes())

    def run(out, target_T, parts, part_T, exclude, base, far):
        ex = np.full(out.n_grids, -1, dtype=np.int32) if exclude is None else exclude.numpy().astype(np.int32)
        with open(d / "in.bin", "wb") as f:
            f.write(np.array((out.n_grids,) + out.shape, dtype=np.int32).tobytes())
            f.write(np.array(list(out.origin) + [out.voxel, far], dtype=np.float32).tobytes())
            f.write(target_T.numpy().astype(np.float32).tobytes())
            f.write(ex.tobytes())
            f.write(np.array([len(parts), int(base is not None)], dtype=np.int32).tobytes())
            f.write(part_T.numpy().astype(np.float32).tobytes())
            for F in list(parts) + ([base] if base is not None else []):
                f.write(grid_bytes(F))
        subprocess.check_call([exe, str(d / "in.bin"), str(d / "out.bin")])
        raw = np.fromfile(d / "out.bin", dtype=np.float32)
        n = out.n_grids * int(np.prod(out.shape))
        culled, pairs = raw[n:].view(np.int32)
        return raw[:n].reshape((out.n_grids,) + out.shape), int(culled), int(pairs)

    return run


def _close(got, ref, tag):
    ref = ref.numpy()
    assert np.array_equal(np.isnan(got), np.isnan(ref)), tag
    ok = ~np.isnan(ref)
    print(f"[{tag}] max abs err {np.abs(got[ok] - ref[ok]).max():.3e} (max |phi| {np.abs(ref[ok]).max():.3e})")
    np.testing.assert_allclose(got[ok], ref[ok], rtol=1e-5, atol=1e-6, err_msg=tag)


@pytest.mark.parametrize("with_base", [True, False])
@pytest.mark.parametrize("kind,seed", [("affine", co.SEEDS[0]), ("random", co.SEEDS[0]), ("random", co.SEEDS[1])])
def test_compose_body_matches_the_oracle(body, kind, seed, with_base):
    out, tT, parts, pT, ex, base = co.layout(seed, kind)
    base = base if with_base else None
    ref, info = co.compose(out, tT, parts, pT, ex, base, co.FAR)
    print(f"[{kind} {seed} base={with_base}] guards: nearest boundary plane {info['edge']:.2e} cells, inside {info['inside']:.3f}")
    if kind == "random":
        assert info["edge"] >= co.EDGE and info["inside"] >= 0.10, info
    got, _, _ = body(out, tT, parts, pT, ex, base, co.FAR)
    _close(got, ref, f"{kind} {seed} base={with_base}")
    assert (got < co.FAR).mean() >= 0.2  # the parts are seen


def test_shape_beyond_one_tile_and_a_part_out_of_reach(body):
    """(5,9,17) nodes: two tiles along x and z, three along y, none of them full.  A part far from every target is culled for
    every tile and changes nothing."""
    out, tT, parts, pT, ex, base = co.layout(co.SEEDS[0], "random", out_shape=co.OUT_SHAPE_TILES)
    ref, info = co.compose(out, tT, parts, pT, ex, base, co.FAR)
    assert info["edge"] >= co.EDGE and info["inside"] >= 0.10, info
    got, culled, pairs = body(out, tT, parts, pT, ex, base, co.FAR)
    _close(got, ref, "(5,9,17)")
    assert pairs == 3 * 2 * 3 * 2 * 3
    far_T = pT.clone()
    far_T[1, :, 3] = torch.tensor([0.5, -0.5, 0.5])
    got_far, culled_far, _ = body(out, tT, parts, far_T, ex, base, co.FAR)
    got_without, culled_without, _ = body(out, tT, [parts[0], parts[2]], pT[[0, 2]], torch.tensor([0, -1, 1], dtype=torch.int32), base, co.FAR)
    assert np.array_equal(got_far, got_without)
    assert culled_far == culled_without + 3 * 2 * 3 * 2 and 0 < culled < culled_far  # each of the 36 tiles leaves it out
    _close(got_far, co.compose(out, tT, parts, far_T, ex, base, co.FAR)[0], "part out of reach")


def test_non_finite_and_huge_target_poses(body):
    """Targets whose translation holds NaN, +inf, -inf: every node NaN; 3e38: finite, outside every volume, ``far``.  The
    first target is ordinary and unaffected."""
    out, tT, parts, pT, _, base = co.layout(co.SEEDS[0], "random")
    out = co.Out(5, out.shape, out.origin, out.voxel)
    T = tT[[0, 0, 1, 2, 1]].clone()
    T[1, 0, 3], T[2, 1, 3], T[3, 2, 3], T[4, 0, 3] = float("nan"), float("inf"), float("-inf"), 3e38
    ex = torch.tensor([0, -1, 2, 1, -1], dtype=torch.int32)
    ref, _ = co.compose(out, T, parts, pT, ex, base, co.FAR)
    got, _, _ = body(out, T, parts, pT, ex, base, co.FAR)
    _close(got, ref, "special poses")
    assert np.isnan(got[1:4]).all() and (got[4] == np.float32(co.FAR)).all() and np.isfinite(got[0]).all()
    # a NaN in a part's pose: every node that includes the part is NaN, the target that excludes it is not
    bad = pT.clone()
    bad[2, 1, 1] = float("nan")
    got, _, _ = body(co.Out(3, out.shape, out.origin, out.voxel), tT, parts, bad, torch.tensor(co.EXCLUDE, dtype=torch.int32), base, co.FAR)
    assert np.isnan(got[0]).all() and np.isnan(got[1]).all() and np.isfinite(got[2]).all()


def test_a_nan_node_value_is_not_dropped_by_the_min(body):
    out, tT, parts, pT, ex, base = co.layout(co.SEEDS[0], "random")
    v = parts[1].values.clone()
    v[1, 2, 2] = float("nan")
    poisoned = so.Field(parts[1].shape, parts[1].origin, parts[1].voxel, values=v)
    ref, _ = co.compose(out, tT, [parts[0], poisoned, parts[2]], pT, ex, base, co.FAR)
    got, _, _ = body(out, tT, [parts[0], poisoned, parts[2]], pT, ex, base, co.FAR)
    assert np.isnan(ref.numpy()).sum() >= 10 and np.array_equal(np.isnan(got), np.isnan(ref.numpy()))
