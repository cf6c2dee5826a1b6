"""The device bodies of the ESDF (csrc/edt_dev.h: tile geometry, seed, envelope, finish) compiled for the HOST with
AddressSanitizer and UBSan, run as a program of its own and compared with the fp64 brute-force oracle (tests/_esdf_oracle.py)
under the bound of the GPU test: rtol 1e-5 / atol 1e-6 on every node, in-band and void nodes bit for bit.  The volume, the
intermediate buffers, the output and every tile are allocations of exactly their size, so a node or an LDS word touched outside one
ends the program with a non-zero status.  No GPU involved, and nothing is loaded into Python under a sanitizer."""
import subprocess

import numpy as np
import pytest

import _host_program
import _esdf_oracle as eo
import _surfel_oracle as so



@pytest.fixture(scope="module")
def body(tmp_path_factory):
    d = tmp_path_factory.mktemp("esdf_body")
    exe = _host_program.build("esdf_body_host", d)

    def run(D, voxel, trunc, max_distance):
        """-> phi float32 of D's shape.  A sanitizer report or any other failure of the program raises (check_call)."""
        D = np.asarray(D, dtype=np.float32)
        stack = D if D.ndim == 4 else D[None]
        with open(d / "in.bin", "wb") as f:
            f.write(np.asarray(stack.shape, dtype=np.int32).tobytes() + np.asarray([voxel, trunc, max_distance], dtype=np.float32).tobytes())
            f.write(np.ascontiguousarray(stack).tobytes())
        subprocess.check_call([exe, str(d / "in.bin"), str(d / "out.bin")])  # a sanitizer report is a non-zero exit
        return np.fromfile(d / "out.bin", dtype=np.float32).reshape(D.shape)

    return run


@pytest.mark.parametrize("name", ["A", "B"])
def test_body_matches_the_oracle_on_fused_volumes(body, name):
    D, _, _, voxel, trunc = so.fused(name)
    phi, info = eo.assert_parity(body(D, voxel, trunc, 0.06), D, voxel, trunc, 0.06, name)
    for i in info:  # the case does not pass hollow
        mid = i["out"] & (i["e"] > np.float32(trunc)) & (i["e"] < np.float32(0.06))
        assert i["crossings"] >= 50 and i["band"].mean() >= 0.10 and mid.mean() >= 0.25, (name, i["crossings"], i["band"].mean(), mid.mean())


@pytest.mark.parametrize("name", ["sphere", "plane"])
def test_body_matches_the_oracle_on_analytic_volumes(body, name):
    D, _, voxel, trunc = eo.analytic(name)
    eo.assert_parity(body(D, voxel, trunc, 0.08), D, voxel, trunc, 0.08, name)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_long_lines(body, axis):
    D, voxel, trunc, dmax = eo.long_lines(axis)
    _, info = eo.assert_parity(body(D, voxel, trunc, dmax), D, voxel, trunc, dmax, f"long axis {axis}")
    e = info[0]["e"] / voxel
    assert info[0]["crossings"] >= 100 and (e > 60).any() and ((e > 60) & (e < eo.LONG_R)).any() and (e > eo.LONG_R).any()


@pytest.mark.parametrize("name", sorted(eo.hand_made()))
def test_hand_made_volumes(body, name):
    D, voxel, trunc, dmax = eo.hand_made()[name]
    eo.assert_parity(body(D, voxel, trunc, dmax), D, voxel, trunc, dmax, name)


def test_a_stack_is_its_grids(body):
    D, _, _, voxel, trunc = so.fused("B")
    whole = body(D, voxel, trunc, 0.06)
    for g in range(D.shape[0]):
        assert np.array_equal(whole[g].view(np.int32), body(D[g], voxel, trunc, 0.06).view(np.int32))
