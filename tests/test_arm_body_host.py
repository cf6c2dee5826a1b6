"""The device bodies of the arm clearance term (csrc/armscene_dev.h: the chain of link frames, the sphere point, the hinge on the grid,
the sphere's share of dE/dq, the frozen column, J g_q and J J' in fp64, the unrolled fp64 Cholesky; with the reach term's joint bodies
and gq_scene_sample) compiled for the HOST with AddressSanitizer and UBSan.  tests/armscene_body_host.cpp walks the stations of a row
through them serially in the kernel's order, for all five arms of tests/_reach_oracle.py with K in {0, 2}, and the float32 results
are held to the fp64 oracle at the bounds of the GPU test: per row |E - E_64| <= 1e-5 m, the pose gradient norm-wise within
1e-3 |g_64| on the rows whose gradient is not zero.  No GPU involved."""
import subprocess

import numpy as np
import pytest

import _arm_oracle as ao
import _host_program
import _reach_oracle as ro


@pytest.fixture(scope="module")
def body(tmp_path_factory):
    d = tmp_path_factory.mktemp("arm_body")
    exe = _host_program.build("armscene_body_host", d)

    def run(arm, fld, pose9, base, q, K, cw, distance, lam=ao.LAM_A):
        f32 = lambda x: np.ascontiguousarray(x, dtype=np.float32).tobytes()
        i32 = lambda x: np.ascontiguousarray(x, dtype=np.int32).tobytes()
        R = ro.gramschmidt(ro.torch.as_tensor(pose9[None, 3:9], dtype=ro.F64))[0].numpy()
        typ, pre, axs, lo, hi, _ = ro.padded(arm)
        with open(d / "in.bin", "wb") as f:
            f.write(i32([arm.n_joints, K, arm.n_spheres, *fld.shape]))
            f.write(f32([distance if K else 0.0, lam, ro.RHO, cw, ao.MARGIN, fld.voxel]) + f32(fld.origin) + f32(ro.AXIS) + f32(R))
            f.write(f32(base) + f32(arm.tool_T) + i32(typ) + f32(pre) + f32(axs) + f32(lo) + f32(hi) + f32(q))
            f.write(i32(arm.sphere_link) + f32(arm.sphere_centre) + f32(arm.sphere_radius) + f32(fld.values.numpy()))
        subprocess.check_call([exe, str(d / "in.bin"), str(d / "out.bin")])
        o = np.fromfile(d / "out.bin", dtype=np.float32).astype(np.float64)
        assert o.size == 13 + K + 1
        return o[0], o[1:13], o[13:]

    return run


@pytest.mark.parametrize("stations,kind", [(0, "affine"), (2, "affine"), (2, "random")])
@pytest.mark.parametrize("name", ro.ARM_NAMES)
def test_rows_match_the_oracle(body, name, stations, kind):
    cs = ao.case(name, stations, kind)
    arm = cs["arm"]
    if kind == "affine":
        ao.assert_coverage(cs["res"], arm, f"host {name} K={stations}")
    E, grad = np.zeros(8), np.zeros((8, 9))
    for b in range(8):
        E[b], gRt, Ek = body(arm, cs["field"], cs["pose9"][b], cs["base_T"][b // 4], cs["q"][b], stations, cs["up"][b], cs["distance"])
        grad[b] = ro.pose_grad_of_gRt(gRt, cs["pose9"][b])
        assert np.abs(Ek - cs["res"]["Ek"][b]).max() <= 1e-5
    ao.assert_close(E, grad, cs, f"host {name} K={stations} {kind}")
