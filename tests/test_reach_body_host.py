"""The device bodies of the reach term (csrc/reach_dev.h: joint transform, product, pose error with the log map, Jacobian column,
the entries of J J', the unrolled 6 x 6 Cholesky solve, the capped and clamped step, the winner of a station, the gradient in the gRt
layout) compiled for the HOST with AddressSanitizer and UBSan.  tests/reach_body_host.cpp walks every lane group of a row through
them serially in the kernel's order, for all five arms of tests/_reach_oracle.py, and the float32 results are held to the fp64
oracle at the bounds of the GPU test on the settled rows: per row |E - E_64| <= 2e-3 E_64 + 1e-10, the pose gradient norm-wise 1e-3
overall and 2e-3 on the translation part and on the rotation part.  The printed errors are the comparison behind the choice of
fp32 for the 6 x 6 solve.  No GPU involved."""
import subprocess

import numpy as np
import pytest

import _host_program
import _reach_oracle as ro


@pytest.fixture(scope="module")
def body(tmp_path_factory):
    d = tmp_path_factory.mktemp("reach_body")
    exe = _host_program.build("reach_body_host", d)

    def run(arm, pose9, base, K, cw, distance=0.10, n_iter=ro.M):
        N, S = arm.n_joints, arm.n_seeds
        f32 = lambda x: np.ascontiguousarray(x, dtype=np.float32).tobytes()
        i32 = lambda x: np.ascontiguousarray(x, dtype=np.int32).tobytes()
        # R as the FK forward forms it: float32 of the Gram-Schmidt map of the float32 rot6d entries
        R = ro.gramschmidt(ro.torch.as_tensor(pose9[None, 3:9], dtype=ro.F64))[0].numpy()
        typ, pre, axs, lo, hi, seeds = ro.padded(arm)
        with open(d / "in.bin", "wb") as f:
            f.write(i32([N, S, K, n_iter]) + f32([distance if K else 0.0, ro.LAM, ro.RHO, cw]) + f32(ro.AXIS) + f32(pose9[:3]) + f32(R))
            f.write(f32(base) + f32(arm.tool_T) + i32(typ) + f32(pre) + f32(axs) + f32(lo) + f32(hi) + f32(seeds))
        subprocess.check_call([exe, str(d / "in.bin"), str(d / "out.bin")])
        o = np.fromfile(d / "out.bin", dtype=np.float32).astype(np.float64)
        assert o.size == 13 + (K + 1) + (K + 1) * S + (K + 1) * N
        a, b = 13 + (K + 1), 13 + (K + 1) + (K + 1) * S
        return o[0], o[1:13], o[13:a].astype(int), o[a:b].reshape(K + 1, S), o[b:].reshape(K + 1, N)

    return run


@pytest.mark.parametrize("n_seeds,stations", [(1, 0), (4, 2)])
@pytest.mark.parametrize("name", ro.ARM_NAMES)
def test_rows_match_the_oracle(body, name, n_seeds, stations):
    cs = ro.case(name, n_seeds, stations)
    arm, ref = cs["arm"], cs["ref"]
    E, grad = np.zeros(8), np.zeros((8, 9))
    for b in range(8):
        E[b], gRt, seed, Eks, q = body(arm, cs["pose9"][b], cs["base_T"][b // 4], stations, cs["up"][b], cs["distance"])
        grad[b] = ro.pose_grad_of_gRt(gRt, cs["pose9"][b])
        assert (q >= arm.lower - 1e-6).all() and (q <= arm.upper + 1e-6).all()
        if cs["settled"][b]:
            two = np.sort(ref["Eks"][b], -1)
            clear = (two[:, 1] > 1.01 * two[:, 0] + 1e-12) if n_seeds > 1 else np.ones(stations + 1, bool)
            assert (seed[clear] == ref["seed"][b][clear]).all(), (b, seed, ref["seed"][b])
    ro.assert_close(E, grad, cs, f"host {name} S={n_seeds} K={stations}")
