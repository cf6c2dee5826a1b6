"""The device bodies of the approach tracking term (csrc/track_dev.h: the distance of a waypoint, the station a waypoint stands for,
the running sums of a row; on top of csrc/reach_dev.h: the reach term's update) compiled for the HOST with AddressSanitizer and
UBSan.  tests/track_body_host.cpp walks the lane groups serially in the kernel's order, for all five arms of tests/_reach_oracle.py,
and the float32 results are held to the fp64 oracle of tests/_track_oracle.py at the bounds of the GPU test on the stable rows:
per row |E - E_64| <= 2e-3 E_64 + 1e-10, the pose gradient norm-wise 1e-3 overall and 2e-3 on the translation part and on the
rotation part, track_q within 1e-3, track_step within 2e-3.  No GPU involved."""
import subprocess

import numpy as np
import pytest

import _host_program
import _reach_oracle as ro
import _track_oracle as to


@pytest.fixture(scope="module")
def body(tmp_path_factory):
    d = tmp_path_factory.mktemp("track_body")
    exe = _host_program.build("track_body_host", d)

    def run(cs, K):
        arm, T, U = cs["arm"], cs["T"], cs["U"]
        B, N = len(cs["pose9"]), arm.n_joints
        f32 = lambda x: np.ascontiguousarray(x, dtype=np.float32).tobytes()
        i32 = lambda x: np.ascontiguousarray(x, dtype=np.int32).tobytes()
        typ, pre, axs, lo, hi, _ = ro.padded(arm)
        with open(d / "in.bin", "wb") as f:
            f.write(i32([B, N, T, U, K]) + f32([cs["distance"], ro.LAM, ro.RHO]) + f32(cs["axis"]))
            f.write(i32(typ) + f32(pre) + f32(axs) + f32(lo) + f32(hi) + f32(arm.tool_T))
            for b in range(B):
                # R as the FK forward forms it: float32 of the Gram-Schmidt map of the float32 rot6d entries
                R = ro.gramschmidt(ro.torch.as_tensor(cs["pose9"][b][None, 3:9], dtype=ro.F64))[0].numpy()
                f.write(f32([cs["up"][b]]) + f32(cs["pose9"][b][:3]) + f32(R) + f32(cs["base_T"][b // cs["batch_each"]]) + f32(cs["q_start"][b]))
        subprocess.check_call([exe, str(d / "in.bin"), str(d / "out.bin")])
        per = 15 + (T + 1) * N + ((K + 1) * N if K else 0)
        o = np.fromfile(d / "out.bin", dtype=np.float32).reshape(B, per)
        q = o[:, 15:15 + (T + 1) * N].reshape(B, T + 1, N)
        sq = o[:, 15 + (T + 1) * N:].reshape(B, K + 1, N) if K else None
        return o[:, 0], o[:, 1], o[:, 2], o[:, 3:15], q, sq

    return run


@pytest.mark.parametrize("n_seeds,T,U,K", [(1, 8, 3, 2), (4, 4, 2, 1)])
@pytest.mark.parametrize("name", ro.ARM_NAMES)
def test_rows_match_the_oracle(body, name, n_seeds, T, U, K):
    cs = to.case(name, n_seeds, T, U)
    arm, ref = cs["arm"], cs["ref"]
    E, worst, step, gRt, q, sq = body(cs, K)
    grad = np.stack([ro.pose_grad_of_gRt(gRt[b].astype(np.float64), cs["pose9"][b]) for b in range(len(E))])
    assert (q >= arm.lower.astype(np.float32)).all() and (q <= arm.upper.astype(np.float32)).all()
    to.assert_close(E, grad, q, step, cs, f"host {name} S={n_seeds} T={T} U={U}")
    m = cs["stable"]
    assert (np.abs(worst.astype(np.float64) - ref["worst"])[m] <= to.e_bound(ref["worst"])[m]).all()
    for k in range(K + 1):  # the station copies are the waypoints' bits
        assert np.array_equal(sq[:, k], q[:, T * (K - k) // K])
