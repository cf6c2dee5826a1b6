"""The per-lane device bodies of the payload-holding term (csrc/hold_dev.h: inward normal, load scaling, p = F'w, the evaluation of an
iterate, the force and dE/dp shares of a column, the torque share of a (contact, joint) pair and the fold with the coupling matrix)
compiled for the HOST with AddressSanitizer and UBSan.  tests/hold_body_host.cpp walks one row of gq_hold_kernel through them serially
in the kernel's order, with the iterates x of the fp64 loop (tests/_hold_cases.py) rounded to float32, and the float32 results are held
to the fp64 reference on the same x.  The wave-level loop itself is the GPU tests' subject.

Bounds: everything here is a few dozen float32 operations on operands of the size of the load |w| (2 .. 60 N) and of x (<= 4 N), so
an error of 100 float32 roundings (6e-6 relative to that size) is the allowance: E, resid and V / |w|^2 2e-5 absolute (they are
ratios to |w|), p, force and torque 2e-5 of the row's largest |w| (torque: times the 0.3 m a hand spans), the gradient 2e-5 absolute
plus 1e-4 of its norm.  Every buffer the program reads is exactly sized, so an index outside one ends the program.  No GPU involved."""
import subprocess

import numpy as np
import pytest
import torch

import _host_program
import _hold_cases as hc
import _pregrasp_cases as pc
from ref_cpu import kin


@pytest.fixture(scope="module")
def body(tmp_path_factory):
    d = tmp_path_factory.mktemp("hold_body")
    exe = _host_program.build("hold_body_host", d)

    def run(spec, n, k, L, R, c_up, nrm, cols, loads, x, a, p, start, xh):
        J, JA = spec.n_nodes, spec.n_dofs
        f32 = lambda v: np.ascontiguousarray(v, dtype=np.float32).tobytes()
        i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32).tobytes()
        with open(d / "in.bin", "wb") as f:
            f.write(i32([n, k, L, J, JA, int(spec.is_coupled)]) + f32(np.concatenate([np.ravel(R), [hc.TW, hc.RIDGE, c_up]])))
            f.write(f32(nrm) + f32(cols) + f32(loads) + f32(x) + i32(spec.node_parent) + i32(spec.node_type) + f32(a) + f32(p))
            f.write(i32(start) + f32(xh) + (f32(spec.coupling) if spec.is_coupled else b""))
        subprocess.check_call([exe, str(d / "in.bin"), str(d / "out.bin")])
        o = np.fromfile(d / "out.bin", dtype=np.float32).astype(np.float64)
        nz = n * k
        sizes = [n * 3, L * nz, 1, L, L, L * n * 3, L * JA, n * 3]
        assert o.size == sum(sizes)
        parts = np.split(o, np.cumsum(sizes)[:-1])
        return (parts[0].reshape(n, 3), parts[1].reshape(L, nz), float(parts[2][0]), parts[3], parts[4], parts[5].reshape(L, n, 3),
                parts[6].reshape(L, JA), parts[7].reshape(n, 3))

    return run


@pytest.mark.parametrize("name", hc.HANDS)
@pytest.mark.parametrize("n,k", hc.NK)
def test_row_matches_fp64(body, name, n, k):
    L = 3
    spec = hc.spec_of(name)
    hp, idx, cp, nrm, cog = hc.inputs(name, n)
    ref = hc.reference(name, n, k, L)
    hc.assert_populated(ref, n, f"{name} n={n} k={k}")
    lw = hc.loads(L).double().numpy()
    c_up = 1.7
    for b in range(hc.B):  # every regime: two rows of each object
        hp64 = hp[b:b + 1].double()
        W, T, aw = pc.reduced_frames(spec, hp64[0, 9:].numpy())
        R = kin.special_gramschmidt(hp64[:, 3:9])[0].numpy()
        ix = idx[b].numpy()
        link = np.asarray(spec.cand_link)[ix]
        cpos = np.asarray(spec.cand_pos, np.float64)[ix]
        xh = np.einsum("nab,nb->na", T[link][:, :3, :3], cpos) + T[link][:, :3, 3]
        F = ref["F"][b]  # (6,nz) fp64
        w = lw[b // hc.BE]
        nin, p, E, resid, V, force, torque, g = body(spec, n, k, L, R, c_up, nrm[b].numpy(), F.T, w, ref["x"][b], aw, W[:, :3, 3],
                                                     np.asarray(spec.link_node)[link], xh)
        ws = np.concatenate([w[:, :3], hc.TW * w[:, 3:]], 1)
        wmax = np.linalg.norm(ws, axis=1).max()
        tag = f"{name} n={n} k={k} row {b}"
        print(f"[{tag}] E {E:.5f} vs {ref['E'][b]:.5f}, resid err {np.abs(resid - ref['resid'][b]).max():.1e}, p err "
              f"{np.abs(p - ws @ F).max():.1e}, force err {np.abs(force - ref['force'][b]).max():.1e} N, torque err "
              f"{np.abs(torque - ref['torque'][b]).max():.1e} N m, g err {np.linalg.norm(g - c_up * ref['g'][b]):.1e} of "
              f"{np.linalg.norm(c_up * ref['g'][b]):.1e}")
        assert np.array_equal(nin, -nrm[b].double().numpy()), tag
        assert np.abs(p - ws @ F).max() <= 2e-5 * wmax, tag
        assert abs(E - ref["E"][b]) <= 2e-5 and np.abs(resid - ref["resid"][b]).max() <= 2e-5, tag
        Vref = np.array([hc.evaluate(torch.as_tensor(F), torch.as_tensor(ws[l]), torch.as_tensor(ref["x"][b, l]))[1] for l in range(L)])
        assert np.abs(V - Vref).max() <= 2e-5 * wmax ** 2, tag
        assert np.abs(force - ref["force"][b]).max() <= 2e-5 * wmax, tag
        assert np.abs(torque - ref["torque"][b]).max() <= 2e-5 * wmax * 0.3, tag
        gr = c_up * ref["g"][b]
        assert np.linalg.norm(g - gr) <= 2e-5 + 1e-4 * np.linalg.norm(gr), tag
