"""The device bodies of the squeeze term (csrc/squeeze_dev.h: Jacobian column, motion of a contact, the entries of the normal
equations, the Cholesky column, the substitution step, the Hessian walk of a joint, the contact-point gradient) compiled for the HOST
with AddressSanitizer and UBSan.  tests/squeeze_body_host.cpp walks one row of gq_squeeze_kernel through them serially in the
kernel's order, and the float32 results are held to the fp64 oracle (ref_cpu.export.get_req_joint_velocities with autograd) at the
bounds of the GPU tests: values rtol 2e-3 / atol 1e-9, theta rtol 2e-3 / atol 2e-5, gradients norm-wise 2e-3 per part.  Every buffer
the program reads is exactly sized, so an index outside one ends the program.  No GPU involved."""
import subprocess

import numpy as np
import pytest
import torch

import _host_program
import _pregrasp_cases as pc
import _squeeze_cases as sq
from ref_cpu import kin


@pytest.fixture(scope="module")
def body(tmp_path_factory):
    d = tmp_path_factory.mktemp("squeeze_body")
    sq.set_synthetic_root(tmp_path_factory.mktemp("synthetic_hands"))
    exe = _host_program.build("squeeze_body_host", d)

    def run(spec, R, tau, lam, c, a, p, start, T, cpos, d2, nrm, closest, pw):
        n, J = len(start), spec.n_nodes
        f32 = lambda x: np.ascontiguousarray(x, dtype=np.float32).tobytes()
        i32 = lambda x: np.ascontiguousarray(x, dtype=np.int32).tobytes()
        with open(d / "in.bin", "wb") as f:
            f.write(i32([n, J]) + f32(np.concatenate([np.ravel(R), [tau, lam, c]])))
            f.write(i32(spec.node_parent) + i32(spec.node_type) + f32(a) + f32(p))
            f.write(i32(start) + f32(T) + f32(cpos) + f32(d2) + f32(nrm) + f32(closest) + f32(pw))
        subprocess.check_call([exe, str(d / "in.bin"), str(d / "out.bin")])
        o = np.fromfile(d / "out.bin", dtype=np.float32).astype(np.float64)
        assert o.size == 1 + 2 * J + 9 + 3 * n
        return o[0], o[1:1 + J], o[1 + J:1 + 2 * J], o[1 + 2 * J:10 + 2 * J].reshape(3, 3), o[10 + 2 * J:].reshape(n, 3)

    return run


CASES = [("allegro", 1), ("allegro", 12), ("shadow_hand", 16), ("chain64", 5), ("star63", 5), ("comb43", 5), ("allegro", 64)]


@pytest.mark.parametrize("name,n", CASES)
def test_row_matches_the_oracle(body, name, n):
    spec = sq.spec_of(name)
    assert not spec.is_coupled  # C / C' are plain products of the kernel; the coupled hands are the GPU tests'
    hp, idx = sq.inputs(name, 2, n)
    up = 1.7
    free = clamped = 0
    parts = {k: [[], []] for k in ("g_theta", "g_R", "g_p")}
    for b in range(2):  # row 0 has its contact 0 at the clamp, row 1 above tau
        hp64 = hp[b:b + 1].double()
        theta = hp64[:, 9:]
        W, T, aw = pc.reduced_frames(spec, theta[0].numpy())
        R = kin.special_gramschmidt(hp64[:, 3:9])
        ix = idx[b].numpy()
        link = np.asarray(spec.cand_link)[ix]
        cpos = np.asarray(spec.cand_pos, np.float64)[ix]
        xh = np.einsum("nab,nb->na", T[link][:, :3, :3], cpos) + T[link][:, :3, 3]
        pw = xh @ R[0].numpy().T + hp64[0, :3].numpy()
        ref = sq.oracle_parts(spec, theta, R, idx[b:b + 1], pw[None], up)
        tag = f"{name} n={n} row {b}"
        near, d2min, fr, cl = sq.guards(ref["dist"], sq.TAU)
        assert near >= sq.KINK and d2min >= sq.MIN_D2, tag
        free, clamped = free + fr, clamped + cl
        E, th, g_theta, g_R, g_p = body(spec, R[0].numpy(), sq.TAU, sq.LAM, up, aw, W[:, :3, 3], np.asarray(spec.link_node)[link],
                                        T[link][:, :3, :], cpos, ref["d2"], ref["normal"], ref["closest"], pw)
        rel = lambda x, y: np.linalg.norm(x - y) / max(np.linalg.norm(y), 1e-300)
        print(f"[{tag}] E {E:.4e} vs {ref['E']:.4e}, theta err {np.abs(th - ref['theta']).max():.2e}, g_theta rel {rel(g_theta, ref['g_theta']):.2e} "
              f"(norm {np.linalg.norm(ref['g_theta']):.2e}), g_R rel {rel(g_R, ref['g_R']):.2e}, g_p rel {rel(g_p, ref['g_p']):.2e} "
              f"(norm {np.linalg.norm(ref['g_p']):.2e})")
        np.testing.assert_allclose(E, ref["E"], rtol=2e-3, atol=1e-9)
        np.testing.assert_allclose(th, ref["theta"], rtol=2e-3, atol=2e-5)
        for k, val in (("g_theta", g_theta), ("g_R", g_R), ("g_p", g_p)):
            parts[k][0].append(np.ravel(val))
            parts[k][1].append(np.ravel(ref[k]))
    assert free > 0 and clamped > 0  # the contact-point path is exercised, and so is the clamp
    for k, (got, want) in parts.items():
        got, want = np.concatenate(got), np.concatenate(want)
        assert np.linalg.norm(want) > 0, k
        assert np.linalg.norm(got - want) <= 2e-3 * np.linalg.norm(want), k


def test_a_clamped_contact_has_no_contact_point_gradient(body):
    spec = sq.spec_of("allegro")
    hp, idx = sq.inputs("allegro", 2, 1)
    hp64 = hp[:1].double()
    W, T, aw = pc.reduced_frames(spec, hp64[0, 9:].numpy())
    R = kin.special_gramschmidt(hp64[:, 3:9])
    ix = idx[0].numpy()
    link = np.asarray(spec.cand_link)[ix]
    cpos = np.asarray(spec.cand_pos, np.float64)[ix]
    pw = (np.einsum("nab,nb->na", T[link][:, :3, :3], cpos) + T[link][:, :3, 3]) @ R[0].numpy().T + hp64[0, :3].numpy()
    ref = sq.oracle_parts(spec, hp64[:, 9:], R, idx[:1], pw[None], 1.0)
    assert float(ref["dist"].abs().max()) < sq.TAU
    E, _, g_theta, g_R, g_p = body(spec, R[0].numpy(), sq.TAU, sq.LAM, 1.0, aw, W[:, :3, 3], np.asarray(spec.link_node)[link],
                                   T[link][:, :3, :], cpos, ref["d2"], ref["normal"], ref["closest"], pw)
    assert E > 0 and (g_p == 0).all() and (ref["g_p"] == 0).all() and np.abs(g_R).max() > 0 and np.abs(g_theta).max() > 0
