"""The decision bodies of finger closing (csrc/close_dev.h: direction normalisation, the (phi, index) key, the stop mask, the clamped
update) compiled for the HOST with AddressSanitizer and UBSan and run as a program (tests/close_body_host.cpp) on records dumped
from the cases of tests/_close_cases.py, against the fp64 oracle (tests/_close_oracle.py).

What is exact: which rows move at all and the fastest joint's increment (+-step, bit for bit), the per-link minimum and its sample
(ties to the lowest index; the fold gives the same keys in either order), the stop flags, and the clamped update against the same
float32 operations done by numpy.  What is rounded: Delta = step (u / m) is three correctly rounded float32 operations on the
oracle's exact operands, so it is held to 4 float32 ulps of the fp64 value; the updated joint to that plus one rounding of the sum.
Nothing is loaded into Python under a sanitizer.  No GPU involved."""
import subprocess

import numpy as np
import pytest
import torch

import _close_cases as cc
import _close_oracle as co
import _host_program
from graspqp_amd import ops
from graspqp_amd.hands import get_hand_spec
from ref_cpu import kin

EPS = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def body(tmp_path_factory):
    d = tmp_path_factory.mktemp("close_body")
    exe = _host_program.build("close_body_host", d)

    def run(JA, L, step, lo, hi, masks, lnk, records):
        f32 = lambda v: np.ascontiguousarray(v, dtype=np.float32).tobytes()
        with open(d / "in.bin", "wb") as f:
            f.write(np.array([JA, L, len(lnk), len(records)], np.int32).tobytes() + f32(step) + f32(lo) + f32(hi))
            f.write(np.ascontiguousarray(masks, np.uint64).tobytes() + np.ascontiguousarray(lnk, np.int32).tobytes())
            for v, th, touched, phi in records:
                f.write(f32(v) + f32(th) + np.array([touched], np.uint64).tobytes() + f32(phi))
        subprocess.check_call([exe, str(d / "in.bin"), str(d / "out.bin")])
        raw = np.fromfile(d / "out.bin", dtype=np.uint8)
        rec = 4 * (JA + 1 + L + L + JA + JA)
        assert raw.size == rec * len(records)
        out = []
        for r in range(len(records)):
            w = raw[r * rec:(r + 1) * rec]
            f = lambda a, n, dt=np.float32: (w[4 * a:4 * (a + n)].view(dt), a + n)
            delta, a = f(0, JA)
            m, a = f(a, 1)
            ml, a = f(a, L)
            idx, a = f(a, L, np.int32)
            stopped, a = f(a, JA, np.int32)
            tnew, a = f(a, JA)
            out.append((delta, float(m[0]), ml, idx, stopped, tnew))
        return out

    return run


@pytest.mark.parametrize("name,Ns,S", [("allegro", 512, 32), ("ability_hand", 96, 8), ("panda", 512, 8)])
def test_bodies_match_the_fp64_oracle(body, name, Ns, S):
    spec = get_hand_spec(name)
    JA, L = spec.n_dofs, spec.n_links
    pts, lnk = cc.samples(name, Ns)
    hp, dirs, step = cc.inputs(name, Ns, S)
    ref = cc.reference(name, Ns, S)
    lo, hi = np.asarray(spec.joints_lower, np.float32), np.asarray(spec.joints_upper, np.float32)
    masks = ops.close_stop_masks_host(spec)
    # the per-sample phi of every row at its final state, by the oracle's own pieces; a second set quantised to 1 mm: ties
    oh = co.so.hand_oracle(spec, pts, lnk)
    x, _ = co.sample_world(oh, torch.as_tensor(ref["theta"]), kin.special_gramschmidt(hp[:, 3:9].double()), hp[:, :3].double())
    ph = co.stack_phi(cc.fields(), x).numpy().astype(np.float32)
    with np.errstate(invalid="ignore"):
        coarse = np.where(np.isfinite(ph), np.round(ph * 1e3) / 1e3, np.inf).astype(np.float32)
    gen = np.random.default_rng(7)
    records, meta = [], []
    for b in range(cc.B):
        for s, phi in ((0, ph[b]), (min(S, 2), coarse[b]), (S, ph[b])):
            touched = sum(1 << l for l in range(L) if 0 <= ref["touch_step"][b, l] <= s)
            records.append((dirs[b].numpy(), ref["thetas"][s, b].astype(np.float32), touched, phi))
            meta.append((b, s))
    for bad in (np.nan, np.inf):  # a command with a non-finite entry: the row does not move
        v = dirs[0].numpy().copy()
        v[gen.integers(JA)] = bad
        records.append((v, ref["thetas"][0, 0].astype(np.float32), 0, ph[0]))
        meta.append((0, 0))
    out = body(JA, L, step, lo, hi, masks, lnk, records)
    n_ties = 0
    for (v, th, touched, phi), (b, s), (delta, m, ml, idx, stopped, tnew) in zip(records, meta, out):
        st64, v64 = step.astype(np.float64), np.asarray(v, np.float64)
        d64 = co.direction_delta(torch.as_tensor(v64)[None], torch.as_tensor(st64))[0].numpy()
        u64 = v64 / st64
        if not np.isfinite(u64).all() or np.abs(u64).max() == 0:
            assert (delta == 0).all() and (d64 == 0).all()
        else:
            assert m == np.float32(np.abs((np.asarray(v, np.float32) / step)).max())
            fast = int(np.argmax(np.abs(u64)))
            assert abs(float(delta[fast])) == float(step[fast])  # exactly its step
            assert (np.abs(delta - d64) <= 4 * EPS * np.abs(d64)).all(), (b, s)
            assert ((delta == 0) == (d64 == 0)).all()
        m64, i64, _ = co.link_minima(torch.as_tensor(phi.astype(np.float64))[None], lnk, L)
        assert np.array_equal(ml.astype(np.float64), m64[0].numpy()) and np.array_equal(idx, i64[0]), (b, s)
        n_ties += sum(int((phi[lnk == l] == ml[l]).sum() > 1) for l in range(L) if np.isfinite(ml[l]))
        want_stop = np.array([bool(int(masks[a]) & touched) for a in range(JA)])
        assert np.array_equal(stopped != 0, want_stop), (b, s)
        if np.isfinite(v).all() and s < S:  # the oracle's own stop flags and update of this step
            assert np.array_equal(want_stop, (ref["joint_stop"][b] >= 0) & (ref["joint_stop"][b] <= s)), (b, s)
        with np.errstate(invalid="ignore"):
            emu = np.where(want_stop | (delta == 0), th, np.minimum(np.maximum(th + delta, lo), hi)).astype(np.float32)
        assert np.array_equal(tnew, emu), (b, s)
        o64 = np.where(want_stop | (d64 == 0), th.astype(np.float64), np.minimum(np.maximum(th.astype(np.float64) + d64, lo), hi))
        assert (np.abs(tnew - o64) <= EPS * np.maximum(np.abs(o64), 1e-3) + 4 * EPS * np.abs(d64)).all(), (b, s)
        assert (tnew[want_stop] == th[want_stop]).all()
    assert n_ties > 0, "no record has a tie: the quantised set is there to make some"
