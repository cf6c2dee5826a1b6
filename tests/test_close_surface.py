"""The surface of finger closing without a launch: what gq_close_check refuses (host only), the registration with the dispatcher and
its fake kernel, the CPU-tensor refusal, the stepper's term table, export's signature -- and, on the GPU, the class surface and
export_poses with and without ``closed=``."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import _squeeze_cases as sq


def _grids(n_grids=4, shape=(8, 8, 8), voxel=0.01):
    from graspqp_amd import _C

    buf = np.zeros((n_grids,) + shape, np.float32)  # the check is host only: it never reads the values
    g = _C.ClutterGrids()
    g.values, g.n_grids, (g.nx, g.ny, g.nz) = buf.ctypes.data, n_grids, shape
    g.origin, g.voxel = (ctypes.c_float * 3)(0.0, 0.0, 0.0), voxel
    return g, buf


def _check(grids, batch=8, rows=2, J=16, JA=16, L=14, Ns=512, S=32, step=None, touch=5e-4):
    from graspqp_amd import _C

    st = None if step is None else np.ascontiguousarray(step, np.float32)
    _C.call("gq_close_check", ctypes.byref(grids), ctypes.c_int64(batch), ctypes.c_int64(rows), J, JA, L, ctypes.c_int64(Ns), S,
            None if st is None else st.ctypes.data_as(ctypes.c_void_p), float(touch))


def test_close_check_refusals():
    g, keep = _grids()
    good = np.full(16, 0.01, np.float32)
    _check(g, step=good)
    _check(g, step=None, S=1), _check(g, step=good, S=64, touch=0.0)
    bad = [dict(S=0), dict(S=65), dict(S=-3), dict(touch=-1e-6), dict(touch=float("nan")), dict(touch=float("inf")),
           dict(step=np.r_[good[:5], 0.0, good[6:]]), dict(step=np.r_[good[:5], -0.01, good[6:]]),
           dict(step=np.r_[good[:15], np.nan]), dict(step=np.r_[np.inf, good[1:]]),
           dict(batch=8, rows=3), dict(batch=6, rows=2), dict(rows=0),  # a stack that does not cover the batch
           dict(J=65), dict(JA=65), dict(L=65), dict(J=0), dict(Ns=0)]
    for kw in bad:
        with pytest.raises(RuntimeError, match="close"):
            _check(g, **dict(dict(step=good), **kw))
    with pytest.raises(RuntimeError, match="close"):
        from graspqp_amd import _C

        _C.call("gq_close_check", None, ctypes.c_int64(8), ctypes.c_int64(2), 16, 16, 14, ctypes.c_int64(512), 32, None, 5e-4)
    del keep


def test_python_checks_raise_value_errors():
    from graspqp_amd import ops

    spec = sq.spec_of("allegro")
    scene = None  # no device: the grid argument is refused by type before anything else
    with pytest.raises(ValueError, match="SceneSDF"):
        ops.close_check(scene, 8, spec, 512, 32, np.full(16, 0.01, np.float32), 5e-4)
    with pytest.raises(ValueError, match="step"):
        ops._close_step(type("H", (), {"J": 16, "spec": spec})(), [0.01, 0.02])
    assert ops._close_step(type("H", (), {"J": 16, "spec": spec})(), 0.02).tolist() == [np.float32(0.02)] * 16


def test_op_is_registered_with_a_fake_kernel():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from graspqp_amd import ops

    assert hasattr(torch.ops.graspqp_amd, "close_fingers") and hasattr(ops._Eager, "close_fingers")
    stand_in = type("H", (), {"L": 14})()  # what the fake kernel reads of a hand: its links
    hid = ops._register_handle(stand_in)
    Bn, JA, Ns = 6, 16, 96
    with FakeTensorMode():
        e = lambda *s, **kw: torch.empty(*s, device="cuda", **kw)
        out = torch.ops.graspqp_amd.close_fingers(e(Bn, 9 + JA), e(Ns, 3), e(Ns, dtype=torch.int32), hid, e(Bn, 3, 3), e(2, 8, 8, 8),
                                                  [0.0, 0.0, 0.0], 0.01, e(Bn, JA), 32, e(JA), 5e-4, e(JA, dtype=torch.int64))
    shapes = [(Bn, JA), (Bn, 14), (Bn, JA), (Bn, 14), (Bn, 14), (Bn, 14, 3), (Bn, 14, 3)]
    dtypes = [torch.float32, torch.int32, torch.int32, torch.float32, torch.int32, torch.float32, torch.float32]
    assert [tuple(t.shape) for t in out] == shapes and [t.dtype for t in out] == dtypes
    assert all(t.device.type == "cuda" and not t.requires_grad for t in out)
    assert ops.CloseResult._fields == ("theta", "touch_step", "joint_stop", "phi", "sample", "point", "normal", "touched")


def test_cpu_tensors_are_refused():
    from graspqp_amd import ops

    with pytest.raises(RuntimeError, match="CUDA"):
        ops.close_fingers(torch.zeros(2, 25), None, None, torch.zeros(2, 3, 3), None, torch.zeros(2, 16))
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.hold_contacts(torch.zeros(2, 3, 3), torch.zeros(2, 3, 3), torch.zeros(2, 3), ops.hold_loads(0.2), 1, 0.5, 5.0, 4, 4.0)


def test_contacts_pads_with_zero_normals():
    from graspqp_amd import ops

    B, L = 3, 5
    touched = torch.tensor([[0, 1, 0, 1, 1], [0, 0, 0, 0, 0], [1, 0, 0, 0, 0]], dtype=torch.bool)
    point = torch.arange(B * L * 3, dtype=torch.float32).reshape(B, L, 3) + 1
    normal = -point
    ts = torch.where(touched, 2, -1).int()
    res = ops.CloseResult(torch.zeros(B, 2), ts, torch.zeros(B, 2).int(), torch.zeros(B, L), torch.zeros(B, L).int(), point, normal, touched)
    for n in (2, 4, 7):
        cp, nr = res.contacts(n)
        assert cp.shape == nr.shape == (B, n, 3)
        for b in range(B):
            links = torch.nonzero(touched[b]).flatten().tolist()[:n]  # the touched links in link order, at most n
            assert torch.equal(cp[b, :len(links)], point[b, links]) and torch.equal(nr[b, :len(links)], normal[b, links])
            assert (cp[b, len(links):] == 0).all() and (nr[b, len(links):] == 0).all()
    with pytest.raises(ValueError):
        res.contacts(0)


def test_the_stepper_table_and_export_signature_are_as_they_were():
    from graspqp_amd import export, stepper

    assert len(stepper.TERMS) == 9 and not any("close" in t.key for t in stepper.TERMS)
    for fn in (export.export_poses, export.snapshot_dicts):
        par = inspect.signature(fn).parameters
        assert par["closed"].default is None and list(par)[-1] == "selection"
    assert "closed" in inspect.signature(stepper.GraspStepper.hold).parameters


@pytest.fixture(scope="module")
def gq(tmp_path_factory):
    import types

    from graspqp_amd import _C, ops

    assert torch.cuda.is_available()
    sq.set_synthetic_root(tmp_path_factory.mktemp("synthetic_hands"))
    return types.SimpleNamespace(C=_C, ops=ops)


@pytest.mark.gpu
def test_class_surface_and_export(gq, tmp_path):
    from graspqp_amd import export
    from graspqp_amd.core.hand_model import HandModel
    from graspqp_amd.core.object_model import ObjectModel

    Bn, n = 6, 5
    hp, idx = sq.inputs("allegro", Bn, n)
    fv, sp = sq.sphere()
    hm = HandModel(sq.spec_of("allegro"), "cuda")
    om = ObjectModel(batch_size_each=Bn, num_samples=sp.shape[0])
    om.initialize_from_meshes([fv], surface_points_list=[sp])
    hm.set_parameters(hp.cuda(), idx.cuda())
    c = np.asarray(fv, np.float32).reshape(-1, 3).mean(0)
    origin = [float(x) - 0.1575 for x in c]
    grid = gq.ops.SceneSDF.from_meshes([fv], origin, (64, 64, 64), 0.005)
    v = torch.ones(Bn, hm.n_dofs)
    res = hm.close_fingers(grid, v, steps=16)
    _, pts, lnk = hm._surface_handle()
    want = gq.ops.close_fingers(hm.hand_pose.detach(), hm._hand, gq.ops.SurfaceSamples(hm.spec, pts, lnk), hm.global_rotation.detach(), grid,
                                v.cuda(), steps=16)
    for a, b in zip(res, want):
        assert torch.equal(a, b)
    assert not any(t.requires_grad for t in res)
    energy = torch.zeros(Bn, device="cuda")
    plain = export.snapshot_dicts(hm, energy, om, 1, Bn)
    closed = export.snapshot_dicts(hm, energy, om, 1, Bn, closed=res)
    assert set(closed[0]) - set(plain[0]) == {"joint_positions_closed", "n_touched_links"}
    assert all(torch.equal(plain[0][k], closed[0][k]) for k in ("values", "contact_idx"))
    names = list(hm._actuated_joints_names)
    assert list(closed[0]["joint_positions_closed"]) == names
    assert torch.equal(closed[0]["joint_positions_closed"][names[3]], res.theta[:, 3].cpu())
    assert torch.equal(closed[0]["n_touched_links"], res.touched.sum(1).cpu())
    with pytest.raises(ValueError, match="closed"):
        export.snapshot_dicts(hm, energy, om, 1, Bn, closed=gq.ops.CloseResult(*(t[:2] for t in res)))
