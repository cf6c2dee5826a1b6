"""CPU-side checks of the exact grasp-quality metrics: C-ABI symbols and argument validation, fake kernels, the class
surface (solver classes, factory unchanged), and that tools/make_golden_exact.py reproduces the committed fixtures."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from graspqp_amd import _C, ops
from graspqp_amd.metrics import (EucledianFrictionConeSpanMetric, EucledianGraspSpanMetric, GraspSpanMetricFactory,
                                 OverallFrictionConeSpanMetric, ScipyLsqSolver, SpanMetricWrapper, SQPLsqSolver)

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def test_exact_symbols_are_declared_and_exported():
    protos = _C.parse_header()
    lib = _C.lib()
    for name in ("gq_lsq_exact_check", "gq_lsq_exact_forward", "gq_span_exact_check", "gq_span_exact_forward"):
        assert name in protos and hasattr(lib, name), name
    assert protos["gq_lsq_exact_check"][1][3] is ctypes.c_double  # bounds cross the ABI in fp64


def test_exact_argument_validation_without_gpu():
    lib = _C.lib()
    assert lib.gq_lsq_exact_check(16, 6, 128, 0.0, 50.0, 100) == 0
    assert lib.gq_lsq_exact_check(16, 6, 129, 0.0, 50.0, 100) != 0 and b"nz" in lib.gq_last_error()
    assert lib.gq_lsq_exact_check(16, 9, 48, 0.0, 50.0, 100) != 0 and b"m = 9" in lib.gq_last_error()
    assert lib.gq_lsq_exact_check(16, 6, 48, 2.0, 1.0, 100) != 0 and b"lower" in lib.gq_last_error()
    assert lib.gq_lsq_exact_check(16, 6, 48, 0.0, float("inf"), 100) != 0 and b"finite" in lib.gq_last_error()
    assert lib.gq_lsq_exact_check(16, 6, 48, float("nan"), 1.0, 100) != 0
    assert lib.gq_span_exact_check(16, 12, 8, 12, 0.0, 50.0, 100) == 0
    assert lib.gq_span_exact_check(16, 17, 8, 12, 0.0, 50.0, 100) != 0 and b"128" in lib.gq_last_error()
    assert lib.gq_span_exact_check(16, 4, 4, 3, 0.0, 50.0, 100) != 0 and b"n_basis" in lib.gq_last_error()


def test_exact_ops_registered_with_fake_kernels():
    from torch._subclasses.fake_tensor import FakeTensorMode

    ns = torch.ops.graspqp_amd
    assert hasattr(ns, "lsq_box_exact") and hasattr(ns, "span_exact")
    with FakeTensorMode():
        x, c, st = ns.lsq_box_exact(torch.empty(5, 6, 48, device="cuda"), torch.empty(5, 6, device="cuda"), 0.0, 50.0, 64)
        assert x.shape == (5, 48) and c.shape == (5,) and st.dtype == torch.int32 and x.dtype == torch.float32
        x, c, st = ns.lsq_box_exact(torch.empty(2, 3, 7, device="cuda", dtype=torch.float64),
                                    torch.empty(2, 3, device="cuda", dtype=torch.float64), 0.0, 1.0, 64)
        assert x.dtype == torch.float64 and c.dtype == torch.float64
        v, xs, svd, st = ns.span_exact(torch.empty(4, 12, 3, device="cuda"), torch.empty(4, 12, 3, device="cuda"),
                                       torch.empty(4, 3, device="cuda"), 8, 0.2, 5.0, 12, 0.0, 50.0, 64)
        assert v.shape == (4, 12) and xs.shape == (4, 12, 12) and svd.shape == (4,) and st.shape == (4, 12)


def test_cpu_tensors_are_refused():
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.lsq_box_exact(torch.zeros(2, 6, 8), torch.zeros(2, 6), 0.0, 1.0)
    with pytest.raises(RuntimeError, match="CUDA"):
        ScipyLsqSolver().solve(torch.zeros(2, 6, 8), torch.zeros(2, 6), min_bound=0.0, max_bound=1.0)


def test_solver_classes_and_metric_surface():
    assert not issubclass(ScipyLsqSolver, SQPLsqSolver)  # the PDIPM routes must not accept it
    s = ScipyLsqSolver.from_mat(torch.zeros(3, 12, 6, 16), torch.zeros(3, 12, 6))
    assert s._num_wrenches == 16 and s._batch_size == 36
    OverallFrictionConeSpanMetric(solver_cls=ScipyLsqSolver)
    m = EucledianFrictionConeSpanMetric.from_dim(12, 6, solver_cls=ScipyLsqSolver, friction=0.3, n_cone_vecs=8,
                                                 solver_kwargs={"n_cone_vecs": 8})
    assert m._mu == 0.3 and m.n_cone_vecs == 8 and m.n_basis_vectors == 12
    # registry.py:120-131 nests n_cone_vecs inside solver_kwargs: warned about and ignored, k stays 4
    w = SpanMetricWrapper(EucledianFrictionConeSpanMetric, {"solver_cls": ScipyLsqSolver, "friction": None, "max_limit": 30.0,
                                                            "solver_kwargs": {"n_cone_vecs": 8}})
    assert w.exact and w._exact.n_cone_vecs == 4 and w._exact._mu == 0.2 and w._exact._max_limit_value == 30.0
    assert EucledianGraspSpanMetric().n_cone_vecs == 1

    class Foreign:
        pass

    for cls in (EucledianFrictionConeSpanMetric, EucledianGraspSpanMetric):
        with pytest.raises(NotImplementedError, match="solver_cls"):
            cls(solver_cls=SQPLsqSolver)
        with pytest.raises(NotImplementedError, match="solver_cls"):
            cls(solver_cls=Foreign)
    with pytest.raises(NotImplementedError, match="solver_cls"):
        OverallFrictionConeSpanMetric(solver_cls=Foreign)
    assert not SpanMetricWrapper(OverallFrictionConeSpanMetric, {"solver_cls": SQPLsqSolver}).exact
    assert SpanMetricWrapper(OverallFrictionConeSpanMetric, {"solver_cls": ScipyLsqSolver}).exact


def test_factory_still_refuses_the_scipy_types():
    GF = GraspSpanMetricFactory
    for t in (GF.MetricType.GRASPQP_SCIPY, GF.MetricType.GRASPQP_EUCLIDIAN_SCIPY):
        with pytest.raises(NotImplementedError):
            GF.create(t)


def test_hand_model_has_the_entropies():
    from graspqp_amd.core.hand_model import HandModel

    assert callable(HandModel.joint_entropy) and callable(HandModel.pose_entropy)


REF = os.environ.get("GRASPQP_REFERENCE", "/root/reference")


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "graspqp")), reason="reference tree not available")
def test_make_golden_exact_reproduces_the_fixtures(tmp_path):
    env = dict(os.environ, GRASPQP_GOLDEN_OUT=str(tmp_path), GRASPQP_REFERENCE=REF)
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_golden_exact.py")], env=env, check=True,
                   capture_output=True, timeout=600)
    for n, k in ((12, 4), (12, 8), (16, 4), (16, 8)):
        name = f"span_euclid_n{n}_k{k}.npz"
        a, b = np.load(os.path.join(ROOT, "tests", "golden", name)), np.load(os.path.join(tmp_path, name))
        assert set(a.files) == set(b.files)
        for key in a.files:
            np.testing.assert_allclose(a[key], b[key], rtol=1e-6, atol=1e-9, err_msg=f"{name}:{key}")
