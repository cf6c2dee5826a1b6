from .ops.dexgrasp import DexgraspSpanMetric
from .ops.registry import GraspSpanMetricFactory, SpanMetricWrapper
from .ops.tdg import TDGSpanMetric
from .ops.span import EucledianFrictionConeSpanMetric, EucledianGraspSpanMetric, OverallFrictionConeSpanMetric
from .solver.qp_solver import QPFunction, SQPLsqSolver
from .solver.scipy_solver import ScipyLsqSolver

GraspQPSpanMetric = SpanMetricWrapper
__all__ = ["GraspSpanMetricFactory", "SpanMetricWrapper", "GraspQPSpanMetric", "SQPLsqSolver", "QPFunction",
           "DexgraspSpanMetric", "TDGSpanMetric", "ScipyLsqSolver", "OverallFrictionConeSpanMetric",
           "EucledianGraspSpanMetric", "EucledianFrictionConeSpanMetric"]
