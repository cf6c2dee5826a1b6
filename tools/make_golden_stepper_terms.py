#!/usr/bin/env python3
"""Generate tests/golden/stepper_terms_parent_bits.npz: what GraspStepper computes in the three configurations of
tests/_stepper_terms_case.py (A: all ten optional terms, B: clutter with scene, approach, squeeze, reach and arm, C: pre-grasp and
lift on their own grids) -- every term, total and gradient of ``evaluate``, the state after ``reset`` plus three steps with the
fixture's draws and after one ``step_reset`` with a fixed mask, and reach_q, track_q, squeeze_theta and lift_object where they exist.

It was run once, on an MI355X, in a checkout of the PARENT commit of the change that turned the stepper's optional terms into one
table (this file and tests/_stepper_terms_case.py copied into that checkout: they use the stepper's public surface alone);
tests/test_gpu_stepper_terms.py compares the current tree with these bits.  Every case is run twice, and nothing is written unless
the two runs agree bit for bit.  Needs a GPU."""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))  # ref_cpu, which the oracles of tests/ import
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _stepper_terms_case as stc  # noqa: E402


def main():
    out_path = os.environ.get("GRASPQP_GOLDEN_OUT") or os.path.join(ROOT, "tests", "golden", "stepper_terms_parent_bits.npz")
    blob = {}
    for case in stc.CASES:
        first, second = stc.run(case), stc.run(case)
        assert list(first) == list(second)
        for k in first:
            if not np.array_equal(first[k], second[k], equal_nan=True):
                sys.exit(f"{case}.{k}: two runs differ, nothing written")
            assert np.isfinite(first[k]).all(), (case, k)
        print(f"{case}: {len(first)} arrays; total {np.round(first['evaluate.total'], 3).tolist()}; accepted in three steps + reset "
              f"{first['steps.accept'].tolist()} {first['reset.accept'].tolist()}")
        for k in [k for k in first if k.startswith("evaluate.E_")]:
            print(f"   {k} max {float(np.abs(first[k]).max()):.4e}")
        blob.update({f"{case}.{k}": v for k, v in first.items()})
    np.savez_compressed(out_path, **blob)
    print(f"{out_path}: {os.path.getsize(out_path)} bytes, {len(blob)} arrays")


if __name__ == "__main__":
    main()
