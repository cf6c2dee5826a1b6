#!/usr/bin/env python3
"""Generate tests/golden/fk_backward_parent_bits.npz: seeded inputs of two gq_fk_backward calls (Allegro, 5 rows, 12 and 70
contacts, every gradient input present, fused energy and accept tail) and the outputs of the library it is run with.

Run it with the PARENT's library through GRASPQP_HIP_LIB (a build of the commit before the change under test):
tests/test_gpu_fk_backward_block.py then compares the current library with these bits.  Needs a GPU."""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _fk_backward_case as fkb  # noqa: E402
from graspqp_amd import _C, ops  # noqa: E402
from graspqp_amd.hands import get_hand_spec  # noqa: E402

CASES = {"n12": (5, 12, 31), "n70": (5, 70, 32)}  # tag -> rows, contacts, seed


def main():
    assert os.environ.get("GRASPQP_HIP_LIB"), "choose the parent's library with GRASPQP_HIP_LIB"
    out_path = os.environ.get("GRASPQP_GOLDEN_OUT") or os.path.join(ROOT, "tests", "golden", "fk_backward_parent_bits.npz")
    spec = get_hand_spec("allegro")
    hand = ops.HandHandle(spec)
    blob = {}
    for tag, (B, n, seed) in CASES.items():
        inp = fkb.make_inputs(spec, B, n, seed)
        inp.update(fkb.forward_state(_C, hand, inp))
        out = fkb.run_backward(_C, hand, inp)
        assert np.isfinite(out["grad_pose"]).all() and np.isfinite(out["total"]).all()
        print(f"{tag}: accept {out['accept'].tolist()} total {np.round(out['total'], 3).tolist()} e_joints {np.round(out['e_joints'], 4).tolist()}")
        blob.update({f"{tag}.in.{k}": v for k, v in inp.items()})
        blob.update({f"{tag}.out.{k}": v for k, v in out.items()})
    np.savez_compressed(out_path, **blob)
    print(f"{out_path}: {os.path.getsize(out_path)} bytes from {_C.LIB_PATH}")


if __name__ == "__main__":
    main()
