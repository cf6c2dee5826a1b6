#!/usr/bin/env python3
"""Generate tests/golden/fc_tail_parent_bits.npz: the contacts of eight Allegro grasps after 100 MALA* steps (the eight rows
of tests/test_gpu_fc_tail_slot.py, found as that test finds them, with its mid-way eps) and every output of the fc tail
(gq_fc_tail_kernel<1, 4>) of the library this is run with, at five settings: the default eps, eps = 1e30, the mid-way
eps, eps = 0 (only the not-improved count can stop the rule early), and max_iter = 1.

Run it with the PARENT's library through GRASPQP_HIP_LIB (a build of the commit before the change under test):
tests/test_gpu_fc_tail_candidates.py then compares the current library with these bits.  Needs a GPU."""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import _fc_tail_case as ftc  # noqa: E402
import test_gpu_fc_tail_slot as slot  # noqa: E402
from graspqp_amd import _C, ops  # noqa: E402


def main():
    assert os.environ.get("GRASPQP_HIP_LIB"), "choose the parent's library with GRASPQP_HIP_LIB"
    out_path = os.environ.get("GRASPQP_GOLDEN_OUT") or os.path.join(ROOT, "tests", "golden", "fc_tail_parent_bits.npz")
    _C.lib()
    s = slot._scene(ops, 8)
    blob = {"in.pts": s.pts.numpy().astype(np.float32), "in.nrm": s.nrm.numpy().astype(np.float32),
            "in.cog": s.cog.numpy().astype(np.float32), "in.eps_mid": np.float64(s.eps_mid)}
    cases = {"default": (slot.EPS_DEFAULT, slot.MAX_ITER), "huge": (slot.EPS_HUGE, slot.MAX_ITER),
             "mid": (s.eps_mid, slot.MAX_ITER), "zero": (0.0, slot.MAX_ITER), "one": (slot.EPS_DEFAULT, 1)}
    for tag, (eps, max_iter) in cases.items():
        out = ftc.run(ops, blob["in.pts"], blob["in.nrm"], blob["in.cog"], eps, max_iter)
        for k in ftc.OUTPUTS:
            assert not (out[k] == np.float32(ftc.SENTINEL)).any() and np.isfinite(out[k]).all(), (tag, k)
            blob[f"{tag}.{k}"] = out[k]
        print(f"{tag}: eps {eps:.3g} max_iter {max_iter} n_iter {int(out['n_iter'][0])} e_fc {np.round(out['e_fc'], 4).tolist()}")
    np.savez_compressed(out_path, **blob)
    print(f"{out_path}: {os.path.getsize(out_path)} bytes from {_C.LIB_PATH}")


if __name__ == "__main__":
    main()
