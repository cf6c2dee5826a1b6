"""Block timeline of stage B (config 2), role by role: fc tail, penetration backward, self penetration.  How long does every
role run beside the others, and inside the tail: when is k* known, when does the row wavefront reach the hand-over, when
is its candidate evaluated?  Inside the penetration backward: when has dis landed, when is the list built, the fold done?
Needs the -DGQ_BLOCK_TIMES build (tools/block_timeline.sh) through GRASPQP_HIP_LIB.  Same record scheme as
block_timeline_stage_a.py: eight words per block behind the 128 span words, the blocks of stage A first."""
import os, sys
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
import torch
from graspqp_amd import ops
from graspqp_amd.hands import get_hand_spec
from graspqp_amd.stepper import GraspStepper
from graspqp_amd.utils import meshes
from bench import make_initial_state

assert "libgraspqp_hip_A" in os.environ.get("GRASPQP_HIP_LIB", ""), "run with the -DGQ_BLOCK_TIMES build (tools/block_timeline.sh)"
spec = get_hand_spec("allegro")
fv = meshes.superquadric(0)
sp = meshes.surface_points(fv, 2500, oversample=4, seed=42)
hand = ops.HandHandle(spec)
st = GraspStepper(hand, ops.MeshSet([fv]), torch.tensor(sp)[None], 256, 12, seed=1)
B = st.B
n_a = B * 5 + B // 4           # stage A: five query blocks per row (two points per thread) + four fc rows per block
n_b = 2 * B + (B + 3) // 4     # stage B: tail, penetration backward, self penetration (four rows per block)
st._span = torch.zeros(64 + 4 * (B * 13 + 32), 2, dtype=torch.int64, device="cuda")  # both launches at either block count
st._span[:64, 0] = -1
st._pen_desc.span = st._span.data_ptr()
hp, idx = make_initial_state(spec, fv, 256, 12, 1000)
st.reset(hp.cuda(), idx.cuda())
st.capture(iters=8)
assert st.graph_mode == "one grid"
torch.cuda.synchronize()
st._span.view(-1)[128:].zero_()  # records of the eager warm-up launches (another grid) must not be read as this one's
import collections
hist = collections.Counter()
for _ in range(int(sys.argv[1]) if len(sys.argv) > 1 else 600):
    st.step()
    hist[int(st.n_iter.item())] += 1
print("n_iter histogram over the replayed iterations:", sorted(hist.items()))
st.flush()
torch.cuda.synchronize()
rec = st._span.view(-1)[128:].view(-1, 8).cpu().numpy()[n_a:n_a + n_b]
roles = {"fc tail": rec[:B], "pen backward": rec[B:2 * B], "self penetration": rec[2 * B:]}
t0 = rec[:, 0].min()
pc = lambda a: " ".join(f"{np.percentile(a, p):6.2f}" for p in (0, 10, 50, 90, 99, 100)) if len(a) else "-"
us = lambda a: (a.astype(np.int64) - t0) / 100.0
print(f"stage B, last captured iteration, {B} rows: first start -> last end {(rec[:, 1].max() - t0) / 100.0:.2f} us")
print("   per role, us after the first block start (min p10 p50 p90 p99 max)")
for name, r in roles.items():
    print(f"   {name:17s} blocks {len(r):4d}  start {pc(us(r[:, 0]))}   end {pc(us(r[:, 1]))}   duration {pc((r[:, 1] - r[:, 0]) / 100.0)}")
    print(f"   {name:17s} role span: first start -> last end {(r[:, 1].max() - r[:, 0].min()) / 100.0:.2f} us")
tail = roles["fc tail"]
if (tail[:, 2] != 0).any():  # the one-trip tail stamps its hand-over: [2] k* known (stop wavefront), [3] row done on the slot
    print(f"   fc tail: k* known after {pc((tail[:, 2] - tail[:, 0]) / 100.0)} us of the block, row wavefront ready to commit "
          f"after {pc((tail[:, 3] - tail[:, 0]) / 100.0)} us")
    print(f"   fc tail: k* known -> block end (apply + commit) {pc((tail[:, 1] - tail[:, 7]) / 100.0)} us")
    # [4] / [5]: launches in which the row had to redo from the table / launches, since the start.  The tail that evaluates
    # both candidates before k* packs the two counts into [4] (low / high word) and stamps "candidate evaluated" in [5]
    redo, n_l = tail[:, 4], int(tail[:, 5].max())
    if (tail[:, 4] >> 32).any():
        redo, n_l = tail[:, 4] & 0xFFFFFFFF, int((tail[:, 4] >> 32).max())
        print(f"   fc tail: candidate evaluated (wavefront 0) after {pc((tail[:, 5] - tail[:, 0]) / 100.0)} us of the block")
    tail = np.concatenate([tail[:, :4], redo[:, None], tail[:, 5:]], 1)
    print(f"   fc tail: {n_l} launches; rows that redo from the table per launch: mean {tail[:, 4].sum() / max(n_l, 1):.2f} of {B}, "
          f"per-row redo rate min / max {tail[:, 4].min() / max(n_l, 1):.3f} / {tail[:, 4].max() / max(n_l, 1):.3f}")
pen = roles["pen backward"]
if (pen[:, 2] != 0).any():  # phases of the penetration backward's first round: [2] dis landed, [3] list built, [4] fold done
    for name, a, b in (("dis landed", 0, 2), ("list built", 2, 3), ("fold done", 3, 4), ("end", 4, 1)):
        print(f"   pen backward: {name:10s} +{pc((pen[:, b] - pen[:, a]) / 100.0)} us   (after the block start {pc((pen[:, b] - pen[:, 0]) / 100.0)})")
