"""Block timeline of the FK backward launch (config 2, 256 rows), chain by chain: when have the prologue loads landed, when
are the (f, m, node) records written, the node fold and the tree sweep done, and when do the global-pose chain and the energy
chain finish?  Needs the -DGQ_BLOCK_TIMES build (tools/block_timeline.sh) through GRASPQP_HIP_LIB.  Eight words per block
(100 MHz ticks): [0] start, [1] end, [2] loads landed, [3] records written, [4] fold done, [5] sweep done, [6] pose chain done,
[7] energy chain done.  The buffer reaches the launcher through gq_debug_fk_backward_times, a symbol of that build only."""
import ctypes, os, sys
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
import torch
from graspqp_amd import _C, ops
from graspqp_amd.hands import get_hand_spec
from graspqp_amd.stepper import GraspStepper
from graspqp_amd.utils import meshes
from bench import make_initial_state

assert "libgraspqp_hip_A" in os.environ.get("GRASPQP_HIP_LIB", ""), "run with the -DGQ_BLOCK_TIMES build (tools/block_timeline.sh)"
B = 256
spec = get_hand_spec("allegro")
fv = meshes.superquadric(0)
sp = meshes.surface_points(fv, 2500, oversample=4, seed=42)
hand = ops.HandHandle(spec)
st = GraspStepper(hand, ops.MeshSet([fv]), torch.tensor(sp)[None], B, 12, seed=1)
# the stage kernels of this build stamp too: their records need the span buffer of block_timeline_stage_b.py, in place before
# the first launch (eight words per block of both stage launches behind the 128 span words)
st._span = torch.zeros(64 + 4 * (B * 13 + 32), 2, dtype=torch.int64, device="cuda")
st._span[:64, 0] = -1
st._pen_desc.span = st._span.data_ptr()
rec_t = torch.zeros(B, 8, dtype=torch.int64, device="cuda")
fn = _C.lib().gq_debug_fk_backward_times
fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p]
assert fn(ctypes.c_void_p(rec_t.data_ptr())) == 0  # before the capture: the pointer is a kernel argument of the graph
hp, idx = make_initial_state(spec, fv, B, 12, 1000)
st.reset(hp.cuda(), idx.cuda())
st.capture(iters=8)
assert st.graph_mode == "one grid"  # the span buffer above is sized for the two stage launches of this mode
torch.cuda.synchronize()
names = ["loads landed", "records written", "fold done", "sweep done", "pose chain done", "energy chain done", "end"]
cols = [2, 3, 4, 5, 6, 7, 1]
acc = []
for _ in range(int(sys.argv[1]) if len(sys.argv) > 1 else 200):  # one sample of every block per replay: its last iteration
    for _ in range(8):
        st.step()
    torch.cuda.synchronize()
    acc.append(rec_t.cpu().numpy().copy())
rec = np.stack(acc).reshape(-1, 8)
fn(ctypes.c_void_p(0))
pc = lambda a: " ".join(f"{np.percentile(a, p):6.2f}" for p in (10, 50, 90))
print(f"FK backward, {B} rows, {len(acc)} launches sampled: block duration (us) p10 p50 p90: {pc((rec[:, 1] - rec[:, 0]) / 100.0)}; "
      f"launch first start -> last end, median {np.median([(r[:, 1].max() - r[:, 0].min()) / 100.0 for r in acc]):.2f} us")
print("   us after the block's start (p10 p50 p90), and the mean")
for name, c in zip(names, cols):
    d = (rec[:, c] - rec[:, 0]) / 100.0
    print(f"   {name:18s} {pc(d)}   mean {d.mean():6.2f}")
