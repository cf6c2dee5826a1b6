"""Which FK forward kernel answers the contact queries of a mesh set (csrc/fk_slots.h: gq_fk_query_slots), as a program of its
own under AddressSanitizer and UBSan (tests/fk_slots_host.cpp): the smallest KC in 1..3 with 64 KC >= the largest per-mesh
cluster count, and the four-slot kernel (0) above 192 clusters.  No GPU."""
import subprocess

import _host_program


def test_slots_follow_the_largest_cluster_count(tmp_path):
    exe = _host_program.build("fk_slots_host", tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    rows = [tuple(int(v) for v in ln.split()) for ln in out.split("\n") if ln]
    assert len(rows) == 401 + 4
    for c, slots in rows:
        assert slots == (0 if c > 192 else max(1, -(-c // 64))), (c, slots)
    got = dict(rows)
    # the edges, spelled out
    assert [got[c] for c in (0, 1, 64, 65, 128, 129, 141, 192, 193, 256, 257, 2 ** 31)] == [1, 1, 1, 2, 2, 3, 3, 3, 0, 0, 0, 0]
