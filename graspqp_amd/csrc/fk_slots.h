// Which FK forward kernel answers the contact queries of a mesh set (kin.hip: gq_fk_forward): a pure host rule, in a header
// of its own so that tests/fk_slots_host.cpp can compile it stand-alone.
#pragma once

#define GQ_FK_MAX_SLOTS 3  // box slots per lane of gq_fk_forward_slots_kernel: 64, 128 or 192 clusters per pass

// max_clusters = the largest per-mesh count of 64-face clusters in the set.  Returns KC, the smallest number of box slots
// with 64 * KC >= max_clusters (gq_fk_forward_slots_kernel<KC>), or 0 for gq_fk_forward_kernel (four slots; further passes
// beyond 256 clusters) where a mesh of the set has more than 192 clusters.
static inline int gq_fk_query_slots(long long max_clusters) {
  if (max_clusters > 64ll * GQ_FK_MAX_SLOTS) return 0;
  for (int kc = 1; kc < GQ_FK_MAX_SLOTS; ++kc)
    if (max_clusters <= 64ll * kc) return kc;
  return GQ_FK_MAX_SLOTS;
}
