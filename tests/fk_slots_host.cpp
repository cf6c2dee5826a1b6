// The dispatch rule of the contact queries in the FK forward launch (graspqp_amd/csrc/fk_slots.h) compiled for the HOST:
// tests/test_fk_slots_host.py builds this program with the host compiler and sanitizers and runs it.  No GPU involved.
// usage: fk_slots_host            -> one line "max_clusters slots" for every count 0 .. 400 and for a few huge ones
#include <cstdio>

#include "../graspqp_amd/csrc/fk_slots.h"

int main() {
  const long long huge[] = {1ll << 20, (1ll << 31) - 1, 1ll << 31, 1ll << 40};
  for (long long c = 0; c <= 400; ++c) printf("%lld %d\n", c, gq_fk_query_slots(c));
  for (long long c : huge) printf("%lld %d\n", c, gq_fk_query_slots(c));
  return 0;
}
