// The stream kernel's slice plan (csrc/lsmck_splan.h) as a plain C++ shared
// object for the tests (tests/splan_model.py builds and loads it): the same
// functions the cut pass runs on the device and the launcher on the host.
#include "lsmck_splan.h"

extern "C" {
double splan_fraction(uint32_t s, uint32_t S, uint32_t W) { return lsmck::splan::fraction(s, S, W); }
uint32_t splan_slices(int ncu, uint64_t n) { return lsmck::splan::slices(ncu, n); }
uint32_t splan_slices_max(int ncu) { return lsmck::splan::slices_max(ncu); }
uint32_t splan_waves(int ncu) { return lsmck::splan::waves(ncu); }
}
