// pair_kernels_inst.hip — one translation unit per compiled SH order.
// Built once per order with -DSHP_L=<L> (L = -1: run-time order, loop kernel);
// exports shp_launch_L<L>() and shp_instance_L<L>() to the dispatch tables in shpair_api.hip.
#include "pair_kernel.hpp"

#ifndef SHP_L
#error "compile with -DSHP_L=<order>"
#endif

#define SHP_CAT2(a, b) a##b
#define SHP_CAT(a, b) SHP_CAT2(a, b)
#if SHP_L < 0
#define SHP_FN shp_launch_Lrt
#define SHP_IFN shp_instance_Lrt
#else
#define SHP_FN SHP_CAT(shp_launch_L, SHP_L)
#define SHP_IFN SHP_CAT(shp_instance_L, SHP_L)
#endif

namespace shp {
void SHP_FN(const PairParams& P, const ContactPlan& pl, bool needv, hipStream_t st, hipEvent_t w) { launch_pair_contact<SHP_L>(P, pl, needv, st, w); }
const void* SHP_IFN(const ContactPlan& plan, bool needv) { return pair_contact_instance<SHP_L>(plan, needv); }
}  // namespace shp
