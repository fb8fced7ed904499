// cloudsc2_kern_ad.hip -- one kernel family of the library as a translation unit of its own (cloudsc2_sweep_kernels.hpp says why):
// ad_kernel<F> (both sweeps of CLOUDSC2AD) and ad_reverse_kernel<F> (the reverse sweep alone, also as the vector-Jacobian product,
// C2F_VJP), every valid flag combination, reached through one accessor.
#include "cloudsc2_sweep_kernels.hpp"

namespace cloudsc2 {
namespace {
// (C2F_SATLIN: the vector-Jacobian form with SATUR differentiated in the sweep -- ASSIGN | VJP, without QSAT: PRECISE x EVAP x OFF32)
C2_VARIANT_TABLE(g_ad_reverse_kernels, ad_reverse_kernel, AdArgs, 256,
                 (F & C2F_SATLIN) ? (F & ~(C2F_PRECISE | C2F_EVAP | C2F_OFF32)) == (C2F_SATLIN | C2F_ASSIGN | C2F_VJP)
                                  : (!(F & C2F_ADNORM) || ((F & C2F_ASSIGN) && !(F & C2F_EVAP))) && (!(F & C2F_VJP) || ((F & C2F_ASSIGN) && !(F & C2F_ADNORM))))
C2_VARIANT_TABLE(g_ad_kernels, ad_kernel, AdArgs, 64, !(F & C2F_ADNORM))
}  // namespace
KernelFn<AdArgs> ad_reverse_variant(unsigned f) { return f < g_ad_reverse_kernels.size() ? g_ad_reverse_kernels[f] : nullptr; }
KernelFn<AdArgs> ad_variant(unsigned f) { return f < g_ad_kernels.size() ? g_ad_kernels[f] : nullptr; }
}  // namespace cloudsc2
