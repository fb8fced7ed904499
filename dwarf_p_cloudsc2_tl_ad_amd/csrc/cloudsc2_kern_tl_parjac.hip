// cloudsc2_kern_tl_parjac.hip -- one kernel family of the library as a translation unit of its own (cloudsc2_sweep_kernels.hpp says why):
// tl_parjac_kernel<F>: the sensitivities of CLOUDSC2's outputs to the tunable parameters in one sweep over the trajectory (no tangent
// planes), reached through one accessor.
#include "cloudsc2_sweep_kernels.hpp"

namespace cloudsc2 {
namespace {
C2_VARIANT_TABLE(g_tl_parjac_kernels, tl_parjac_kernel, TlParJacArgs, 64, parjac_variant_valid(F))
}  // namespace
KernelFn<TlParJacArgs> tl_parjac_variant(unsigned f) { return f < g_tl_parjac_kernels.size() ? g_tl_parjac_kernels[f] : nullptr; }
}  // namespace cloudsc2
