// cloudsc2_kern_tl_par.hip -- one kernel family of the library as a translation unit of its own (cloudsc2_sweep_kernels.hpp says why):
// tl_par_kernel<F>: CLOUDSC2TL with the tangents of the four tunable parameters (C2F_PARLIN), reached through one accessor.
#include "cloudsc2_sweep_kernels.hpp"

namespace cloudsc2 {
namespace {
C2_VARIANT_TABLE(g_tl_par_kernels, tl_par_kernel, TlParArgs, 512, par_variant_valid(F, 0u))
}  // namespace
KernelFn<TlParArgs> tl_par_variant(unsigned f) { return f < g_tl_par_kernels.size() ? g_tl_par_kernels[f] : nullptr; }
}  // namespace cloudsc2
