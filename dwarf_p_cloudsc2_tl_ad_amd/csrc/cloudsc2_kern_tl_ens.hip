// cloudsc2_kern_tl_ens.hip -- one kernel family of the library as a translation unit of its own (cloudsc2_sweep_kernels.hpp says why):
// tl_ens_kernel<F>: CLOUDSC2TL with the parameter tangents (C2F_PARLIN) for the members of a perturbed-parameter ensemble, each over
// its own argument block in device memory, reached through one accessor.
#include "cloudsc2_sweep_kernels.hpp"

namespace cloudsc2 {
namespace {
C2_VARIANT_TABLE(g_tl_ens_kernels, tl_ens_kernel, TlEnsArgs, 512, par_variant_valid(F, 0u))
}  // namespace
KernelFn<TlEnsArgs> tl_ens_variant(unsigned f) { return f < g_tl_ens_kernels.size() ? g_tl_ens_kernels[f] : nullptr; }
}  // namespace cloudsc2
