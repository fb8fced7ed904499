// cloudsc2_kern_nl_ens.hip -- one kernel family of the library as a translation unit of its own (cloudsc2_sweep_kernels.hpp says why):
// nl_ens_kernel<F>: the NL sweep of the differentiable op for the members of a perturbed-parameter ensemble, each over its own argument
// block in device memory, reached through one accessor.
#include "cloudsc2_sweep_kernels.hpp"

namespace cloudsc2 {
namespace {
C2_VARIANT_TABLE(g_nl_ens_kernels, nl_ens_kernel, NlEnsArgs, 64, nl_ens_variant_valid(F))
}  // namespace
KernelFn<NlEnsArgs> nl_ens_variant(unsigned f) { return f < g_nl_ens_kernels.size() ? g_nl_ens_kernels[f] : nullptr; }
}  // namespace cloudsc2
