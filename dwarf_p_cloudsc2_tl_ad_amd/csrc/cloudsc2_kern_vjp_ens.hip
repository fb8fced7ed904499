// cloudsc2_kern_vjp_ens.hip -- one kernel family of the library as a translation unit of its own (cloudsc2_sweep_kernels.hpp says why):
// vjp_ens_kernel<F>: the vector-Jacobian form of the reverse sweep with the parameter adjoints (C2F_PARLIN) for the members of a
// perturbed-parameter ensemble, each over its own argument block in device memory, reached through one accessor.
#include "cloudsc2_sweep_kernels.hpp"

namespace cloudsc2 {
namespace {
C2_VARIANT_TABLE(g_vjp_ens_kernels, vjp_ens_kernel, VjpEnsArgs, 512, par_variant_valid(F, C2F_ASSIGN | C2F_VJP))
}  // namespace
KernelFn<VjpEnsArgs> vjp_ens_variant(unsigned f) { return f < g_vjp_ens_kernels.size() ? g_vjp_ens_kernels[f] : nullptr; }
}  // namespace cloudsc2
