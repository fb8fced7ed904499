// cloudsc2_kern_vjp_par.hip -- one kernel family of the library as a translation unit of its own (cloudsc2_sweep_kernels.hpp says why):
// vjp_par_kernel<F>: the vector-Jacobian form of the reverse sweep with the adjoints of the four tunable parameters (C2F_PARLIN),
// reached through one accessor.
#include "cloudsc2_sweep_kernels.hpp"

namespace cloudsc2 {
namespace {
C2_VARIANT_TABLE(g_vjp_par_kernels, vjp_par_kernel, AdParArgs, 512, par_variant_valid(F, C2F_ASSIGN | C2F_VJP))
}  // namespace
KernelFn<AdParArgs> vjp_par_variant(unsigned f) { return f < g_vjp_par_kernels.size() ? g_vjp_par_kernels[f] : nullptr; }
}  // namespace cloudsc2
