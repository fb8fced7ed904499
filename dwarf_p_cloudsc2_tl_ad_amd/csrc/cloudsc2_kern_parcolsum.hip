// cloudsc2_kern_parcolsum.hip -- a translation unit of its own like the kernel families (cloudsc2_sweep_kernels.hpp says why):
// parcolsum_kernel<F>: the sensitivities of the column sums of CLOUDSC2's outputs to the tunable parameters, or their Gauss-Newton
// normal equations (C2F_NORMAL), in one sweep over the trajectory (no sensitivity plane exists), reached through one accessor.
#include "cloudsc2_sweep_kernels.hpp"

namespace cloudsc2 {
namespace {
C2_VARIANT_TABLE(g_parcolsum_kernels, parcolsum_kernel, ParColsumArgs, 64, parcolsum_variant_valid(F))
}  // namespace
KernelFn<ParColsumArgs> parcolsum_variant(unsigned f) { return f < g_parcolsum_kernels.size() ? g_parcolsum_kernels[f] : nullptr; }
}  // namespace cloudsc2
