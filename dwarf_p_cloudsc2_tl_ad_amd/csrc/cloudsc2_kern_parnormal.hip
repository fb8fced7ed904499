// cloudsc2_kern_parnormal.hip -- a translation unit of its own like the kernel families (cloudsc2_sweep_kernels.hpp says why):
// parnormal_kernel<F>: the Gauss-Newton normal equations of the tunable parameters, J^T W J and J^T W r, summed per column in one sweep
// over the trajectory (no sensitivity plane exists), reached through one accessor.
#include "cloudsc2_sweep_kernels.hpp"

namespace cloudsc2 {
namespace {
C2_VARIANT_TABLE(g_parnormal_kernels, parnormal_kernel, ParNormalArgs, 8, true)
}  // namespace
KernelFn<ParNormalArgs> parnormal_variant(unsigned f) { return f < g_parnormal_kernels.size() ? g_parnormal_kernels[f] : nullptr; }
}  // namespace cloudsc2
