// cloudsc2_kern_vjp_batch.hip -- one kernel family of the library as a translation unit of its own (cloudsc2_sweep_kernels.hpp says
// why): vjp_batch_kernel<F>: the reverse sweep of CLOUDSC2AD in its vector-Jacobian form for up to kBatchMax cotangents over one
// trajectory, every valid flag combination and direction count, reached through one accessor.
#include "cloudsc2_sweep_kernels.hpp"

namespace cloudsc2 {
namespace {
C2_VARIANT_TABLE(g_vjp_batch_kernels, vjp_batch_kernel, VjpBatchArgs, 64 * (kBatchMax + 1), batch_kernel_valid(F))
}  // namespace
KernelFn<VjpBatchArgs> vjp_batch_variant(unsigned f, int directions) {
  return f < 64u && directions >= 0 && directions <= kBatchMax ? g_vjp_batch_kernels[f + 64u * (unsigned)directions] : nullptr;
}
}  // namespace cloudsc2
