// cloudsc2_kern_tl_batch.hip -- one kernel family of the library as a translation unit of its own (cloudsc2_sweep_kernels.hpp says why):
// tl_batch_kernel<F>: CLOUDSC2TL for up to kBatchMax tangents over one trajectory, every valid flag combination and direction count,
// reached through one accessor.
#include "cloudsc2_sweep_kernels.hpp"

namespace cloudsc2 {
namespace {
C2_VARIANT_TABLE(g_tl_batch_kernels, tl_batch_kernel, TlBatchArgs, 64 * (kBatchMax + 1), batch_kernel_valid(F))
}  // namespace
KernelFn<TlBatchArgs> tl_batch_variant(unsigned f, int directions) {
  return f < 64u && directions >= 0 && directions <= kBatchMax ? g_tl_batch_kernels[f + 64u * (unsigned)directions] : nullptr;
}
}  // namespace cloudsc2
