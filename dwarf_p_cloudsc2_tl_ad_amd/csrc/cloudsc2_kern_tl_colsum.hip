// cloudsc2_kern_tl_colsum.hip -- one kernel family of the library as a translation unit of its own (cloudsc2_sweep_kernels.hpp says why):
// tl_colsum_kernel<F>: the sparse TL sweep that stores no tangent plane but the weighted level sums of the output tangents (C2F_COLSUM),
// with qsat as a plane or SATUR differentiated in the sweep, reached through one accessor.
#include "cloudsc2_sweep_kernels.hpp"

namespace cloudsc2 {
namespace {
C2_VARIANT_TABLE(g_tl_colsum_kernels, tl_colsum_kernel, TlColsumArgs, 256, sparse_variant_valid(F))
}  // namespace
KernelFn<TlColsumArgs> tl_colsum_variant(unsigned f) { return f < g_tl_colsum_kernels.size() ? g_tl_colsum_kernels[f] : nullptr; }
}  // namespace cloudsc2
