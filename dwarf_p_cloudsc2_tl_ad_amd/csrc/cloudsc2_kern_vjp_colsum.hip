// cloudsc2_kern_vjp_colsum.hip -- one kernel family of the library as a translation unit of its own (cloudsc2_sweep_kernels.hpp says why):
// vjp_colsum_kernel<F>: the sparse reverse sweep whose cotangent of a level is weight x the cotangent of the column's sum (C2F_COLSUM),
// with qsat as a plane or SATUR differentiated in the sweep, reached through one accessor.
#include "cloudsc2_sweep_kernels.hpp"

namespace cloudsc2 {
namespace {
C2_VARIANT_TABLE(g_vjp_colsum_kernels, vjp_colsum_kernel, AdColsumArgs, 256, sparse_variant_valid(F))
}  // namespace
KernelFn<AdColsumArgs> vjp_colsum_variant(unsigned f) { return f < g_vjp_colsum_kernels.size() ? g_vjp_colsum_kernels[f] : nullptr; }
}  // namespace cloudsc2
