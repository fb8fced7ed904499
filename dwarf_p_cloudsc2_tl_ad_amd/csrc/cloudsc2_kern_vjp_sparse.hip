// cloudsc2_kern_vjp_sparse.hip -- one kernel family of the library as a translation unit of its own (cloudsc2_sweep_kernels.hpp says why):
// vjp_sparse_kernel<F>: the vector-Jacobian form of the reverse sweep that reads only the cotangent planes and writes only the gradient
// planes of the launch's two masks (C2F_SPARSE), with qsat as a plane or SATUR differentiated in the sweep, reached through one accessor.
#include "cloudsc2_sweep_kernels.hpp"

namespace cloudsc2 {
namespace {
C2_VARIANT_TABLE(g_vjp_sparse_kernels, vjp_sparse_kernel, AdSparseArgs, 256, sparse_variant_valid(F))
}  // namespace
KernelFn<AdSparseArgs> vjp_sparse_variant(unsigned f) { return f < g_vjp_sparse_kernels.size() ? g_vjp_sparse_kernels[f] : nullptr; }
}  // namespace cloudsc2
