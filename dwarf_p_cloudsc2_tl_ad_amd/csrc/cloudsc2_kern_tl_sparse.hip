// cloudsc2_kern_tl_sparse.hip -- one kernel family of the library as a translation unit of its own (cloudsc2_sweep_kernels.hpp says why):
// tl_sparse_kernel<F>: the TL sweep without trajectory stores that reads and writes only the tangent planes of the launch's two masks
// (C2F_SPARSE), with qsat as a plane or SATUR differentiated in the sweep, reached through one accessor.
#include "cloudsc2_sweep_kernels.hpp"

namespace cloudsc2 {
namespace {
C2_VARIANT_TABLE(g_tl_sparse_kernels, tl_sparse_kernel, TlSparseArgs, 256, sparse_variant_valid(F))
}  // namespace
KernelFn<TlSparseArgs> tl_sparse_variant(unsigned f) { return f < g_tl_sparse_kernels.size() ? g_tl_sparse_kernels[f] : nullptr; }
}  // namespace cloudsc2
