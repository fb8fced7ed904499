// cloudsc2_kern_tl_ens_colsum.hip -- one kernel family of the library as a translation unit of its own (cloudsc2_sweep_kernels.hpp says why):
// tl_ens_colsum_kernel<F>: the column-sum TL sweep with the parameter tangents (C2F_SPARSE | C2F_COLSUM | C2F_PARLIN) for the members of a
// perturbed-parameter ensemble, each over its own argument block in device memory, reached through one accessor.
#include "cloudsc2_sweep_kernels.hpp"

namespace cloudsc2 {
namespace {
C2_VARIANT_TABLE(g_tl_ens_colsum_kernels, tl_ens_colsum_kernel, TlEnsColsumKArgs, 256, sparse_variant_valid(F))
}  // namespace
KernelFn<TlEnsColsumKArgs> tl_ens_colsum_variant(unsigned f) { return f < g_tl_ens_colsum_kernels.size() ? g_tl_ens_colsum_kernels[f] : nullptr; }
}  // namespace cloudsc2
