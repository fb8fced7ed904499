// cloudsc2_kern_nl_ens_colsum.hip -- one kernel family of the library as a translation unit of its own (cloudsc2_sweep_kernels.hpp says why):
// nl_ens_colsum_kernel<F>: the column-sum NL sweep (C2F_COLSUM) for the members of a perturbed-parameter ensemble, each over its own
// argument block in device memory, with or without the planes the reverse sweep re-reads (C2F_CKPT), reached through one accessor.
#include "cloudsc2_sweep_kernels.hpp"

namespace cloudsc2 {
namespace {
C2_VARIANT_TABLE(g_nl_ens_colsum_kernels, nl_ens_colsum_kernel, NlEnsColsumArgs, 64, nl_colsum_variant_valid(F))
}  // namespace
KernelFn<NlEnsColsumArgs> nl_ens_colsum_variant(unsigned f) { return f < g_nl_ens_colsum_kernels.size() ? g_nl_ens_colsum_kernels[f] : nullptr; }
}  // namespace cloudsc2
