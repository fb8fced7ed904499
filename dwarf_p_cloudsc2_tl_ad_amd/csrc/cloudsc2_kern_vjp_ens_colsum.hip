// cloudsc2_kern_vjp_ens_colsum.hip -- one kernel family of the library as a translation unit of its own (cloudsc2_sweep_kernels.hpp says why):
// vjp_ens_colsum_kernel<F>: the column-sum reverse sweep with the parameter adjoints (C2F_SPARSE | C2F_COLSUM | C2F_PARLIN) for the members
// of a perturbed-parameter ensemble, each over its own argument block in device memory, reached through one accessor.
#include "cloudsc2_sweep_kernels.hpp"

namespace cloudsc2 {
namespace {
C2_VARIANT_TABLE(g_vjp_ens_colsum_kernels, vjp_ens_colsum_kernel, VjpEnsColsumKArgs, 256, sparse_variant_valid(F))
// (fp32 only: the pass that stores the field gradients in the column-sum twin's bits, cloudsc2_sweep_kernels.hpp says why)
C2_VARIANT_TABLE(g_vjp_ens_colsum_fields_kernels, vjp_ens_colsum_fields_kernel, VjpEnsColsumKArgs, 256, kEnsColsumFieldsPass && sparse_variant_valid(F))
}  // namespace
KernelFn<VjpEnsColsumKArgs> vjp_ens_colsum_variant(unsigned f) { return f < g_vjp_ens_colsum_kernels.size() ? g_vjp_ens_colsum_kernels[f] : nullptr; }
KernelFn<VjpEnsColsumKArgs> vjp_ens_colsum_fields_variant(unsigned f) {
  return f < g_vjp_ens_colsum_fields_kernels.size() ? g_vjp_ens_colsum_fields_kernels[f] : nullptr;
}
}  // namespace cloudsc2
