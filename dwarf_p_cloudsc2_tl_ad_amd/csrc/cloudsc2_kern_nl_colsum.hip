// cloudsc2_kern_nl_colsum.hip -- one kernel family of the library as a translation unit of its own (cloudsc2_sweep_kernels.hpp says why):
// nl_colsum_kernel<F>: the NL sweep that stores no output plane but the per-column weighted level sums of its outputs (C2F_COLSUM), with qsat
// as a plane or SATUR evaluated in the sweep, with or without the planes the reverse sweep re-reads (C2F_CKPT), reached through one accessor.
#include "cloudsc2_sweep_kernels.hpp"

namespace cloudsc2 {
namespace {
C2_VARIANT_TABLE(g_nl_colsum_kernels, nl_colsum_kernel, NlColsumArgs, 64, nl_colsum_variant_valid(F))
}  // namespace
KernelFn<NlColsumArgs> nl_colsum_variant(unsigned f) { return f < g_nl_colsum_kernels.size() ? g_nl_colsum_kernels[f] : nullptr; }
}  // namespace cloudsc2
