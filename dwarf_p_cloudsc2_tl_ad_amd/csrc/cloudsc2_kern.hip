// cloudsc2_kern.hip -- the source of every kernel-family unit: compiled once per name of the Makefile's FAMILIES with
// -DC2_FAMILY=<unit>, it defines the variant tables of that unit's rows (C2_ROWS_<unit> in cloudsc2_sweep_kernels.hpp, which says why the
// families are units of their own) and their accessors, and so holds the code object of exactly those kernels.  A name the table does
// not know does not compile.
#include "cloudsc2_sweep_kernels.hpp"

#ifndef C2_FAMILY
#error "cloudsc2_kern.hip is compiled with -DC2_FAMILY=<unit>, a name of the Makefile's FAMILIES"
#endif
#define C2_ROWS_OF_(unit) C2_ROWS_##unit
#define C2_ROWS_OF(unit) C2_ROWS_OF_(unit)

namespace cloudsc2 {
C2_ROWS_OF(C2_FAMILY)(C2_DEFINE_VARIANT)
}  // namespace cloudsc2
