// cloudsc2_fields.hpp -- the one table of the 16 input and 10 output fields of the C ABI (include/cloudsc2_hip.h) and what the launchers
// derive from it.  Host only, no HIP call: tests/hostcheck/fields_check.cpp builds it into a program of its own.  cloudsc2_inputs /
// cloudsc2_outputs are blocks of 16 / 10 cloudsc2_field, InPtrs / InPtrsRW / OutPtrs blocks of as many pointers in the same member order
// (asserted below and in cloudsc2_column.hpp): everything here walks them as arrays, field k of a block being member k of its struct.
#pragma once
#include "../../include/cloudsc2_hip.h"
#include "cloudsc2_column.hpp"

namespace cloudsc2 {

int fail(int code, const char* msg);  // cloudsc2_launch.hip (a test program brings its own)

// the layout groups, in the member order of Strides (cloudsc2_column.hpp says what each is)
enum FieldGroup { kFull = 0, kHalf = 1, kCml = 2, kClv = 3, kLoc = 4, kGroups = 5 };
constexpr int kNumIn = 16, kNumOut = 10;
// paph pap q qsat t l i lude lu mfu mfd gtent gtenq gtenl gteni supsat; all required but qsat
constexpr FieldGroup kInGroup[kNumIn] = {kHalf, kFull, kFull, kFull, kFull, kClv, kClv, kFull, kFull, kFull, kFull, kCml, kCml, kCml, kCml, kFull};
constexpr int kInQsat = 3;
// tent tenq tenl teni clc fplsl fplsn fhpsl fhpsn covptot; the kHalf ones have NLEV + 1 levels
constexpr FieldGroup kOutGroup[kNumOut] = {kLoc, kLoc, kLoc, kLoc, kFull, kHalf, kHalf, kHalf, kHalf, kFull};

static_assert(sizeof(cloudsc2_inputs) == kNumIn * sizeof(cloudsc2_field) && sizeof(cloudsc2_outputs) == kNumOut * sizeof(cloudsc2_field) &&
                  sizeof(InPtrs) == kNumIn * sizeof(void*) && sizeof(OutPtrs) == kNumOut * sizeof(void*), "blocks of fields and of pointers");
inline const cloudsc2_field* fields_of(const cloudsc2_inputs& x) { return reinterpret_cast<const cloudsc2_field*>(&x); }
inline const cloudsc2_field* fields_of(const cloudsc2_outputs& x) { return reinterpret_cast<const cloudsc2_field*>(&x); }

inline int outputs_given(const cloudsc2_outputs& out) {
  int n = 0;
  for (int k = 0; k < kNumOut; ++k) n += fields_of(out)[k].ptr ? 1 : 0;
  return n;
}

// NBLOCKS * NPROMA: the columns of the whole blocks that hold ngptot columns
inline long long ncols_pad(int nproma, int ngptot) { return (((long long)ngptot + nproma - 1) / nproma) * nproma; }

// the block strides of the fields given (non-NULL) per layout group: the first one's, and whether the others agree
struct GroupStrides {
  long long v[kGroups] = {};
  bool set[kGroups] = {};
  bool ok = true;
  void add(FieldGroup g, const cloudsc2_field& f) {
    if (!f.ptr) return;
    if (!set[g]) { v[g] = f.block_stride; set[g] = true; }
    else if (v[g] != f.block_stride) ok = false;
  }
};

// s: full, half, cml and clv are set (0: no field of the group given), loc is left as it is
inline int resolve_in(const cloudsc2_inputs& in, bool need_qsat, Strides& s, InPtrs& p) {
  const cloudsc2_field* f = fields_of(in);
  for (int k = 0; k < kNumIn; ++k)
    if (k != kInQsat && !f[k].ptr) return fail(CLOUDSC2_EINVAL, "a required input field has a NULL pointer");
  if (need_qsat && !f[kInQsat].ptr) return fail(CLOUDSC2_EINVAL, "qsat field required");
  GroupStrides g;
  for (int k = 0; k < kNumIn; ++k) {
    g.add(kInGroup[k], f[k]);
    reinterpret_cast<const real_t**>(&p)[k] = f[k].ptr;
  }
  if (!g.ok) return fail(CLOUDSC2_EINVAL, "fields of one layout group (full-level / PGTEN* / PL,PI) must share one block stride");
  s.full = g.v[kFull]; s.half = g.v[kHalf]; s.cml = g.v[kCml]; s.clv = g.v[kClv];
  return 0;
}

// s on entry: the strides of the inputs the outputs go with (0: none) -- the full-level and half-level outputs must have theirs; on
// return full and half are the outputs' where one is given, loc is the outputs' (0: none given)
inline int resolve_out(const cloudsc2_outputs& out, bool all_required, Strides& s, OutPtrs& p) {
  const cloudsc2_field* f = fields_of(out);
  if (all_required && outputs_given(out) != kNumOut) return fail(CLOUDSC2_EINVAL, "a required output field has a NULL pointer");
  GroupStrides g;
  for (int k = 0; k < kNumOut; ++k) {
    g.add(kOutGroup[k], f[k]);
    reinterpret_cast<real_t**>(&p)[k] = f[k].ptr;
  }
  if (!g.ok) return fail(CLOUDSC2_EINVAL, "output fields of one layout group must share one block stride");
  if (g.set[kFull] && s.full && s.full != g.v[kFull]) return fail(CLOUDSC2_EINVAL, "PCLC/PCOVPTOT stride differs from the input full-level stride");
  if (g.set[kHalf] && s.half && s.half != g.v[kHalf]) return fail(CLOUDSC2_EINVAL, "flux stride differs from the PAPH stride");
  if (g.set[kFull]) s.full = g.v[kFull];
  if (g.set[kHalf]) s.half = g.v[kHalf];
  s.loc = g.v[kLoc];
  return 0;
}

// The sparse launchers' blocks (cloudsc2_tl_launch_sparse: pert_in, pert_out; cloudsc2_vjp_launch_sparse: adj_in, adj_out): any field
// may be NULL.  s: the block stride of every layout group with a member present on either side (the full-level and half-level groups
// span both blocks, as in resolve_out), 0 for a group with none -- it has no stride and needs none; the pointers as given; in_mask /
// out_mask: one bit per field present, in this table's order.  `written`: which of the two blocks the sweep writes ('i' or 'o'): a plane
// given twice there is refused.
inline int resolve_sparse(const cloudsc2_inputs& in, const cloudsc2_outputs& out, char written, Strides& s, InPtrs& pi, OutPtrs& po,
                          unsigned& in_mask, unsigned& out_mask) {
  const cloudsc2_field *fi = fields_of(in), *fo = fields_of(out);
  GroupStrides g;
  in_mask = out_mask = 0u;
  for (int k = 0; k < kNumIn; ++k) {
    g.add(kInGroup[k], fi[k]);
    reinterpret_cast<const real_t**>(&pi)[k] = fi[k].ptr;
    if (fi[k].ptr) in_mask |= 1u << k;
  }
  for (int k = 0; k < kNumOut; ++k) {
    g.add(kOutGroup[k], fo[k]);
    reinterpret_cast<real_t**>(&po)[k] = fo[k].ptr;
    if (fo[k].ptr) out_mask |= 1u << k;
  }
  if (!g.ok) return fail(CLOUDSC2_EINVAL, "sparse sweep: the present fields of one layout group must share one block stride");
  const cloudsc2_field* fw = written == 'i' ? fi : fo;
  const int nw = written == 'i' ? kNumIn : kNumOut;
  for (int a = 0; a < nw; ++a)
    for (int b = a + 1; b < nw; ++b)
      if (fw[a].ptr && fw[a].ptr == fw[b].ptr) return fail(CLOUDSC2_EINVAL, "sparse sweep: a written plane is given twice");
  s.full = g.v[kFull]; s.half = g.v[kHalf]; s.cml = g.v[kCml]; s.clv = g.v[kClv]; s.loc = g.v[kLoc];
  return 0;
}

// the pointers of a block the sweep writes (the input adjoints)
inline InPtrsRW writable(const cloudsc2_inputs& x) {
  InPtrsRW p;
  for (int k = 0; k < kNumIn; ++k) reinterpret_cast<real_t**>(&p)[k] = fields_of(x)[k].ptr;
  return p;
}

}  // namespace cloudsc2
