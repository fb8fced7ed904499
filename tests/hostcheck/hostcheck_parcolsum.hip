// TEST-ONLY: the parameter column-sum sweep (parcolsum_column: what cloudsc2_parjac_launch_colsum and cloudsc2_parnormal_launch_colsum
// run) compiled for the HOST, on top of the helpers of hostcheck.hip.  The sensitivities it must fold are hostcheck_parjac.hip's
// hostcheck_tl_parjac; the fold over the columns of the normal form is summed by the test.  Absent sums, residuals and weights are NULL
// pointers: a guard that is missing in the column function dereferences one here, on the CPU.  Like hostcheck.hip, never loaded by the
// package.
#include "hostcheck.hip"

template <unsigned F> struct HcParColsum {
  static void run(long long gc, const ParColsumArgs* a) {
    if constexpr ((F & ~(C2F_QSAT | C2F_PRECISE | C2F_EVAP | C2F_NORMAL)) == 0) parcolsum_column<F>(gc, a);
  }
};

// the fields given of a block of (nblocks, nproma) arrays: their pointers, the mask, the block stride of the last one
static unsigned hc_parcolsum_block(const cloudsc2_outputs& blk, OutPtrs& y, long long& stride) {
  static_assert(sizeof(cloudsc2_outputs) == 10 * sizeof(cloudsc2_field) && sizeof(OutPtrs) == 10 * sizeof(void*), "ten fields, ten pointers");
  const cloudsc2_field* f = reinterpret_cast<const cloudsc2_field*>(&blk);
  unsigned mask = 0u;
  for (int k = 0; k < 10; ++k) {
    reinterpret_cast<real_t**>(&y)[k] = f[k].ptr;
    if (f[k].ptr) { mask |= 1u << k; stride = f[k].block_stride; }
  }
  return mask;
}

static void hc_parcolsum_run(const ParColsumArgs& a, unsigned f) {
  for (long long gc = 0; gc < a.g.ncols_pad; ++gc) hc_dispatch<HcParColsum, 16>(f, gc, &a);
}

extern "C" {

// cloudsc2_parjac_launch_colsum: sums[k] receives the sensitivities of the sums present to parameter k, k in CLOUDSC2_NPAR order (the
// fields present are those of sums[0]); in->qsat NULL: SATUR evaluated in the sweep.  Without the evaporation branch sums[3] is not
// looked at.
int hostcheck_parjac_colsum(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, const cloudsc2_inputs* in,
                            const cloudsc2_real* wtable, const cloudsc2_outputs* sums) {
  ParColsumArgs a;
  LevelTab tab;
  const unsigned f = hc_par_head(a, tab, prm, ptsphy, nproma, nlev, ngptot, in);
  a.cs.w = wtable;
  for (int b = 0; b < hc_par_directions(a.c); ++b) {
    const unsigned m = hc_parcolsum_block(sums[b], a.y[b], a.cs.stride);
    if (b == 0) a.cs.mask = m;
    else if (m != a.cs.mask) return -1;
  }
  if (!a.cs.mask) return -1;
  hc_parcolsum_run(a, f);
  return 0;
}

// cloudsc2_parnormal_launch_colsum's sweep: work[(CLOUDSC2_NNORMAL, ncols_pad)] receives every active column's sums (without the evaporation
// branch the rows with rpecons are not written).  resid: a NULL field is an unobserved sum; weight: NULL, or NULL fields = weight 1.
int hostcheck_parnormal_colsum(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, const cloudsc2_inputs* in,
                               const cloudsc2_real* wtable, const cloudsc2_outputs* resid, const cloudsc2_outputs* weight, double* work) {
  ParColsumArgs a;
  LevelTab tab;
  const unsigned f = hc_par_head(a, tab, prm, ptsphy, nproma, nlev, ngptot, in);
  a.cs.w = wtable;
  if (!(a.cs.mask = hc_parcolsum_block(*resid, a.y[0], a.cs.stride))) return -1;
  long long unused = 0;
  if (weight) hc_parcolsum_block(*weight, a.y[1], unused);
  a.work = work;
  hc_parcolsum_run(a, f | C2F_NORMAL);
  return 0;
}

}  // extern "C"
