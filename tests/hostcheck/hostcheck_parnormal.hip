// TEST-ONLY: the normal-equations sweep of the parameters (parnormal_column: what cloudsc2_parnormal_launch runs first) compiled for
// the HOST, on top of the helpers of hostcheck.hip.  The sensitivities it must contract are hostcheck_parjac.hip's hostcheck_tl_parjac;
// the fold over the columns is summed by the test.  Like hostcheck.hip, never loaded by the package.
#include "hostcheck.hip"

template <unsigned F> struct HcParNormal {
  static void run(long long gc, const ParNormalArgs* a) {
    if constexpr ((F & ~(C2F_QSAT | C2F_PRECISE | C2F_EVAP)) == 0) parnormal_column<F>(gc, a);
  }
};

extern "C" {

// cloudsc2_parnormal_launch's sweep: work[(CLOUDSC2_NNORMAL, ncols_pad)] receives every active column's sums (without the evaporation
// branch the rows with rpecons are not written).  resid: a NULL field is an unobserved output; weight: NULL, or NULL fields = weight 1;
// in->qsat NULL: SATUR evaluated in the sweep.
int hostcheck_parnormal(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, const cloudsc2_inputs* in,
                        const cloudsc2_outputs* resid, const cloudsc2_outputs* weight, double* work) {
  ParNormalArgs a;
  LevelTab tab;
  const unsigned f = hc_par_head(a, tab, prm, ptsphy, nproma, nlev, ngptot, in);
  hc_out(*resid, a.sr, a.resid);
  // (one block stride per layout group, taken from whichever member is observed)
  a.sr.loc = resid->tent.ptr ? resid->tent.block_stride : resid->tenq.ptr ? resid->tenq.block_stride
             : resid->tenl.ptr ? resid->tenl.block_stride : resid->teni.block_stride;
  a.sr.half = resid->fplsl.ptr ? resid->fplsl.block_stride : resid->fplsn.ptr ? resid->fplsn.block_stride
              : resid->fhpsl.ptr ? resid->fhpsl.block_stride : resid->fhpsn.block_stride;
  a.sr.full = resid->clc.ptr ? resid->clc.block_stride : resid->covptot.block_stride;
  if (weight) { Strides unused = {0, 0, 0, 0, 0}; hc_out(*weight, unused, a.weight); }
  a.work = work;
  for (long long gc = 0; gc < a.g.ncols_pad; ++gc) hc_dispatch<HcParNormal, 8>(f, gc, &a);
  return 0;
}

}  // extern "C"
