// TEST-ONLY: the parameter Jacobian's sweep (tl_parjac_column: what cloudsc2_tl_launch_parjac runs) compiled for the HOST, on top of
// the helpers of hostcheck.hip (the single-direction parameter TL it must reproduce bit for bit is hostcheck_par.hip's
// hostcheck_tl_par).  Like hostcheck.hip, never loaded by the package.
#include "hostcheck.hip"

template <unsigned F> struct HcTlParJac {
  static void run(long long gc, const TlParJacArgs* a) {
    if constexpr ((F & ~(C2F_QSAT | C2F_PRECISE | C2F_EVAP)) == 0) tl_parjac_column<F>(gc, a);
  }
};

extern "C" {

// cloudsc2_tl_launch_parjac: dout[k] receives d out / d p_k, k in CLOUDSC2_NPAR order; in->qsat NULL: SATUR evaluated in the sweep.
// Without the evaporation branch dout[3] is not looked at.
int hostcheck_tl_parjac(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, const cloudsc2_inputs* in,
                        const cloudsc2_outputs* dout) {
  TlParJacArgs a;
  LevelTab tab;
  const unsigned f = hc_par_head(a, tab, prm, ptsphy, nproma, nlev, ngptot, in);
  for (int b = 0; b < hc_par_directions(a.c); ++b) {
    hc_out(dout[b], a.sp, a.dout[b]);
    a.sp.full = dout[b].clc.block_stride; a.sp.half = dout[b].fplsl.block_stride;
  }
  for (long long gc = 0; gc < a.g.ncols_pad; ++gc) hc_dispatch<HcTlParJac, 8>(f, gc, &a);
  return 0;
}

}  // extern "C"
