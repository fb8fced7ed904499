// TEST-ONLY: the parameter forms of the TL sweep and of the reverse sweep's vector-Jacobian product (C2F_PARLIN: what
// cloudsc2_tl_launch_par and cloudsc2_vjp_launch_par run) compiled for the HOST, on top of the helpers of hostcheck.hip.  Like
// hostcheck.hip, never loaded by the package.
#include "hostcheck.hip"

// the flag words cloudsc2_tl_launch_par (form = 0) and cloudsc2_vjp_launch_par (form = ASSIGN | VJP) produce (64-bit offsets)
static constexpr bool hc_par_flags(unsigned f, unsigned form) {
  const unsigned rest = f & ~(C2F_PRECISE | C2F_EVAP);
  return rest == (C2F_PARLIN | form | C2F_QSAT) || rest == (C2F_PARLIN | form | C2F_SATLIN);
}
template <unsigned F> struct HcTlPar {
  static void run(long long gc, const TlParArgs* a) {
    if constexpr (hc_par_flags(F, 0u)) tl_column<F>(gc, &a->a);
  }
};
template <unsigned F> struct HcVjpPar {
  static void run(long long gc, const AdParArgs* a) {
    if constexpr (hc_par_flags(F, C2F_ASSIGN | C2F_VJP)) ad_reverse_column<F>(gc, &a->a);
  }
};

extern "C" {

// cloudsc2_tl_launch_par.  satur = 0: in->qsat and din->qsat given; satur = 1: both NULL, SATUR differentiated in the sweep
int hostcheck_tl_par(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, int satur, const cloudsc2_inputs* in,
                     const cloudsc2_inputs* din, const double* dpar, const cloudsc2_outputs* dout) {
  if (satur ? (in->qsat.ptr || din->qsat.ptr) : (!in->qsat.ptr || !din->qsat.ptr)) return -1;
  TlParArgs pa;
  memset(&pa, 0, sizeof(pa));
  TlArgs& a = pa.a;
  a.g = hc_geom(nproma, nlev, ngptot);
  a.c = hc_consts(*prm, ptsphy);
  LevelTab tab; hc_tables(*prm, tab, a.g);
  a.tab = &tab;
  a.s = Strides{0, 0, 0, 0, 0}; a.sp = Strides{0, 0, 0, 0, 0};
  hc_in(*in, a.s, a.in); hc_in(*din, a.sp, a.din); hc_out(*dout, a.sp, a.dout);
  pa.par = make_parlin(a.c, dpar);
  const unsigned f = C2F_PARLIN | (satur ? C2F_SATLIN : C2F_QSAT) | (g_hc_precise ? C2F_PRECISE : 0u) | (a.c.evap ? C2F_EVAP : 0u);
  for (long long gc = 0; gc < a.g.ncols_pad; ++gc) hc_dispatch<HcTlPar, 512>(f, gc, &pa);
  return 0;
}

// cloudsc2_vjp_launch_par: the reverse sweep alone (out: PFPLSL5 / PFPLSN5 are read; `scratch`: the cover checkpoints of the trajectory
// pass), then the fold of the workspace.  work: 4 * ncols_pad doubles (written for the active columns only); par_adj: 4 doubles, the
// active columns' sums in column order (the device's fold kernel adds in another fixed order).
int hostcheck_vjp_par(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, int satur, const cloudsc2_inputs* in,
                      const cloudsc2_outputs* out, const cloudsc2_inputs* ain, const cloudsc2_outputs* aout, cloudsc2_real* scratch,
                      double* work, double* par_adj) {
  if (satur ? (in->qsat.ptr || ain->qsat.ptr) : (!in->qsat.ptr || !ain->qsat.ptr)) return -1;
  AdParArgs pa;
  memset(&pa, 0, sizeof(pa));
  AdArgs& a = pa.a;
  a.nl.g = hc_geom(nproma, nlev, ngptot);
  a.nl.c = hc_consts(*prm, ptsphy);
  LevelTab tab; hc_tables(*prm, tab, a.nl.g);
  a.nl.tab = &tab;
  a.nl.s = Strides{0, 0, 0, 0, 0}; a.sa = Strides{0, 0, 0, 0, 0};
  hc_in(*in, a.nl.s, a.nl.in); hc_out(*out, a.nl.s, a.nl.out);
  InPtrs aip_c;
  hc_in(*ain, a.sa, aip_c); hc_out(*aout, a.sa, a.aout);
  a.ain.paph = ain->paph.ptr; a.ain.pap = ain->pap.ptr; a.ain.q = ain->q.ptr; a.ain.qsat = ain->qsat.ptr; a.ain.t = ain->t.ptr;
  a.ain.l = ain->l.ptr; a.ain.i = ain->i.ptr; a.ain.lude = ain->lude.ptr; a.ain.lu = ain->lu.ptr; a.ain.mfu = ain->mfu.ptr;
  a.ain.mfd = ain->mfd.ptr; a.ain.gt = ain->gtent.ptr; a.ain.gq = ain->gtenq.ptr; a.ain.gl = ain->gtenl.ptr;
  a.ain.gi = ain->gteni.ptr; a.ain.supsat = ain->supsat.ptr;
  a.nl.ckpt = scratch;
  pa.par = make_parlin(a.nl.c, nullptr);
  pa.work = work;
  const unsigned f = C2F_PARLIN | C2F_ASSIGN | C2F_VJP | (satur ? C2F_SATLIN : C2F_QSAT) | (g_hc_precise ? C2F_PRECISE : 0u) |
                     (a.nl.c.evap ? C2F_EVAP : 0u);
  const long long np = a.nl.g.ncols_pad;
  for (long long gc = 0; gc < np; ++gc) hc_dispatch<HcVjpPar, 512>(f, gc, &pa);
  for (int i = 0; i < PAR_COUNT; ++i) {
    double s = 0.0;
    for (long long gc = 0; gc < ngptot; ++gc) s += work[i * np + gc];
    par_adj[i] = s;
  }
  return 0;
}

}  // extern "C"
