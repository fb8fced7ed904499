// TEST-ONLY: SATUR with its partial derivatives (satur_lin_point) and the sweeps that differentiate through it (C2F_SATLIN:
// cloudsc2_tl_launch_satur, cloudsc2_vjp_launch_satur) compiled for the HOST, on top of the helpers of hostcheck.hip.  Like
// hostcheck.hip, never loaded by the package.
#include "hostcheck.hip"

template <unsigned F> struct HcTlSatur {
  static void run(long long gc, const TlArgs* a) {
    // the flag words cloudsc2_tl_launch_satur produces (64-bit offsets)
    if constexpr ((F & ~(C2F_PRECISE | C2F_EVAP)) == C2F_SATLIN) tl_column<F>(gc, a);
  }
};
template <unsigned F> struct HcVjpSatur {
  static void run(long long gc, const AdArgs* a) {
    // the flag words cloudsc2_vjp_launch_satur produces (64-bit offsets)
    if constexpr ((F & ~(C2F_PRECISE | C2F_EVAP)) == (C2F_SATLIN | C2F_ASSIGN | C2F_VJP)) ad_reverse_column<F>(gc, a);
  }
};

extern "C" {

// cloudsc2_satur_lin_launch: qsat (may be NULL) and the two partial planes
int hostcheck_satur_lin(const cloudsc2_params* prm, int nproma, int nlev, int ngptot, cloudsc2_field pap, cloudsc2_field t,
                        cloudsc2_field qsat, cloudsc2_field dqs_dpap, cloudsc2_field dqs_dt) {
  SaturLinArgs a;
  a.g = hc_geom(nproma, nlev, ngptot);
  a.c = hc_consts(*prm, 1.0);
  a.s = Strides{pap.block_stride, 0, 0, 0, 0};
  a.pap = pap.ptr; a.t = t.ptr; a.qsat = qsat.ptr; a.dqs_dpap = dqs_dpap.ptr; a.dqs_dt = dqs_dt.ptr;
  for (long long gc = 0; gc < a.g.ncols_pad; ++gc) { if (g_hc_precise) satur_lin_column<true>(gc, &a); else satur_lin_column<false>(gc, &a); }
  return 0;
}

// cloudsc2_tl_launch_satur: in->qsat and din->qsat are not read (pass NULL); no trajectory stores
int hostcheck_tl_satur(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, const cloudsc2_inputs* in,
                       const cloudsc2_inputs* din, const cloudsc2_outputs* dout) {
  if (in->qsat.ptr || din->qsat.ptr) return -1;
  TlArgs a;
  memset(&a, 0, sizeof(a));
  a.g = hc_geom(nproma, nlev, ngptot);
  a.c = hc_consts(*prm, ptsphy);
  LevelTab tab; hc_tables(*prm, tab, a.g);
  a.tab = &tab;
  a.s = Strides{0, 0, 0, 0, 0}; a.sp = Strides{0, 0, 0, 0, 0};
  hc_in(*in, a.s, a.in); hc_in(*din, a.sp, a.din); hc_out(*dout, a.sp, a.dout);
  const unsigned f = C2F_SATLIN | (g_hc_precise ? C2F_PRECISE : 0u) | (a.c.evap ? C2F_EVAP : 0u);
  for (long long gc = 0; gc < a.g.ncols_pad; ++gc) hc_dispatch<HcTlSatur, 256>(f, gc, &a);
  return 0;
}

// cloudsc2_vjp_launch_satur: the reverse sweep alone; out: PFPLSL5 / PFPLSN5 are read, `scratch`: the cover checkpoints of the
// trajectory pass (hostcheck_vjp_sweep, sweep 1); in->qsat and ain->qsat are not read or written (pass NULL)
int hostcheck_vjp_satur(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, const cloudsc2_inputs* in,
                        const cloudsc2_outputs* out, const cloudsc2_inputs* ain, const cloudsc2_outputs* aout, cloudsc2_real* scratch) {
  if (in->qsat.ptr || ain->qsat.ptr) return -1;
  AdArgs a;
  memset(&a, 0, sizeof(a));
  a.nl.g = hc_geom(nproma, nlev, ngptot);
  a.nl.c = hc_consts(*prm, ptsphy);
  LevelTab tab; hc_tables(*prm, tab, a.nl.g);
  a.nl.tab = &tab;
  a.nl.s = Strides{0, 0, 0, 0, 0}; a.sa = Strides{0, 0, 0, 0, 0};
  hc_in(*in, a.nl.s, a.nl.in); hc_out(*out, a.nl.s, a.nl.out);
  InPtrs aip_c;
  hc_in(*ain, a.sa, aip_c); hc_out(*aout, a.sa, a.aout);
  a.ain.paph = ain->paph.ptr; a.ain.pap = ain->pap.ptr; a.ain.q = ain->q.ptr; a.ain.qsat = nullptr; a.ain.t = ain->t.ptr;
  a.ain.l = ain->l.ptr; a.ain.i = ain->i.ptr; a.ain.lude = ain->lude.ptr; a.ain.lu = ain->lu.ptr; a.ain.mfu = ain->mfu.ptr;
  a.ain.mfd = ain->mfd.ptr; a.ain.gt = ain->gtent.ptr; a.ain.gq = ain->gtenq.ptr; a.ain.gl = ain->gtenl.ptr;
  a.ain.gi = ain->gteni.ptr; a.ain.supsat = ain->supsat.ptr;
  a.nl.ckpt = scratch;
  const unsigned f = C2F_SATLIN | C2F_ASSIGN | C2F_VJP | (g_hc_precise ? C2F_PRECISE : 0u) | (a.nl.c.evap ? C2F_EVAP : 0u);
  for (long long gc = 0; gc < a.nl.g.ncols_pad; ++gc) hc_dispatch<HcVjpSatur, 256>(f, gc, &a);
  return 0;
}

}  // extern "C"
