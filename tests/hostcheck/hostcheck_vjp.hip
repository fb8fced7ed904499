// TEST-ONLY: the vector-Jacobian form of the adjoint's reverse sweep (C2F_VJP, cloudsc2_vjp_launch) compiled for the HOST next to
// the assign form it is compared with, on top of the helpers of hostcheck.hip.  Like hostcheck.hip, never loaded by the package.
#include "hostcheck.hip"

template <unsigned F> struct HcVjp {
  static void run(long long gc, const AdArgs* a) {
    // the flag words cloudsc2_ad_launch_forward / cloudsc2_ad_launch_reverse(assign=1) / cloudsc2_vjp_launch produce (64-bit offsets)
    if constexpr ((F & ~(C2F_QSAT | C2F_PRECISE | C2F_EVAP | C2F_ASSIGN | C2F_VJP)) == 0 && (F & C2F_ASSIGN)) {
      if (g_hc_ad_sweep == 1) nl_column<(F & ~(C2F_ASSIGN | C2F_VJP)) | C2F_CKPT>(gc, &a->nl);
      else ad_reverse_column<F>(gc, a);
    }
  }
};

extern "C" {

// sweep 1: the trajectory pass (traj_out and the cover checkpoints in `scratch` written; ain / aout not touched);
// sweep 2: the reverse sweep alone, the assign form (vjp = 0, cloudsc2_ad_launch_reverse with assign = 1) or the vector-Jacobian
// product (vjp = 1, cloudsc2_vjp_launch)
int hostcheck_vjp_sweep(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, const cloudsc2_inputs* in,
                        const cloudsc2_outputs* out, const cloudsc2_inputs* ain, const cloudsc2_outputs* aout, cloudsc2_real* scratch,
                        int sweep, int vjp) {
  if (sweep != 1 && sweep != 2) return -1;
  AdArgs a;
  memset(&a, 0, sizeof(a));
  a.nl.g = hc_geom(nproma, nlev, ngptot);
  a.nl.c = hc_consts(*prm, ptsphy);
  LevelTab tab; hc_tables(*prm, tab, a.nl.g);
  a.nl.tab = &tab;
  a.nl.s = Strides{0, 0, 0, 0, 0}; a.sa = Strides{0, 0, 0, 0, 0};
  hc_in(*in, a.nl.s, a.nl.in); hc_out(*out, a.nl.s, a.nl.out);
  if (sweep == 2) {
    InPtrs aip_c;
    hc_in(*ain, a.sa, aip_c); hc_out(*aout, a.sa, a.aout);
    a.ain.paph = ain->paph.ptr; a.ain.pap = ain->pap.ptr; a.ain.q = ain->q.ptr; a.ain.qsat = ain->qsat.ptr; a.ain.t = ain->t.ptr;
    a.ain.l = ain->l.ptr; a.ain.i = ain->i.ptr; a.ain.lude = ain->lude.ptr; a.ain.lu = ain->lu.ptr; a.ain.mfu = ain->mfu.ptr;
    a.ain.mfd = ain->mfd.ptr; a.ain.gt = ain->gtent.ptr; a.ain.gq = ain->gtenq.ptr; a.ain.gl = ain->gtenl.ptr;
    a.ain.gi = ain->gteni.ptr; a.ain.supsat = ain->supsat.ptr;
  }
  a.nl.ckpt = scratch;
  const unsigned f = (in->qsat.ptr ? C2F_QSAT : 0u) | (g_hc_precise ? C2F_PRECISE : 0u) | (a.nl.c.evap ? C2F_EVAP : 0u) |
                     C2F_ASSIGN | (vjp ? C2F_VJP : 0u);
  g_hc_ad_sweep = sweep;
  for (long long gc = 0; gc < a.nl.g.ncols_pad; ++gc) hc_dispatch<HcVjp, 128>(f, gc, &a);
  g_hc_ad_sweep = 0;
  return 0;
}

}  // extern "C"
