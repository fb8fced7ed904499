// TEST-ONLY: per-column parameter maps (C2F_PARMAP: what cloudsc2_{nl,tl,vjp}_launch_parmap run) compiled for the HOST, on top of the
// helpers of hostcheck.hip: the derivation of a lane's constants from its four doubles (lane_consts) and the three sweeps.  Like
// hostcheck.hip, never loaded by the package.
#ifndef CLOUDSC2_HOSTCHECK_PARMAP_HIP
#define CLOUDSC2_HOSTCHECK_PARMAP_HIP
#include "hostcheck.hip"

// the flag words the three launchers produce (64-bit offsets)
template <unsigned F> struct HcNlParmap {
  static void run(long long gc, const NlParmapArgs* a) {
    if constexpr ((F & ~(C2F_QSAT | C2F_PRECISE | C2F_EVAP | C2F_CKPT)) == 0 && ((F & C2F_CKPT) != 0) == ((F & C2F_EVAP) != 0))
      nl_column<F | C2F_PARMAP>(gc, &a->a);
  }
};
static constexpr bool hc_parmap_flags(unsigned f, unsigned form) {
  const unsigned rest = f & ~(C2F_PRECISE | C2F_EVAP);
  return rest == (C2F_PARLIN | form | C2F_QSAT) || rest == (C2F_PARLIN | form | C2F_SATLIN);
}
template <unsigned F> struct HcTlParmap {
  static void run(long long gc, const TlParmapArgs* a) {
    if constexpr (hc_parmap_flags(F, 0u)) tl_column<F | C2F_PARMAP>(gc, &a->a);
  }
};
template <unsigned F> struct HcVjpParmap {
  static void run(long long gc, const AdParmapArgs* a) {
    if constexpr (hc_parmap_flags(F, C2F_ASSIGN | C2F_VJP)) ad_reverse_column<F | C2F_PARMAP>(gc, &a->a);
  }
};

static cloudsc2_params hc_with_row(const cloudsc2_params& prm, const double* par) {
  cloudsc2_params p = prm;
  p.rkconv = par[PAR_RKCONV]; p.rclcrit = par[PAR_RCLCRIT]; p.rlptrc = par[PAR_RLPTRC]; p.rpecons = par[PAR_RPECONS];
  return p;
}
static bool hc_same(real_t a, real_t b) { return memcmp(&a, &b, sizeof(real_t)) == 0; }

extern "C" {

int hostcheck_parmap_real_bytes(void) { return (int)sizeof(real_t); }

// A lane's constants from its four doubles against the host's: make_consts of a parameter block holding them, make_parlin of that
// (dpar may be NULL).  0: the same bytes; bit 0: a constant level_forward reads differs; bit 1: one that level_tl / level_ad read;
// bit 2: the ParLin.
int hostcheck_parmap_lane_consts(const cloudsc2_params* prm, double ptsphy, const double* par, const double* dpar) {
  const Consts base = make_consts(*prm, ptsphy);
  LanePar l;
  memset(&l, 0xff, sizeof(l));
  lane_consts(l, base.evap, base.lregcl, ptsphy, par, dpar);
  Consts want;
  ParLin pwant;
  memset(&want, 0, sizeof(want)); memset(&pwant, 0, sizeof(pwant));
  want = make_consts(hc_with_row(*prm, par), ptsphy);
  pwant = make_parlin(want, dpar);
  int rc = 0;
  const real_t* k3 = want.k3.v;
  if (!hc_same(l.rlptrc, want.k0.v[K0_RLPTRC]) || !hc_same(l.rpecons, want.rpecons) || !hc_same(l.zlcrit_l, k3[K3_ZLCRIT_L]) ||
      !hc_same(l.zlcrit_l_r, k3[K3_ZLCRIT_L_R]) || !hc_same(l.zckcodtl, k3[K3_ZCKCODTL]) || !hc_same(l.zlcrit_i, k3[K3_ZLCRIT_I]) ||
      !hc_same(l.zlcrit_i_r, k3[K3_ZLCRIT_I_R]) || !hc_same(l.zckcodti, k3[K3_ZCKCODTI]))
    rc |= 1;
  if (!hc_same(l.zlcrit_l_r2, want.kt1.v[KT1_ZLCRIT_L_R2]) || !hc_same(l.zlcrit_i_r2, want.kt1.v[KT1_ZLCRIT_I_R2]) ||
      !hc_same(l.ck_l, want.kt2.v[KT2_CK_L]) || !hc_same(l.ck_i, want.kt2.v[KT2_CK_I]))
    rc |= 2;
  ParLin pgot;
  memset(&pgot, 0, sizeof(pgot));
  pgot = l.pl;
  if (memcmp(&pgot, &pwant, sizeof(ParLin))) rc |= 4;
  return rc;
}

// cloudsc2_nl_launch_parmap: the trajectory pass (out: all ten; `scratch`: the cover checkpoints, written with the evaporation branch);
// in->qsat given, or NULL: SATUR evaluated in the sweep.  par: (4, ncols_pad) doubles.
int hostcheck_parmap_nl(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, const double* par,
                        const cloudsc2_inputs* in, const cloudsc2_outputs* out, cloudsc2_real* scratch) {
  NlParmapArgs pa;
  memset(&pa, 0, sizeof(pa));
  NlArgs& a = pa.a;
  a.g = hc_geom(nproma, nlev, ngptot);
  a.c = hc_consts(*prm, ptsphy);
  LevelTab tab; hc_tables(*prm, tab, a.g);
  a.tab = &tab;
  a.s = Strides{0, 0, 0, 0, 0};
  hc_in(*in, a.s, a.in); hc_out(*out, a.s, a.out);
  a.ckpt = scratch;
  pa.par = par; pa.ptsphy = ptsphy;
  const unsigned f = (in->qsat.ptr ? C2F_QSAT : 0u) | (g_hc_precise ? C2F_PRECISE : 0u) | (a.c.evap ? C2F_EVAP | C2F_CKPT : 0u);
  for (long long gc = 0; gc < a.g.ncols_pad; ++gc) hc_dispatch<HcNlParmap, 64>(f, gc, &pa);
  return 0;
}

// cloudsc2_tl_launch_parmap.  satur = 0: in->qsat and din->qsat given; satur = 1: both NULL.  par, dpar: (4, ncols_pad) doubles.
int hostcheck_parmap_tl(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, int satur, const double* par,
                        const double* dpar, const cloudsc2_inputs* in, const cloudsc2_inputs* din, const cloudsc2_outputs* dout) {
  if (satur ? (in->qsat.ptr || din->qsat.ptr) : (!in->qsat.ptr || !din->qsat.ptr)) return -1;
  TlParmapArgs pa;
  memset(&pa, 0, sizeof(pa));
  TlArgs& a = pa.a;
  a.g = hc_geom(nproma, nlev, ngptot);
  a.c = hc_consts(*prm, ptsphy);
  LevelTab tab; hc_tables(*prm, tab, a.g);
  a.tab = &tab;
  a.s = Strides{0, 0, 0, 0, 0}; a.sp = Strides{0, 0, 0, 0, 0};
  hc_in(*in, a.s, a.in); hc_in(*din, a.sp, a.din); hc_out(*dout, a.sp, a.dout);
  pa.par = par; pa.dpar = dpar; pa.ptsphy = ptsphy;
  const unsigned f = C2F_PARLIN | (satur ? C2F_SATLIN : C2F_QSAT) | (g_hc_precise ? C2F_PRECISE : 0u) | (a.c.evap ? C2F_EVAP : 0u);
  for (long long gc = 0; gc < a.g.ncols_pad; ++gc) hc_dispatch<HcTlParmap, 512>(f, gc, &pa);
  return 0;
}

// cloudsc2_vjp_launch_parmap: the reverse sweep alone (out: PFPLSL5 / PFPLSN5 are read; `scratch`: the cover checkpoints of the
// trajectory pass).  par, apar: (4, ncols_pad) doubles; apar is assigned in the active columns.
int hostcheck_parmap_vjp(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, int satur, const double* par,
                         const cloudsc2_inputs* in, const cloudsc2_outputs* out, const cloudsc2_inputs* ain, const cloudsc2_outputs* aout,
                         cloudsc2_real* scratch, double* apar) {
  if (satur ? (in->qsat.ptr || ain->qsat.ptr) : (!in->qsat.ptr || !ain->qsat.ptr)) return -1;
  AdParmapArgs pa;
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
  pa.par = par; pa.apar = apar; pa.ptsphy = ptsphy;
  const unsigned f = C2F_PARLIN | C2F_ASSIGN | C2F_VJP | (satur ? C2F_SATLIN : C2F_QSAT) | (g_hc_precise ? C2F_PRECISE : 0u) |
                     (a.nl.c.evap ? C2F_EVAP : 0u);
  for (long long gc = 0; gc < a.nl.g.ncols_pad; ++gc) hc_dispatch<HcVjpParmap, 512>(f, gc, &pa);
  return 0;
}

}  // extern "C"

#endif  // CLOUDSC2_HOSTCHECK_PARMAP_HIP
