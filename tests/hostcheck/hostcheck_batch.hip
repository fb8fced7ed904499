// TEST-ONLY: the batched TL and reverse sweeps (tl_batch_column, vjp_batch_column: cloudsc2_tl_launch_batch /
// cloudsc2_vjp_launch_batch) compiled for the HOST, on top of the helpers of hostcheck.hip -- to be compared with K runs of the
// single-direction sweeps (hostcheck_tl, hostcheck_vjp_sweep).  Like hostcheck.hip, never loaded by the package.
#include "hostcheck.hip"

// (the direction count is a compile-time one: flag word + 64 x directions, as in the library's variant tables)
template <unsigned G> struct HcTlBatch {
  static void run(long long gc, const TlBatchArgs* a) {
    constexpr unsigned F = G % 64u;
    constexpr int NB = (int)(G / 64u);
    if constexpr ((F & C2F_QSAT) && (F & ~(C2F_QSAT | C2F_PRECISE | C2F_EVAP | C2F_OFF32)) == 0 && NB >= 1 && NB <= kBatchMax)
      tl_batch_column<F, NB>(gc, a);
  }
};
template <unsigned G> struct HcVjpBatch {
  static void run(long long gc, const VjpBatchArgs* a) {
    constexpr unsigned F = G % 64u;
    constexpr int NB = (int)(G / 64u);
    if constexpr ((F & C2F_QSAT) && (F & ~(C2F_QSAT | C2F_PRECISE | C2F_EVAP | C2F_OFF32)) == 0 && NB >= 1 && NB <= kBatchMax)
      vjp_batch_column<F, NB>(gc, a);
  }
};

static unsigned hc_batch_flags(bool evap) {
  return C2F_QSAT | (g_hc_precise ? C2F_PRECISE : 0u) | (evap ? C2F_EVAP : 0u) | (g_hc_off32 ? C2F_OFF32 : 0u);
}

extern "C" {

int hostcheck_batch_max(void) { return kBatchMax; }

// nb <= kBatchMax tangents over one trajectory in ONE sweep (no chunking here: that is the launcher's)
int hostcheck_tl_batch(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, const cloudsc2_inputs* in,
                       int nb, const cloudsc2_inputs* din, const cloudsc2_outputs* dout) {
  if (nb < 1 || nb > kBatchMax || !in->qsat.ptr) return -1;
  TlBatchArgs a;
  memset(&a, 0, sizeof(a));
  a.g = hc_geom(nproma, nlev, ngptot);
  a.c = hc_consts(*prm, ptsphy);
  LevelTab tab; hc_tables(*prm, tab, a.g);
  a.tab = &tab;
  a.s = Strides{0, 0, 0, 0, 0}; a.sp = Strides{0, 0, 0, 0, 0};
  hc_in(*in, a.s, a.in);
  a.s.loc = 0;
  for (int b = 0; b < nb; ++b) { hc_in(din[b], a.sp, a.din[b]); hc_out(dout[b], a.sp, a.dout[b]); }
  const unsigned f = hc_batch_flags(a.c.evap);
  for (long long gc = 0; gc < a.g.ncols_pad; ++gc) hc_dispatch<HcTlBatch, 64 * (kBatchMax + 1)>(f + 64u * (unsigned)nb, gc, &a);
  return 0;
}

// nb <= kBatchMax cotangents in ONE reverse sweep; out: the trajectory outputs of an earlier sweep (PFPLSL5 / PFPLSN5 are read),
// scratch: the cover checkpoints of the trajectory pass
int hostcheck_vjp_batch(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, const cloudsc2_inputs* in,
                        const cloudsc2_outputs* out, int nb, const cloudsc2_inputs* ain, const cloudsc2_outputs* aout,
                        cloudsc2_real* scratch) {
  if (nb < 1 || nb > kBatchMax || !in->qsat.ptr) return -1;
  VjpBatchArgs a;
  memset(&a, 0, sizeof(a));
  a.nl.g = hc_geom(nproma, nlev, ngptot);
  a.nl.c = hc_consts(*prm, ptsphy);
  LevelTab tab; hc_tables(*prm, tab, a.nl.g);
  a.nl.tab = &tab;
  a.nl.s = Strides{0, 0, 0, 0, 0}; a.sa = Strides{0, 0, 0, 0, 0};
  hc_in(*in, a.nl.s, a.nl.in); hc_out(*out, a.nl.s, a.nl.out);
  for (int b = 0; b < nb; ++b) {
    InPtrs aip_c;
    hc_in(ain[b], a.sa, aip_c); hc_out(aout[b], a.sa, a.aout[b]);
    InPtrsRW& p = a.ain[b];
    p.paph = ain[b].paph.ptr; p.pap = ain[b].pap.ptr; p.q = ain[b].q.ptr; p.qsat = ain[b].qsat.ptr; p.t = ain[b].t.ptr;
    p.l = ain[b].l.ptr; p.i = ain[b].i.ptr; p.lude = ain[b].lude.ptr; p.lu = ain[b].lu.ptr; p.mfu = ain[b].mfu.ptr;
    p.mfd = ain[b].mfd.ptr; p.gt = ain[b].gtent.ptr; p.gq = ain[b].gtenq.ptr; p.gl = ain[b].gtenl.ptr; p.gi = ain[b].gteni.ptr;
    p.supsat = ain[b].supsat.ptr;
  }
  a.nl.ckpt = scratch;
  const unsigned f = hc_batch_flags(a.nl.c.evap);
  for (long long gc = 0; gc < a.nl.g.ncols_pad; ++gc) hc_dispatch<HcVjpBatch, 64 * (kBatchMax + 1)>(f + 64u * (unsigned)nb, gc, &a);
  return 0;
}

}  // extern "C"
