// TEST-ONLY: a census of the branch outcomes of level_forward, compiled for the HOST on top of the helpers of hostcheck.hip.
// It walks a column with the pieces nl_column itself is made of (lane_setup, load_level, make_level_in, level_cst, tropopause /
// rhcrit_setup, level_forward<P, EVAP>) and writes one signature word per (block, level, lane): the predicates LevelTraj records,
// which level_tl and level_ad branch on, plus a few derived bits.  The outputs of the walk are stored like nl_column's, so that a
// test can prove the census saw the column the sweep computes.  Like hostcheck.hip, never loaded by the package.
#include <stdint.h>

#include "hostcheck.hip"

// Bit layout of a signature word (tests/branch_atlas.py names the same bits).
//
// Two pairs of LevelTraj are one predicate each and get no bit of their own:
//  * covpclr1 < 0 never holds: covptot1 = newmax ? clc : covptot_in is max(clc, covptot_in), so covpclr1 = covptot1 - clc is the
//    difference of a number and one not larger, which rounds to zero or above;
//  * reset == dpr_clip: zpreclr = zpreclr1 - min(zdpr1, zpreclr1) (the fast form writes the clipped case as an exact 0) is <= 0
//    exactly when zdpr1 >= zpreclr1, while dpr_clip is zdpr1 > zpreclr1: the two differ only where two independently rounded
//    positive doubles are equal.  The walk counts such cells and the census test asserts there are none.
enum : uint32_t {
  SIG_COLD = 1u << 0, SIG_ESDP_CLIP = 1u << 1, SIG_QLIM_IS_QS = 1u << 2, SIG_BELOW_RTICE = 1u << 3,
  SIG_REGIME_SHIFT = 4,  // two bits: 0 clear, 1 overcast, 2 partial
  SIG_LLO1 = 1u << 6, SIG_LLO3 = 1u << 7, SIG_NEWMAX = 1u << 8, SIG_MELT = 1u << 9, SIG_WARM2 = 1u << 10, SIG_MELT_ALL = 1u << 11,
  SIG_CLOUDY = 1u << 12, SIG_FRZ1 = 1u << 13, SIG_LLO2 = 1u << 14, SIG_DPR_CLIP = 1u << 15, SIG_WARM_ADJ = 1u << 16,
  SIG_A_CLIP0 = 1u << 17, SIG_A_CLIP1 = 1u << 18, SIG_DQ_POS = 1u << 19, SIG_FRZ2 = 1u << 20,
  // derived
  SIG_LAST = 1u << 21, SIG_PARTIAL_MELT = 1u << 22, SIG_REGCL_CAPPED = 1u << 23, SIG_A_CLIP0_DQ = 1u << 24,
  SIG_A_CLIP1_DQ = 1u << 25, SIG_ESDP_CLIP_CLOUD = 1u << 26, SIG_LLO2_DPR_CLIP = 1u << 27,
  SIG_ACTIVE = 1u << 31  // set in every word the walk wrote: the padded tail keeps what the caller put there
};

template <bool P, bool EVAP>
static uint32_t census_word(ConstsP c, const LevelCst& k, const LevelTraj& t) {
  uint32_t w = SIG_ACTIVE;
  auto bit = [&](bool v, uint32_t b) { if (v) w |= b; };
  bit(t.cold, SIG_COLD); bit(t.esdp_clip, SIG_ESDP_CLIP); bit(t.qlim_is_qs, SIG_QLIM_IS_QS); bit(t.below_rtice, SIG_BELOW_RTICE);
  w |= (uint32_t)t.regime << SIG_REGIME_SHIFT;
  bit(t.llo1, SIG_LLO1); bit(t.llo3, SIG_LLO3); bit(t.newmax, SIG_NEWMAX);
  bit(t.melt, SIG_MELT); bit(t.warm2, SIG_WARM2); bit(t.melt_all, SIG_MELT_ALL);
  bit(t.cloudy, SIG_CLOUDY); bit(t.frz1, SIG_FRZ1); bit(t.llo2, SIG_LLO2); bit(t.dpr_clip, SIG_DPR_CLIP);
  bit(t.ztpb > c->k4.v[K4_RTT], SIG_WARM_ADJ);  // the phase of the saturation adjustment (level_forward stage L)
  bit(t.a_clip[0], SIG_A_CLIP0); bit(t.a_clip[1], SIG_A_CLIP1); bit(t.dq_pos, SIG_DQ_POS); bit(t.frz2, SIG_FRZ2);
  bit(k.last, SIG_LAST);
  bit(t.melt && t.zsnmlt > RC(0.0) && !t.melt_all, SIG_PARTIAL_MELT);
  bit(t.regime == 2 && regcl_factor(t.zqpd, t.zqcd, k.zscalm) >= RC(0.3), SIG_REGCL_CAPPED);  // fmin(0.3, .) took the 0.3
  bit(t.a_clip[0] && t.dq_pos, SIG_A_CLIP0_DQ); bit(t.a_clip[1] && t.dq_pos, SIG_A_CLIP1_DQ);
  bit(t.esdp_clip && t.zqc2 > RC(0.0), SIG_ESDP_CLIP_CLOUD);
  bit(t.llo2 && t.dpr_clip, SIG_LLO2_DPR_CLIP);
  return w;
}

// nl_column<F> without the perturbation, the checkpoints, the zero plane, the priorities and the pacing; 64-bit offsets
template <bool P, bool EVAP>
static long long census_column(long long gcol, const NlArgs* a, bool has_qsat, uint32_t* sig) {
  LaneOff o; bool active;
  if (!lane_setup(&a->g, &a->s, gcol, o, active)) return 0;
  if (!active) return 0;
  const int nlev = a->g.nlev, nproma = a->g.nproma;
  const long long osig = (gcol / nproma) * ((long long)nproma * nlev) + (gcol % nproma);
  ConstsP c = C2_CONSTS(a);
  RhCrit rh;
  rhcrit_setup(tropopause<false>(c, a->tab, &a->in, o, &a->g, RC(0.0)), rh);
  const real_t paph_surf = EVAP ? a->in.paph[o.half + (long long)nlev * nproma] : RC(0.0);
  store_top(&a->out, o, c);
  Carry cy; cy.rfl = RC(0.0); cy.sfl = RC(0.0); cy.covptot = RC(0.0);
  real_t paph_k = a->in.paph[o.half];
  long long differ = 0;
  for (int jk = 0; jk < nlev; ++jk) {
    RawLevel cur;
    cur.qsat = RC(0.0);
    if (has_qsat) load_level<true>(&a->in, o, nproma, nlev, jk, cur);
    else load_level<false>(&a->in, o, nproma, nlev, jk, cur);
    if (!has_qsat) cur.qsat = satur_point<P>(c, cur.pap, cur.t);
    LevelCst k;
    level_cst(a->tab, jk, jk == nlev - 1, k);
    LevelIn x;
    make_level_in(cur, paph_k, paph_surf, x);
    LevelTraj tr;
    LevelOut lo;
    level_forward<P, EVAP>(c, k, rh, x, cy, tr, lo);
    store_out(&a->out, o, nproma, jk, lo);
    sig[osig + (long long)jk * nproma] = census_word<P, EVAP>(c, k, tr);
    differ += (tr.dpr_clip != tr.reset);
    paph_k = cur.paph_k1;
  }
  return differ;
}

extern "C" {

// sig: (NBLOCKS, NLEV, NPROMA) words; returns the number of cells where dpr_clip and reset differ (see above), or -1
long long hostcheck_census(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, const cloudsc2_inputs* in,
                           const cloudsc2_outputs* out, uint32_t* sig) {
  if (!prm->lphylin && !prm->ldrain1d) return -1;  // the trajectories of the TL and AD sweeps have the LPHYLIN form only
  NlArgs a;
  a.g = hc_geom(nproma, nlev, ngptot);
  a.c = hc_consts(*prm, ptsphy);
  LevelTab tab; hc_tables(*prm, tab, a.g);
  a.tab = &tab;
  a.s = Strides{0, 0, 0, 0, 0};
  hc_in(*in, a.s, a.in); hc_out(*out, a.s, a.out);
  a.zero_plane = nullptr; a.zero_stride = 0; a.lam = 0.0; a.ckpt = nullptr;
  const bool has_qsat = in->qsat.ptr != nullptr;
  long long differ = 0;
  for (long long gc = 0; gc < a.g.ncols_pad; ++gc) {
    if (g_hc_precise) differ += a.c.evap ? census_column<true, true>(gc, &a, has_qsat, sig) : census_column<true, false>(gc, &a, has_qsat, sig);
    else differ += a.c.evap ? census_column<false, true>(gc, &a, has_qsat, sig) : census_column<false, false>(gc, &a, has_qsat, sig);
  }
  return differ;
}

}  // extern "C"
