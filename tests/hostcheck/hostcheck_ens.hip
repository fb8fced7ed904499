// TEST-ONLY: what the ensemble launchers (cloudsc2_{nl,tl,vjp}_launch_ens) run on the device besides the column sweeps, compiled for
// the HOST: the derivation of a member's constants from its parameter row (ens_consts), the member's argument block
// (ens_member_args) and the workgroup -> (member, column) mapping (ens_locate).  Like hostcheck.hip, never loaded by the package.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/cloudsc2_hip.h"
#include "../../dwarf_p_cloudsc2_tl_ad_amd/csrc/cloudsc2_column.hpp"

using namespace cloudsc2;

static cloudsc2_params with_row(const cloudsc2_params& prm, const double* par) {
  cloudsc2_params p = prm;
  p.rkconv = par[PAR_RKCONV]; p.rclcrit = par[PAR_RCLCRIT]; p.rlptrc = par[PAR_RLPTRC]; p.rpecons = par[PAR_RPECONS];
  return p;
}

template <class Ptrs>
static bool advanced(const Ptrs& got, const Ptrs& base, const long long* stride, long long member) {
  const real_t* const* g = (const real_t* const*)&got;
  const real_t* const* b = (const real_t* const*)&base;
  for (int i = 0; i < (int)(sizeof(Ptrs) / sizeof(void*)); ++i)
    if (g[i] != (b[i] ? b[i] + member * stride[i] : nullptr)) return false;
  return true;
}

static bool same_geom(const Geom& a, const Geom& b) {
  return a.nproma == b.nproma && a.nlev == b.nlev && a.ngptot == b.ngptot && a.ncols_pad == b.ncols_pad && a.kb0 == b.kb0 && a.kb1 == b.kb1 &&
         a.fair == b.fair && a.pace_slots == b.pace_slots && a.pace_first == b.pace_first && a.pace_recip_q16 == b.pace_recip_q16;
}

extern "C" {

int hostcheck_ens_real_bytes(void) { return (int)sizeof(real_t); }

// The device-side derivation against the host's: a Consts made from `prm` and rewritten by ens_consts with the row `par`, against
// make_consts of a parameter block holding that row; the ParLin against make_parlin (dpar may be NULL).  0: the same bytes; bit 0:
// the Consts differ; bit 1: the ParLin differs.
int hostcheck_ens_consts(const cloudsc2_params* prm, double ptsphy, const double* par, const double* dpar) {
  Consts got, want;
  ParLin pgot, pwant;
  memset(&got, 0, sizeof(got)); memset(&want, 0, sizeof(want)); memset(&pgot, 0, sizeof(pgot)); memset(&pwant, 0, sizeof(pwant));
  got = make_consts(*prm, ptsphy);
  ens_consts(got, ptsphy, par, dpar, &pgot);
  want = make_consts(with_row(*prm, par), ptsphy);
  pwant = make_parlin(want, dpar);
  return (memcmp(&got, &want, sizeof(Consts)) ? 1 : 0) | (memcmp(&pgot, &pwant, sizeof(ParLin)) ? 2 : 0);
}

// Member `member`'s argument block of each of the three kinds from a template with recognisable pointers (qsat NULL): every pointer
// advanced by member x its stride, NULL left NULL, the workspace slab of the reverse sweep, the constants those of the row, the geometry,
// strides and table the template's.  0: all of it holds; else the number of the first check that failed.
int hostcheck_ens_member_args(const cloudsc2_params* prm, double ptsphy, const double* par, const double* dpar, int member, int ncols_pad) {
  EnsStrides m;
  for (int i = 0; i < 16; ++i) { m.in[i] = 1000 + 7 * i; m.in2[i] = 3000 + 11 * i; }
  for (int i = 0; i < 10; ++i) { m.out[i] = 2000 + 5 * i; m.out2[i] = 4000 + 3 * i; }
  m.ckpt = 5000;
  m.in[2] = 0;  // (a shared field)
  InPtrs in; OutPtrs out; InPtrsRW rw;
  for (int i = 0; i < 16; ++i) { ((real_t**)&in)[i] = (real_t*)(uintptr_t)(0x100000u * (i + 1)); ((real_t**)&rw)[i] = (real_t*)(uintptr_t)(0x100000u * (i + 40)); }
  for (int i = 0; i < 10; ++i) ((real_t**)&out)[i] = (real_t*)(uintptr_t)(0x100000u * (i + 20));
  in.qsat = nullptr; rw.qsat = nullptr;
  const Consts c0 = make_consts(*prm, ptsphy), ck = make_consts(with_row(*prm, par), ptsphy);
  const ParLin pk = make_parlin(ck, dpar);
  const Geom g = {24, prm->nlev, ncols_pad - 2, ncols_pad, 3, 9, 0};
  real_t* const ckpt = (real_t*)(uintptr_t)0x7000000u;

  NlArgs tn; memset(&tn, 0, sizeof(tn));
  tn.c = c0; tn.g = g; tn.s = Strides{11, 12, 13, 14, 15}; tn.in = in; tn.out = out; tn.tab = (const LevelTab*)(uintptr_t)0x8000000u; tn.ckpt = ckpt;
  NlArgs an; memset(&an, 0xff, sizeof(an));
  ens_member_args(an, tn, m, ptsphy, member, par, dpar);
  if (!advanced(an.in, in, m.in, member) || !advanced(an.out, out, m.out, member)) return 1;
  if (an.ckpt != ckpt + (long long)member * m.ckpt) return 2;
  if (memcmp(&an.c, &ck, sizeof(Consts))) return 3;
  if (!same_geom(an.g, g) || memcmp(&an.s, &tn.s, sizeof(Strides)) || an.tab != tn.tab || an.zero_plane || an.zero_stride || an.lam != 0) return 4;

  TlParArgs tt; memset(&tt, 0, sizeof(tt));
  tt.a.c = c0; tt.a.g = g; tt.a.s = tn.s; tt.a.sp = Strides{21, 22, 23, 24, 25}; tt.a.in = in; tt.a.din = in; tt.a.dout = out; tt.a.tab = tn.tab;
  tt.par = make_parlin(c0, nullptr);
  TlParArgs at; memset(&at, 0xff, sizeof(at));
  ens_member_args(at, tt, m, ptsphy, member, par, dpar);
  if (!advanced(at.a.in, in, m.in, member) || !advanced(at.a.din, in, m.in2, member) || !advanced(at.a.dout, out, m.out2, member)) return 5;
  { OutPtrs none; memset(&none, 0, sizeof(none)); if (memcmp(&at.a.out, &none, sizeof(none))) return 6; }
  if (memcmp(&at.a.c, &ck, sizeof(Consts)) || memcmp(&at.par, &pk, sizeof(ParLin))) return 7;
  if (!same_geom(at.a.g, g) || memcmp(&at.a.s, &tt.a.s, sizeof(Strides)) || memcmp(&at.a.sp, &tt.a.sp, sizeof(Strides)) || at.a.tab != tn.tab ||
      at.a.supsat_inc != 0 || at.a.yy)
    return 8;

  AdParArgs ta; memset(&ta, 0, sizeof(ta));
  ta.a.nl = tn; ta.a.sa = Strides{31, 32, 33, 34, 35}; ta.a.ain = rw; ta.a.aout = out; ta.par = make_parlin(c0, nullptr);
  double* const work = (double*)(uintptr_t)0x9000000u;
  ta.work = work;
  AdParArgs aa; memset(&aa, 0xff, sizeof(aa));
  ens_member_args(aa, ta, m, ptsphy, member, par, nullptr);
  if (!advanced(aa.a.nl.in, in, m.in, member) || !advanced(aa.a.nl.out, out, m.out, member) || aa.a.nl.ckpt != ckpt + (long long)member * m.ckpt) return 9;
  if (!advanced(aa.a.ain, rw, m.in2, member) || !advanced(aa.a.aout, out, m.out2, member)) return 10;
  if (aa.work != work + (long long)member * PAR_COUNT * ncols_pad) return 11;
  const ParLin pr = make_parlin(ck, nullptr);
  if (memcmp(&aa.a.nl.c, &ck, sizeof(Consts)) || memcmp(&aa.par, &pr, sizeof(ParLin))) return 12;
  if (!same_geom(aa.a.nl.g, g) || memcmp(&aa.a.nl.s, &tn.s, sizeof(Strides)) || memcmp(&aa.a.sa, &ta.a.sa, sizeof(Strides)) || aa.a.nl.tab != tn.tab ||
      aa.a.norms || aa.a.gmax)
    return 13;
  return 0;
}

// the workgroup -> (member, column) mapping of the ensemble sweeps for every thread of a launch of `members` x wgs_per_member
// workgroups: member[] and column[] receive members * wgs_per_member * block entries in (workgroup, thread) order
void hostcheck_ens_locate(unsigned members, unsigned wgs_per_member, unsigned block, unsigned* member, long long* column) {
  for (unsigned wg = 0; wg < members * wgs_per_member; ++wg)
    for (unsigned t = 0; t < block; ++t) ens_locate(wg, wgs_per_member, t, block, member[(size_t)wg * block + t], column[(size_t)wg * block + t]);
}

}  // extern "C"
