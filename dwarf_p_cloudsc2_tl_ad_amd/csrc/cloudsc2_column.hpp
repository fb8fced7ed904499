// cloudsc2_column.hpp -- what one GPU lane does for its grid column: the 137-level sweeps of SATUR+CLOUDSC2,
// CLOUDSC2TL and CLOUDSC2AD built from the per-level functions of cloudsc2_level.hpp, and the Taylor test's lambda loop as one
// sweep (taylor_column: lane = (column, lambda)).  The __global__ kernels in cloudsc2_sweep_kernels.hpp are thin wrappers
// (gcol = blockIdx*blockDim + threadIdx) around these functions.
//
// Memory access: lane g reads f[jl + NPROMA*(jk + NLEVx*ibl)] with g = ibl*NPROMA + jl, i.e. consecutive lanes
// read consecutive doubles of every plane -> a wave64 fetches 512 contiguous bytes per plane and level.  Inputs of
// level JK+1 are requested before level JK is evaluated (register double buffer), which is what hides HBM latency
// at the 1-3 waves/SIMD this fp64-heavy code runs at (NL 3, TL and AD 1).
#pragma once
#include <type_traits>

#include "cloudsc2_level.hpp"

#ifndef CLOUDSC2_MAX_NLEV
#define CLOUDSC2_MAX_NLEV 200
#endif

namespace cloudsc2 {

// per-level, column-independent tables (device copy)
struct LevelTab {
  struct { real_t ceta, zscalm; } lev[CLOUDSC2_MAX_NLEV];  // interleaved: one 16-byte scalar load per level
};

struct Geom {
  int nproma, nlev, ngptot;
  long long ncols_pad;  // NBLOCKS*NPROMA
  int kb0, kb1;         // tropopause band [kb0,kb1): levels that can satisfy 0.1 < CETA < 0.4 (cloudsc2.F90:320)
  int fair;             // NL: the waves of a SIMD yield to each other by progress (progress_priority); set by the launcher
  // TL / AD: pacing of a launch of a few partial rounds of workgroups (struct Pace below); pace_recip_q16 = 0: off
  int pace_slots = 0, pace_first = 0, pace_recip_q16 = 0;
};

// Fields are grouped by the stride between NPROMA blocks.  `full` = (NPROMA,NLEV,NBLOCKS) arrays,
// `half` = (NPROMA,NLEV+1,NBLOCKS), `cml` = PGTEN* planes of B_CML, `clv` = PL/PI planes of PCLV,
// `loc` = PTEN* planes of B_LOC.  The launchers check that every field of a group has the group's stride.
struct Strides {
  long long full, half, cml, clv, loc;
};

struct InPtrs {
  const real_t *paph, *pap, *q, *qsat, *t, *l, *i, *lude, *lu, *mfu, *mfd, *gt, *gq, *gl, *gi, *supsat;
};
struct OutPtrs {
  real_t *tent, *tenq, *tenl, *teni, *clc, *fplsl, *fplsn, *fhpsl, *fhpsn, *covptot;
};
struct InPtrsRW {
  real_t *paph, *pap, *q, *qsat, *t, *l, *i, *lude, *lu, *mfu, *mfd, *gt, *gq, *gl, *gi, *supsat;
};

// Kernel argument blocks.  Each kernel takes exactly one of these by value; on the device the column functions read
// it in place from the kernel-argument segment through a constant-address-space pointer (see C2_LAUNDER).
struct NlArgs {
  Consts c; Geom g; Strides s; InPtrs in; OutPtrs out; const LevelTab* tab;
  real_t* zero_plane; long long zero_stride; real_t lam;
  real_t* ckpt;  // CKPT + EVAP kernels only: (NPROMA,NLEV,NBLOCKS) plane receiving the precipitation cover carried INTO each
                 // level.  Without the evaporation branch the carried cover feeds nothing but itself (level_forward stage G/J:
                 // covpclr is only read under llo2; level_ad: its adjoint stays zero), so it is neither stored nor re-read.
};
struct TlArgs {
  Consts c; Geom g; Strides s, sp; InPtrs in; OutPtrs out; InPtrs din; OutPtrs dout; const LevelTab* tab;
  real_t supsat_inc;  // C2F_SELFINC: the PSUPSAT increment is supsat_inc*PSUPSAT (0.01 in the Taylor test, 0 in the adjoint test)
  double* yy;         // C2F_SELFINC: NULL, or (ncols_pad) doubles receiving <y,y> of each column's TL outputs (the adjoint test's norm1)
};
// The adjoint's trajectory pass IS the NL sweep (with carry checkpoints, nl.ckpt = the scratch plane), so its
// argument block embeds the NL one.
struct AdArgs {
  NlArgs nl; Strides sa; InPtrsRW ain; OutPtrs aout;
  double* norms;  // C2F_ADNORM: (3, ncols_pad) doubles: norm1 (read), norm2 and norm3 (written)
  double* gmax;   // C2F_ADNORM: one double, raised to the largest |norm3| (the kernel's wave maxima, atomically)
};
// C2F_PARLIN: the sweep's own block first (tl_column / ad_reverse_column take a pointer to it and step on to what follows)
struct TlParArgs {
  TlArgs a; ParLin par;
};
struct AdParArgs {
  AdArgs a; ParLin par;
  double* work;  // (PAR_COUNT, ncols_pad) doubles: every active lane's parameter adjoints (the padded tail is not written)
};
typedef const C2_CONST_AS NlArgs* NlArgsP;
typedef const C2_CONST_AS TlArgs* TlArgsP;
typedef const C2_CONST_AS AdArgs* AdArgsP;
typedef const C2_CONST_AS TlParArgs* TlParArgsP;
typedef const C2_CONST_AS AdParArgs* AdParArgsP;
typedef const C2_CONST_AS InPtrs* InPtrsP;
typedef const C2_CONST_AS OutPtrs* OutPtrsP;
typedef const C2_CONST_AS InPtrsRW* InPtrsRWP;
typedef const C2_CONST_AS LevelTab* LevelTabP;
typedef const C2_CONST_AS Geom* GeomP;
typedef const C2_CONST_AS Strides* StridesP;

// Perturbed-parameter ensembles (cloudsc2_{nl,tl,vjp}_launch_ens): K members, each with an argument block of its own in DEVICE
// MEMORY -- NlArgs, TlParArgs or AdParArgs, the column functions read it through the same constant-address-space pointer -- which
// ens_args_kernel derives from one template block (the host's, built from the caller's parameter block with the base pointers): every
// pointer advanced by member x that field's member stride (elements; 0: the members share the field), the constants from the member's
// row of the (K, 4) parameter array (ens_consts).
struct EnsStrides {
  long long in[16], out[10];    // the trajectory's inputs and outputs, in the order of InPtrs / OutPtrs
  long long in2[16], out2[10];  // TL: the input and output tangents; reverse sweep: the input and output adjoints
  long long ckpt;               // the cover-checkpoint plane
};
static_assert(sizeof(InPtrs) == 16 * sizeof(void*) && sizeof(InPtrsRW) == sizeof(InPtrs) && sizeof(OutPtrs) == 10 * sizeof(void*),
              "the pointer blocks are arrays of 16 / 10 pointers");
template <class Ptrs>
C2_HD void ens_advance_ptrs(Ptrs& p, const long long* stride, long long member) {
  real_t** q = (real_t**)&p;
  for (int i = 0; i < (int)(sizeof(Ptrs) / sizeof(void*)); ++i)
    if (q[i]) q[i] += member * stride[i];
}
C2_HD void ens_advance(NlArgs& a, const EnsStrides& m, long long member) {
  ens_advance_ptrs(a.in, m.in, member);
  ens_advance_ptrs(a.out, m.out, member);
  if (a.ckpt) a.ckpt += member * m.ckpt;
}
C2_HD void ens_advance(TlParArgs& a, const EnsStrides& m, long long member) {
  ens_advance_ptrs(a.a.in, m.in, member);
  ens_advance_ptrs(a.a.din, m.in2, member);
  ens_advance_ptrs(a.a.dout, m.out2, member);
}
C2_HD void ens_advance(AdParArgs& a, const EnsStrides& m, long long member) {  // (work: one (PAR_COUNT, ncols_pad) slab per member)
  ens_advance(a.a.nl, m, member);
  ens_advance_ptrs(a.a.ain, m.in2, member);
  ens_advance_ptrs(a.a.aout, m.out2, member);
  a.work += member * (long long)PAR_COUNT * a.a.nl.g.ncols_pad;
}
C2_HD Consts& ens_consts_of(NlArgs& a) { return a.c; }
C2_HD Consts& ens_consts_of(TlParArgs& a) { return a.a.c; }
C2_HD Consts& ens_consts_of(AdParArgs& a) { return a.a.nl.c; }
C2_HD ParLin* ens_parlin_of(NlArgs&) { return nullptr; }
C2_HD ParLin* ens_parlin_of(TlParArgs& a) { return &a.par; }
C2_HD ParLin* ens_parlin_of(AdParArgs& a) { return &a.par; }
// member `member`'s block from the template: what thread `member` of ens_args_kernel stores (dpar: the member's four parameter
// tangents, or NULL)
template <class Args>
C2_HD void ens_member_args(Args& a, const Args& tmpl, const EnsStrides& m, double ptsphy, long long member, const double* par,
                           const double* dpar) {
  a = tmpl;
  ens_advance(a, m, member);
  ens_consts(ens_consts_of(a), ptsphy, par, dpar, ens_parlin_of(a));
}
// The ensemble sweeps' grid is members x wgs_per_member workgroups of `block` threads: workgroup b works for member b / wgs_per_member
// on that member's columns from (b mod wgs_per_member) x block on (a member's last workgroup may be partly idle; no wave spans two members).
C2_HD void ens_locate(unsigned wg, unsigned wgs_per_member, unsigned thread, unsigned block, unsigned& member, long long& column) {
  member = wg / wgs_per_member;
  column = (long long)(wg - member * wgs_per_member) * block + thread;
}
// The NL column-sum sweep of an ensemble locates its workgroups itself (`wgs`: the grid).  Member-major like ens_locate.  The
// member-interleaved order -- member = wg mod members, column = (wg / members) x block + thread, so that the members' re-reads of a shared
// state meet in the Infinity Cache -- was measured: equal within the spread at 8 members, 7 % faster at 32, identical bits; it had to
// win at both to be kept (profiles/EXPERIMENTS.md, "Ensemble column sums: workgroup order").
C2_HD void ens_colsum_locate(unsigned wg, unsigned wgs_per_member, [[maybe_unused]] unsigned wgs, unsigned thread, unsigned block,
                             unsigned& member, long long& column) {
  ens_locate(wg, wgs_per_member, thread, block, member, column);
}

// Per-lane offsets of the column inside each layout group.  LaneOff: element offsets (64 bit).  LaneOff32: BYTE offsets
// in 32 bits, usable when every buffer is smaller than 4 GiB (C2F_OFF32): the accesses then take the
// `global_load v, v_off32, s[base]` form -- no 64-bit address arithmetic per access, half the offset registers.
template <class OT>
struct LaneOffT {
  OT full, half, cml, clv, loc;
};
typedef LaneOffT<long long> LaneOff;
typedef LaneOffT<unsigned> LaneOff32;
// offset of level jk / of one level row, in the units of the offset type
C2_HD long long level_off(long long, int jk, int nproma) { return (long long)jk * nproma; }
C2_HD unsigned level_off(unsigned, int jk, int nproma) { return (unsigned)jk * (unsigned)nproma * (unsigned)sizeof(real_t); }
C2_HD long long row_off(long long, int nproma) { return nproma; }
C2_HD unsigned row_off(unsigned, int nproma) { return (unsigned)nproma * (unsigned)sizeof(real_t); }

// element offsets -> the offset type of a kernel variant (bytes for LaneOff32)
template <class OT>
C2_HD LaneOffT<OT> lane_off_as(const LaneOff& o) {
  const long long m = sizeof(OT) == 4 ? (long long)sizeof(real_t) : 1;
  LaneOffT<OT> r;
  r.full = (OT)(o.full * m); r.half = (OT)(o.half * m); r.cml = (OT)(o.cml * m); r.clv = (OT)(o.clv * m); r.loc = (OT)(o.loc * m);
  return r;
}

C2_HD bool lane_setup(GeomP g, StridesP s, long long gcol, LaneOff& o, bool& active) {
  if (gcol >= g->ncols_pad) return false;
  long long ibl = gcol / g->nproma;
  long long jl = gcol - ibl * g->nproma;
  o.full = ibl * s->full + jl;
  o.half = ibl * s->half + jl;
  o.cml = ibl * s->cml + jl;
  o.clv = ibl * s->clv + jl;
  o.loc = ibl * s->loc + jl;
  active = gcol < g->ngptot;
  return true;
}

// Everything level jk needs from the input planes EXCEPT PAPHP1(JK), which is the previous level's PAPHP1(JK+1):
// the 14 full-level planes at jk plus the two look-ahead values PAPHP1(JK+1) and PLU(JK+1) (cloudsc2.F90:272,435).
// Loading the look-ahead values together with the level they belong to lets the whole set be requested one full
// level ahead of its use.
struct RawLevel {
  real_t paph_k1, pap, q, qsat, t, l, i, lude, lu_k1, mfu, mfd, gt, gq, gl, gi, supsat;
};

// Streaming accesses: every plane element is read once and written once per launch.  On the device they are
// non-temporal (`nt`), so they do not displace the little that is re-read (tropopause band, level tables); the host builds
// of these headers take plain accesses.
C2_HD real_t ldg(const real_t* p, long long i) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_nontemporal_load(p + i);
#else
  return p[i];
#endif
}
C2_HD void stg(real_t* p, long long i, real_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_nontemporal_store(v, p + i);
#else
  p[i] = v;
#endif
}

C2_HD real_t ldg(const real_t* p, unsigned byte_off) {
  const real_t* q = (const real_t*)((const char*)p + byte_off);
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_nontemporal_load(q);
#else
  return *q;
#endif
}
C2_HD void stg(real_t* p, unsigned byte_off, real_t v) {
  real_t* q = (real_t*)((char*)p + byte_off);
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_nontemporal_store(v, q);
#else
  *q = v;
#endif
}

// STREAM = false: plain loads for data that other waves read too (the Taylor sweep, whose waves share cache lines)
template <bool STREAM>
C2_HD real_t ldx(const real_t* p, long long i) { return STREAM ? ldg(p, i) : p[i]; }
template <bool STREAM>
C2_HD real_t ldx(const real_t* p, unsigned byte_off) { return STREAM ? ldg(p, byte_off) : *(const real_t*)((const char*)p + byte_off); }

template <bool HAS_QSAT, class OT, bool STREAM = true>
C2_HD void load_level(InPtrsP pp, const LaneOffT<OT>& o, int nproma, int nlev, int jk, RawLevel& r) {
  const InPtrs p = *pp;
  const OT d = level_off(OT(), jk, nproma), d1 = d + row_off(OT(), nproma);
  r.paph_k1 = ldx<STREAM>(p.paph, o.half + d1);
  r.lu_k1 = (jk + 1 < nlev) ? ldx<STREAM>(p.lu, o.full + d1) : RC(0.0);
  r.pap = ldx<STREAM>(p.pap, o.full + d);
  r.q = ldx<STREAM>(p.q, o.full + d);
  r.t = ldx<STREAM>(p.t, o.full + d);
  r.l = ldx<STREAM>(p.l, o.clv + d);
  r.i = ldx<STREAM>(p.i, o.clv + d);
  r.lude = ldx<STREAM>(p.lude, o.full + d);
  r.mfu = ldx<STREAM>(p.mfu, o.full + d);
  r.mfd = ldx<STREAM>(p.mfd, o.full + d);
  r.gt = ldx<STREAM>(p.gt, o.cml + d);
  r.gq = ldx<STREAM>(p.gq, o.cml + d);
  r.gl = ldx<STREAM>(p.gl, o.cml + d);
  r.gi = ldx<STREAM>(p.gi, o.cml + d);
  r.supsat = ldx<STREAM>(p.supsat, o.full + d);
  if (HAS_QSAT) r.qsat = ldx<STREAM>(p.qsat, o.full + d);
}

// Perturbed state of the Taylor test: x5 = x + lambda*(0.01*x) (cloudsc_driver_tl_mod.F90:156-171,200-215).
C2_HD real_t pert(real_t x, real_t lam) { return x + lam * (x * RC(0.01)); }

C2_HD void perturb_raw(RawLevel& r, real_t lam) {
  r.paph_k1 = pert(r.paph_k1, lam);
  r.pap = pert(r.pap, lam); r.q = pert(r.q, lam); r.qsat = pert(r.qsat, lam); r.t = pert(r.t, lam);
  r.l = pert(r.l, lam); r.i = pert(r.i, lam); r.lude = pert(r.lude, lam); r.lu_k1 = pert(r.lu_k1, lam);
  r.mfu = pert(r.mfu, lam); r.mfd = pert(r.mfd, lam); r.gt = pert(r.gt, lam); r.gq = pert(r.gq, lam);
  r.gl = pert(r.gl, lam); r.gi = pert(r.gi, lam); r.supsat = pert(r.supsat, lam);
}

C2_HD void make_level_in(const RawLevel& cur, real_t paph_k, real_t paph_surf, LevelIn& x) {
  x.paph_k = paph_k; x.paph_k1 = cur.paph_k1;
  x.pap = cur.pap; x.q = cur.q; x.qs = cur.qsat; x.t = cur.t; x.l = cur.l; x.i = cur.i;
  x.lude = cur.lude; x.lu_k1 = cur.lu_k1; x.mfu = cur.mfu; x.mfd = cur.mfd;
  x.gt = cur.gt; x.gq = cur.gq; x.gl = cur.gl; x.gi = cur.gi; x.supsat = cur.supsat;
  x.paph_surf = paph_surf;
}

// The carries above the model top (cloudsc2.F90:305-312), the carried tangents there and the carried adjoints below the surface.  (A
// macro: as a function, returning by value or filling a reference, it changed the instruction order of the batched and the parameter
// sweeps, whose per-direction carries are arrays -- profiles/EXPERIMENTS.md, "Reverse sweeps: a level's loads and adjoint stores once".)
#define C2_ZERO_CARRY(cy) ((cy).rfl = RC(0.0), (cy).sfl = RC(0.0), (cy).covptot = RC(0.0))

// Tropopause pre-scan (cloudsc2.F90:315-326): the last band level whose first-guess T exceeds the one below.
// The band is ~40 levels; its 2 x 40 loads are requested in batches of kTropBatch levels -- one HBM latency per
// batch instead of one per level at the start of every wave.
constexpr int kTropBatch = 16;
template <bool PERT>
C2_HD real_t tropopause(ConstsP c, LevelTabP tab, InPtrsP p, const LaneOff& o, GeomP g, real_t lam) {
  real_t ztrpaus = RC(0.1);
  const int kb0 = g->kb0, kb1 = g->kb1, nproma = g->nproma;
  if (kb1 > kb0) {
    const real_t ptsphy = c->ptsphy;
    const real_t* pt = p->t;
    const real_t* pg = p->gt;
    long long d = (long long)kb0 * nproma;
    real_t t0 = pt[o.full + d], g0 = pg[o.cml + d];
    if (PERT) { t0 = pert(t0, lam); g0 = pert(g0, lam); }
    real_t tup = t0 + ptsphy * g0;
    for (int jb = kb0; jb < kb1; jb += kTropBatch) {
      real_t tb[kTropBatch], gb[kTropBatch];
#pragma unroll
      for (int u = 0; u < kTropBatch; ++u) {
        const int jk1 = (jb + u + 1 < kb1) ? jb + u + 1 : kb1;  // clamped: level kb1 <= nlev-1 always exists
        const long long d1 = (long long)jk1 * nproma;
        tb[u] = pt[o.full + d1];
        gb[u] = pg[o.cml + d1];
      }
#pragma unroll
      for (int u = 0; u < kTropBatch; ++u) {
        const int jk = jb + u;
        if (jk < kb1) {
          real_t t1 = tb[u], g1 = gb[u];
          if (PERT) { t1 = pert(t1, lam); g1 = pert(g1, lam); }
          const real_t tdn = t1 + ptsphy * g1;
          const real_t ce = tab->lev[jk].ceta;
          if (ce > RC(0.1) && ce < RC(0.4) && tup > tdn) ztrpaus = ce;
          tup = tdn;
        }
      }
    }
  }
  return ztrpaus;
}

// All ten output pointers must be valid (the launchers substitute nothing: a skipped trajectory store is a
// template flag of the TL kernel) -- no per-pointer branches, the pointer block is read with two wide scalar loads.
template <class OT>
C2_HD void store_out(OutPtrsP pp, const LaneOffT<OT>& o, int nproma, int jk, const LevelOut& v) {
  const OutPtrs p = *pp;
  const OT d = level_off(OT(), jk, nproma);
  stg(p.tent, o.loc + d, v.tent);
  stg(p.tenq, o.loc + d, v.tenq);
  stg(p.tenl, o.loc + d, v.tenl);
  stg(p.teni, o.loc + d, v.teni);
  stg(p.clc, o.full + d, v.clc);
  stg(p.covptot, o.full + d, v.covptot);
  const OT d1 = d + row_off(OT(), nproma);
  stg(p.fplsl, o.half + d1, v.fplsl);
  stg(p.fplsn, o.half + d1, v.fplsn);
  stg(p.fhpsl, o.half + d1, v.fhpsl);
  stg(p.fhpsn, o.half + d1, v.fhpsn);
}

C2_HD void store_top(OutPtrsP p, const LaneOff& o, ConstsP c) {
  // fluxes at the model top are zero (cloudsc2.F90:308-309); enthalpy fluxes -0*RLVTT (:732-733)
  const real_t z = RC(0.0);
  p->fplsl[o.half] = z;
  p->fplsn[o.half] = z;
  p->fhpsl[o.half] = -z * c->rlvtt;
  p->fhpsn[o.half] = -z * c->rlstt;
}

C2_HD void level_cst(LevelTabP tab, int jk, bool last, LevelCst& k) {
  k.ceta = tab->lev[jk].ceta;
  k.zscalm = tab->lev[jk].zscalm;
  k.last = last;
  C2_PIN2(k.ceta, k.zscalm);
}

// Pacing of the TL / AD sweeps when a launch is a few PARTIAL rounds of workgroups (round 4; profiles/EXPERIMENTS.md section 7).
// 160 000 columns are 1250 workgroups on 512 workgroup slots (256 CUs x 4 SIMDs at one wave per SIMD, two waves per workgroup): 226
// slots process three workgroups, 286 two, and the launch lasts as long as the three -- the third alone on a machine the others have
// left, at a lone wave's latency-bound pace.  While all slots are busy the memory system is saturated and every wave is slowed alike,
// but only the three-workgroup slots are on the critical path.  With in-order dispatch the workgroups that will share a slot with
// k others (instead of k - 1) are known in advance: position p = blockIdx mod slots of a round is in the FAST class if
// p < (workgroups mod slots).  The others nap at every level for 1/k of the time the level took them: their slot then needs the time
// of k + 1 unpaced workgroups for its k, they leave their share of the bandwidth to the fast class, and both classes end together
// (TL at 160 000 columns: 1.65 -> 1.57 ms, AD 3.01 -> 2.83 ms).  The nap is measured, not tabulated: it follows the clock, the
// variant and the contention by itself.
// How many waves of a launch share a SIMD (observed dispatch of two-wave workgroups on gfx950, profiles/EXPERIMENTS.md "What the
// dispatcher does", checked wave by wave with tools/wave_times.py: 2500 of 2500 in 5 of 5 launches): workgroup i runs on CU
// i mod #CUs; inside a CU the waves of its consecutive workgroups go to the SIMDs in the cyclic order 0,2 | 2,1 | 1,3 | 3,0, whatever
// SIMD the CU starts with -- so wave m of a CU (m = 2 x (i / #CUs) + its index in its workgroup) shares its SIMD with exactly the
// waves m' of that CU with the same ((m' + 1) / 2) mod 4.  `wgs_on_cu` workgroups on the CU; `mine`: waves on this wave's SIMD,
// `most`: on the CU's fullest SIMD.
C2_HD void simd_population(unsigned wgs_on_cu, unsigned j, unsigned wave_in_wg, unsigned& mine, unsigned& most) {
  unsigned pop[4] = {0u, 0u, 0u, 0u};
  for (unsigned k = 0; k < 2u * wgs_on_cu; ++k) pop[((k + 1u) >> 1) & 3u] += 1u;
  const unsigned m = 2u * j + wave_in_wg;
  mine = pop[((m + 1u) >> 1) & 3u];
  most = pop[0];
  for (int g = 1; g < 4; ++g) most = pop[g] > most ? pop[g] : most;
}

// Pace: state of one wave (wave-uniform scalars); begin() before the level loop, nap() once per level with the next loads in flight.
struct Pace {
  unsigned recip_q16 = 0;  // 65536 / k for the slow class, 0 = this workgroup does not nap
  unsigned mark = 0;       // shader clock (low 32 bits) when the previous nap ended
  C2_HD void begin(GeomP g) {
#if defined(__HIP_DEVICE_COMPILE__)
    const unsigned r = (unsigned)g->pace_recip_q16;
    if (r == 0) return;
    unsigned b = blockIdx.x;
    const unsigned s = (unsigned)g->pace_slots;
    while (b >= s) b -= s;  // (at most eight rounds: the launcher paces short launches only)
    if (b >= (unsigned)g->pace_first) { recip_q16 = r; mark = (unsigned)__builtin_amdgcn_s_memtime(); }
#else
    (void)g;
#endif
  }
  // One-round NL launch (g.fair & 4): inside the CUs the launch ends with -- those that carry the most workgroups -- the waves on SIMDs
  // that carry fewer waves than the CU's fullest SIMD nap a share of every level (the CU's memory pipeline is shared by its four
  // SIMDs: what the lighter ones leave, the fuller ones get).  Which SIMD a wave shares with how many others follows from blockIdx
  // alone (simd_population below); 160 000 columns: -2.1 % (profiles/r04_nl_light_ab.txt).
  C2_HD void begin_light(GeomP g) {
#if defined(__HIP_DEVICE_COMPILE__)
    const unsigned cus = (unsigned)g->pace_slots, q = (unsigned)g->pace_first, r = (unsigned)g->fair >> 8;
    unsigned c = blockIdx.x, j = 0;
    while (c >= cus) { c -= cus; ++j; }
    if (r != 0u && c >= r) return;  // only inside the CUs that carry the most workgroups: the launch ends with them
    unsigned mine, most;
    simd_population(q + (r != 0u ? 1u : 0u), j, (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), mine, most);
    if (mine < most) { recip_q16 = (unsigned)g->pace_recip_q16; mark = (unsigned)__builtin_amdgcn_s_memtime(); }
#else
    (void)g;
#endif
  }
  C2_HD void nap() {
#if defined(__HIP_DEVICE_COMPILE__)
    if (recip_q16 == 0) return;
    const unsigned work = (unsigned)__builtin_amdgcn_s_memtime() - mark;             // clocks since the previous nap ended
    const unsigned naps = (unsigned)(((unsigned long long)work * recip_q16) >> 22);    // work / k, in units of 64 clocks
    for (unsigned i = 0; i < naps && i < 512u; ++i) __builtin_amdgcn_s_sleep(1);
    mark = (unsigned)__builtin_amdgcn_s_memtime();
#endif
  }
};

// Compile-time variant flags of the column sweeps (template argument F of the functions below and of the kernels)
enum : unsigned {
  C2F_QSAT = 1u,     // PQSAT is an input (otherwise SATUR is evaluated in the sweep)
  C2F_PRECISE = 2u,  // IEEE divisions / libm transcendentals in reference operation order
  C2F_EVAP = 4u,     // LEVAPLS2 .OR. LDRAIN1D
  C2F_PERT = 8u,     // NL only: inputs perturbed by lambda*0.01*x (Taylor test)
  C2F_CKPT = 16u,    // NL only: trajectory pass of the adjoint (carry checkpoints)
  C2F_TRAJ = 8u,     // TL only: trajectory outputs are stored
  C2F_SELFINC = 16u, // TL only: the increments are 0.01*x of the trajectory inputs themselves, as in both test drivers
                     // (cloudsc_driver_tl_mod.F90:156-171, cloudsc_driver_ad_mod.F90:124-139): no perturbation inputs are read
  C2F_ASSIGN = 8u,   // AD only: the input adjoints are ASSIGNED (x = A^T y) instead of accumulated (x += A^T y): their old
                     // values are neither read nor needed to be zero (the adjoint test zeroes them first, cloudsc_driver_ad_mod.F90:198-213)
  C2F_ADNORM = 16u,  // AD reverse sweep, assign form only: the adjoint test's <x, x_adj> and norm3 are formed in the sweep
                     // (cloudsc_driver_ad_mod.F90:240-264) instead of re-reading the 32 planes afterwards
  C2F_OFF32 = 32u,   // every buffer of the launch < 4 GiB: 32-bit byte offsets (LaneOff32)
  C2F_NOLIN = 64u,   // NL only: .NOT.(LPHYLIN .OR. LDRAIN1D), the FOEALFA / FOEEWM form of stage A (cloudsc2.F90:365-369)
  C2F_VJP = 64u,     // AD reverse sweep, assign form only (never with ADNORM): the vector-Jacobian product of the NL sweep
                     // (cloudsc2_vjp_launch): the output adjoints are only read (not zeroed) and the PSUPSAT adjoint is the true
                     // derivative zqp1 instead of the reference's PTSPHY*zqp1 (cloudsc2ad.F90:1733 vs cloudsc2tl.F90:345).
                     // It shares its bit with NOLIN: the fused ad_kernel, which hands its flags on to nl_column, never takes it.
  C2F_SATLIN = 128u, // TL (without TRAJ / SELFINC) and the VJP form of the reverse sweep, never with QSAT: SATUR is differentiated
                     // inside the sweep (satur_lin_point).  The tangent of qsat is dqs/dpap dpap + dqs/dt dt instead of an input plane,
                     // its adjoint is folded into those of pap and t instead of being stored: no qsat plane on either side
                     // (cloudsc2_tl_launch_satur, cloudsc2_vjp_launch_satur)
  C2F_PARLIN = 256u, // TL (without TRAJ / SELFINC) and the VJP form of the reverse sweep, each with QSAT or with SATLIN: the derivative
                     // with respect to RKCONV, RCLCRIT, RLPTRC, RPECONS (struct ParLin).  The argument block is TlParArgs / AdParArgs.
                     // TL: four parameter tangents add their source terms.  Reverse sweep: the lane sums its column's contributions
                     // in four doubles and stores them to the launch's workspace, which a second kernel folds in a fixed order
                     // (cloudsc2_tl_launch_par, cloudsc2_vjp_launch_par; kernels: the units tl_par, vjp_par)
  C2F_SPARSE = 512u, // TL (without TRAJ / SELFINC; with PARLIN only as C2F_MEMBER says) and the VJP form of the reverse sweep, each with QSAT or with
                     // SATLIN: only the planes of the launch's two bit masks are moved (struct SparseMasks below).  The argument block is
                     // TlSparseArgs / AdSparseArgs (cloudsc2_tl_launch_sparse, cloudsc2_vjp_launch_sparse; kernels:
                     // the units tl_sparse, vjp_sparse).  Off in every other instantiation.
  C2F_COLSUM = 1024u, // NL (LPHYLIN form, never with PERT; with CKPT: the two flux planes and the cover checkpoint are kept), TL and the
                     // reverse sweep (both with SPARSE): an output is not a plane but its per-column weighted level sum (struct ColsumTab
                     // below).  NL / TL fold the level's outputs into accumulators and store one row per sum after the last level; the
                     // reverse sweep forms the cotangent of a level as weight x the column's sum cotangent.  The argument block is
                     // NlColsumArgs / TlColsumArgs / AdColsumArgs (cloudsc2_{nl,tl,vjp}_launch_colsum; kernels:
                     // the units {nl,tl,vjp}_colsum).  Off in every other instantiation.
  C2F_MEMBER = 2048u, // NL and TL with COLSUM: the column belongs to a member of an ensemble, so it is not the grid's global column; the lane
                     // keeps it in an LDS slot for the store of the sums after the level loop (ColsumAcc).  The TL and the reverse sweep of
                     // an ensemble's column sums are SPARSE | COLSUM | PARLIN: the parameter tangents add their source terms while absent
                     // field tangents are opaque zeros; the parameter adjoints are summed while the gradient planes are stored under the
                     // write mask, which may be empty.  The argument block is NlColsumArgs / TlEnsColsumArgs / AdEnsColsumArgs
                     // (cloudsc2_{nl,tl,vjp}_launch_ens_colsum; kernels: the units {nl,tl,vjp}_ens_colsum).
  C2F_PARMAP = 4096u, // NL (LPHYLIN form, never with PERT or COLSUM), TL and the reverse sweep (both with PARLIN, never with SPARSE): RKCONV,
                     // RCLCRIT, RLPTRC, RPECONS are not constants of the launch but (nblocks, nproma) maps.  Before the level loop the lane
                     // loads its four doubles (and, TL, its four tangents) from a (PAR_COUNT, ncols_pad) table and derives its constants
                     // (lane_consts); the level functions take them in place of the launch's (LanePar).  The reverse sweep stores the
                     // lane's four adjoints to a table of that layout, which is the result: there is no fold.  The argument block is
                     // NlParmapArgs / TlParmapArgs / AdParmapArgs (cloudsc2_{nl,tl,vjp}_launch_parmap; kernels: cloudsc2_parmap.hip).
};

// C2F_PARMAP: the sweep's own block first, then the tables -- (PAR_COUNT, ncols_pad) doubles indexed by padded column -- and the
// time step as make_consts was given it (Consts::ptsphy is its real_t rounding)
struct NlParmapArgs {
  NlArgs a; const double* par; double ptsphy;
};
struct TlParmapArgs {
  TlArgs a; const double* par; const double* dpar; double ptsphy;
};
struct AdParmapArgs {
  AdArgs a; const double* par; double* apar; double ptsphy;  // apar: assigned in every active column
};
typedef const C2_CONST_AS NlParmapArgs* NlParmapArgsP;
typedef const C2_CONST_AS TlParmapArgs* TlParmapArgsP;
typedef const C2_CONST_AS AdParmapArgs* AdParmapArgsP;
// the lane's constants from its column of the table(s); dpar may be NULL
C2_HD void lane_load(LanePar& lp, ConstsP c, double ptsphy, const double* par, const double* dpar, long long np, long long gcol) {
  double v[PAR_COUNT], dv[PAR_COUNT];
#pragma unroll
  for (int i = 0; i < PAR_COUNT; ++i) {
    v[i] = par[i * np + gcol];
    dv[i] = dpar ? dpar[i * np + gcol] : 0.0;
  }
  lane_consts(lp, c->evap, c->lregcl, ptsphy, v, dpar ? dv : nullptr);
}

// Waves per SIMD a sweep is built for, from its flag word: the kernels' launch bounds, the priority code of tl_column and the launchers'
// choice between keeping a launch's waves abreast and pacing it all read it here (cloudsc2_sweep_kernels.hpp says what was measured).
// NL (every kernel over nl_column alone): three without the evaporation branch, which fit 168 VGPRs; the others take what they need.
constexpr int nl_waves_per_simd(unsigned f) { return (f & C2F_EVAP) ? 1 : 3; }
// TL (every kernel over tl_column): three in fp32 with 32-bit offsets and without the evaporation branch, one otherwise -- all of fp64.
constexpr int tl_waves_per_simd(unsigned f) { return (sizeof(real_t) == 4 && (f & C2F_OFF32) && !(f & C2F_EVAP)) ? 3 : 1; }

// ---------------------------------------------------------------------------------------------------------
// Sparse sweeps (C2F_SPARSE): presence of a plane is a property of the LAUNCH
// ---------------------------------------------------------------------------------------------------------
// A loss that touches two outputs and wants two gradients moves 4 of the 26 derivative planes.  The launcher puts two bit masks into the
// argument block, one bit per field in the order of cloudsc2_fields.hpp (= the member order of InPtrs / OutPtrs):
//   TL:             rd over the 16 input tangents (absent: a zero tangent, not read), wr over the 10 output tangents (absent: not stored)
//   reverse sweep:  rd over the 10 output adjoints (absent: a zero cotangent, not read), wr over the 16 input adjoints (absent: not stored)
// The masks are kernel arguments, so every test of a bit is wave-uniform: a scalar branch around the access, no lane diverges.  An absent
// plane's pointer is NULL and is only ever used under its bit.  Contract: every present plane has the bits of the dense sweep given zero
// planes for the absent ones.  That takes two things (launder_level below says what the compiler does otherwise):
//   - the zero of an absent plane is opaque (opaque_zero: an empty asm statement per value), so the level is not specialised on it;
//   - a value that is stored under a bit is pinned before the branch (C2_PIN_V: an empty asm statement that only READS it), so the
//     arithmetic that feeds it stays in the level's straight line instead of sinking into the conditional block, where it would
//     contract differently.  The pin must not redefine the value (as C2_LAUNDER_V does): in the fp32 build that keeps the SLP vectoriser
//     from packing what it packs in the dense sweep, and other products fuse.
// (The host builds, compiled without contraction, need neither.)
#if defined(__HIP_DEVICE_COMPILE__)
#define C2_LAUNDER_V(x) asm volatile("" : "+v"(x))
#define C2_PIN_V(x) asm volatile("" : : "v"(x))  // a use in this block, no new value: what feeds x is not sunk past here
#else
#define C2_LAUNDER_V(x) ((void)0)
#define C2_PIN_V(x) ((void)0)
#endif
struct SparseMasks {
  unsigned rd, wr;
};
enum : unsigned {  // bits of a mask over the 16 inputs
  C2I_PAPH = 1u << 0, C2I_PAP = 1u << 1, C2I_Q = 1u << 2, C2I_QSAT = 1u << 3, C2I_T = 1u << 4, C2I_L = 1u << 5, C2I_I = 1u << 6,
  C2I_LUDE = 1u << 7, C2I_LU = 1u << 8, C2I_MFU = 1u << 9, C2I_MFD = 1u << 10, C2I_GT = 1u << 11, C2I_GQ = 1u << 12, C2I_GL = 1u << 13,
  C2I_GI = 1u << 14, C2I_SUPSAT = 1u << 15, C2I_ALL = 0xffffu
};
enum : unsigned {  // bits of a mask over the 10 outputs
  C2O_TENT = 1u << 0, C2O_TENQ = 1u << 1, C2O_TENL = 1u << 2, C2O_TENI = 1u << 3, C2O_CLC = 1u << 4, C2O_FPLSL = 1u << 5,
  C2O_FPLSN = 1u << 6, C2O_FHPSL = 1u << 7, C2O_FHPSN = 1u << 8, C2O_COVPTOT = 1u << 9, C2O_ALL = 0x3ffu
};
struct TlSparseArgs {
  TlArgs a; SparseMasks m;
};
struct AdSparseArgs {
  AdArgs a; SparseMasks m;
};
typedef const C2_CONST_AS TlSparseArgs* TlSparseArgsP;
typedef const C2_CONST_AS AdSparseArgs* AdSparseArgsP;

C2_HD real_t opaque_zero() {
  real_t z = RC(0.0);
  C2_LAUNDER_V(z);
  return z;
}

// load_level for the tangents of a sparse TL launch: a plane is read under its bit, else it is an opaque zero
template <bool HAS_QSAT, class OT>
C2_HD void load_level_sparse(InPtrsP pp, unsigned m, const LaneOffT<OT>& o, int nproma, int nlev, int jk, RawLevel& r) {
  const InPtrs p = *pp;
  const OT d = level_off(OT(), jk, nproma), d1 = d + row_off(OT(), nproma);
  r.paph_k1 = (m & C2I_PAPH) ? ldg(p.paph, o.half + d1) : opaque_zero();
  r.lu_k1 = (jk + 1 < nlev) ? ((m & C2I_LU) ? ldg(p.lu, o.full + d1) : opaque_zero()) : RC(0.0);
  r.pap = (m & C2I_PAP) ? ldg(p.pap, o.full + d) : opaque_zero();
  r.q = (m & C2I_Q) ? ldg(p.q, o.full + d) : opaque_zero();
  r.t = (m & C2I_T) ? ldg(p.t, o.full + d) : opaque_zero();
  r.l = (m & C2I_L) ? ldg(p.l, o.clv + d) : opaque_zero();
  r.i = (m & C2I_I) ? ldg(p.i, o.clv + d) : opaque_zero();
  r.lude = (m & C2I_LUDE) ? ldg(p.lude, o.full + d) : opaque_zero();
  r.mfu = (m & C2I_MFU) ? ldg(p.mfu, o.full + d) : opaque_zero();
  r.mfd = (m & C2I_MFD) ? ldg(p.mfd, o.full + d) : opaque_zero();
  r.gt = (m & C2I_GT) ? ldg(p.gt, o.cml + d) : opaque_zero();
  r.gq = (m & C2I_GQ) ? ldg(p.gq, o.cml + d) : opaque_zero();
  r.gl = (m & C2I_GL) ? ldg(p.gl, o.cml + d) : opaque_zero();
  r.gi = (m & C2I_GI) ? ldg(p.gi, o.cml + d) : opaque_zero();
  r.supsat = (m & C2I_SUPSAT) ? ldg(p.supsat, o.full + d) : opaque_zero();
  if (HAS_QSAT) r.qsat = (m & C2I_QSAT) ? ldg(p.qsat, o.full + d) : opaque_zero();
}

// store_out for the output tangents of a sparse TL launch: every value pinned (C2_PIN_V), then stored under its bit
template <class OT>
C2_HD void store_out_sparse(OutPtrsP pp, unsigned m, const LaneOffT<OT>& o, int nproma, int jk, LevelOut v) {
  C2_PIN_V(v.tent); C2_PIN_V(v.tenq); C2_PIN_V(v.tenl); C2_PIN_V(v.teni); C2_PIN_V(v.clc);
  C2_PIN_V(v.covptot); C2_PIN_V(v.fplsl); C2_PIN_V(v.fplsn); C2_PIN_V(v.fhpsl); C2_PIN_V(v.fhpsn);
  const OutPtrs p = *pp;
  const OT d = level_off(OT(), jk, nproma);
  if (m & C2O_TENT) stg(p.tent, o.loc + d, v.tent);
  if (m & C2O_TENQ) stg(p.tenq, o.loc + d, v.tenq);
  if (m & C2O_TENL) stg(p.tenl, o.loc + d, v.tenl);
  if (m & C2O_TENI) stg(p.teni, o.loc + d, v.teni);
  if (m & C2O_CLC) stg(p.clc, o.full + d, v.clc);
  if (m & C2O_COVPTOT) stg(p.covptot, o.full + d, v.covptot);
  const OT d1 = d + row_off(OT(), nproma);
  if (m & C2O_FPLSL) stg(p.fplsl, o.half + d1, v.fplsl);
  if (m & C2O_FPLSN) stg(p.fplsn, o.half + d1, v.fplsn);
  if (m & C2O_FHPSL) stg(p.fhpsl, o.half + d1, v.fhpsl);
  if (m & C2O_FHPSN) stg(p.fhpsn, o.half + d1, v.fhpsn);
}

// store_top for the flux tangents a sparse TL launch stores
C2_HD void store_top_sparse(OutPtrsP p, unsigned m, const LaneOff& o, ConstsP c) {
  const real_t z = RC(0.0);
  if (m & C2O_FPLSL) p->fplsl[o.half] = z;
  if (m & C2O_FPLSN) p->fplsn[o.half] = z;
  if (m & C2O_FHPSL) p->fhpsl[o.half] = -z * c->rlvtt;
  if (m & C2O_FHPSN) p->fhpsn[o.half] = -z * c->rlstt;
}

// ---------------------------------------------------------------------------------------------------------
// Column sums (C2F_COLSUM): y_n[c] = sum_k w_n[k] out_n[k, c], formed in the sweep
// ---------------------------------------------------------------------------------------------------------
// The contract, to the bit, for every active column: acc = +0; for k = 0 .. nlevx-1: acc = fl(acc + fl(w[k] out[k])), the product rounded
// before the add.  The top half level of a flux is an exact zero, so with finite weights it leaves acc = +0 and is skipped.  w is the
// launch's device table: ten rows of nlev + 1 entries in the order of OutPtrs, entry k of a row the weight of the plane's level index k
// (the last entry of a full-level row is unused).  The row entry of level jk is wave-uniform: it is read through the scalar cache, like
// LevelTab.  The accumulators live in LDS, one slot per lane and sum (ten fp64 accumulators are 20 VGPRs, which the NL sweep's 168 --
// three waves per SIMD -- do not have beside the look-ahead set; 10 KiB per workgroup keep that occupancy): a lane reads and writes its
// own slots only, so there is no barrier and no bank conflict (consecutive lanes, consecutive words).  The host builds keep them in
// an array.  The level's outputs are pinned before the fold and every product is laundered before its add: the device compiler would
// otherwise sink arithmetic into the conditional blocks and fuse the product into the add.
struct ColsumTab {
  const real_t* w;   // (10, nlev + 1)
  OutPtrs y;         // (nblocks, nproma) arrays: NL / TL the sums written, reverse sweep the cotangents of the sums (read only); NULL: absent
  long long stride;  // their block stride
  unsigned mask;     // NL: the sums present, bits C2O_* (TL: SparseMasks::wr; reverse sweep: SparseMasks::rd)
};
struct NlColsumArgs {
  NlArgs a; ColsumTab cs;
};
struct TlColsumArgs {
  TlSparseArgs a; ColsumTab cs;
};
struct AdColsumArgs {
  AdSparseArgs a; ColsumTab cs;
};
// Column sums of an ensemble's members (C2F_MEMBER; cloudsc2_{nl,tl,vjp}_launch_ens_colsum): the column-sum blocks, the TL and the reverse
// sweep's with the parameter derivative behind them (C2F_PARLIN with C2F_SPARSE | C2F_COLSUM: tl_column / ad_reverse_column step on to `par`
// from the head of the block).  NL: NlColsumArgs itself.
struct TlEnsColsumArgs {
  TlColsumArgs a; ParLin par;
};
struct AdEnsColsumArgs {
  AdColsumArgs a; ParLin par;
  double* work;  // (PAR_COUNT, ncols_pad) doubles, as AdParArgs::work
};
typedef const C2_CONST_AS TlEnsColsumArgs* TlEnsColsumArgsP;
typedef const C2_CONST_AS AdEnsColsumArgs* AdEnsColsumArgsP;
// the sums (NL / TL: written, reverse sweep: the cotangents) advance by a member stride of their own, EnsStrides::out2 (no output tangent
// or output adjoint plane exists to claim it); the kept flux planes and the cover checkpoint by ::out and ::ckpt as in the dense ensemble
C2_HD void ens_advance(NlColsumArgs& a, const EnsStrides& m, long long member) {
  ens_advance(a.a, m, member);
  ens_advance_ptrs(a.cs.y, m.out2, member);
}
C2_HD void ens_advance(TlEnsColsumArgs& a, const EnsStrides& m, long long member) {
  ens_advance_ptrs(a.a.a.a.in, m.in, member);
  ens_advance_ptrs(a.a.a.a.din, m.in2, member);
  ens_advance_ptrs(a.a.cs.y, m.out2, member);
}
C2_HD void ens_advance(AdEnsColsumArgs& a, const EnsStrides& m, long long member) {
  ens_advance(a.a.a.a.nl, m, member);
  ens_advance_ptrs(a.a.a.a.ain, m.in2, member);
  ens_advance_ptrs(a.a.cs.y, m.out2, member);
  a.work += member * (long long)PAR_COUNT * a.a.a.a.nl.g.ncols_pad;
}
C2_HD Consts& ens_consts_of(NlColsumArgs& a) { return a.a.c; }
C2_HD Consts& ens_consts_of(TlEnsColsumArgs& a) { return a.a.a.a.c; }
C2_HD Consts& ens_consts_of(AdEnsColsumArgs& a) { return a.a.a.a.nl.c; }
C2_HD ParLin* ens_parlin_of(NlColsumArgs&) { return nullptr; }
C2_HD ParLin* ens_parlin_of(TlEnsColsumArgs& a) { return &a.par; }
C2_HD ParLin* ens_parlin_of(AdEnsColsumArgs& a) { return &a.par; }
typedef const C2_CONST_AS ColsumTab* ColsumTabP;
typedef const C2_CONST_AS real_t* ColsumRowP;
constexpr int kColsumLanes = 128;  // the sweeps' workgroup size (kBlock, asserted in cloudsc2_sweep_kernels.hpp)

struct ColsumAcc {
#if defined(__HIP_DEVICE_COMPILE__)
  real_t* s;  // this lane's slot of sum 0; sum n is kColsumLanes further
  __device__ __forceinline__ void begin(long long) {
    __shared__ real_t slots[10 * kColsumLanes];
    s = slots + threadIdx.x;
    for (int n = 0; n < 10; ++n) s[n * kColsumLanes] = RC(0.0);
  }
  // the lane's column once more after the level loop (the column-sum kernels run global_column()): no register holds it through the loop
  __device__ __forceinline__ long long column() const { return (long long)blockIdx.x * kColsumLanes + threadIdx.x; }
  __device__ __forceinline__ real_t get(int n) const { return s[n * kColsumLanes]; }
  __device__ __forceinline__ void set(int n, real_t v) { s[n * kColsumLanes] = v; }
  // C2F_MEMBER: the column is a member's own, which blockIdx alone does not give: one more LDS slot per lane holds it through the loop
  __device__ __forceinline__ long long& member_slot() const {
    __shared__ long long cols[kColsumLanes];
    return cols[threadIdx.x];
  }
  __device__ __forceinline__ void begin_member(long long column) {
    begin(column);
    member_slot() = column;
  }
  __device__ __forceinline__ long long member_column() const { return member_slot(); }
#else
  real_t s[10];
  long long gcol;
  void begin(long long column) {
    gcol = column;
    for (int n = 0; n < 10; ++n) s[n] = RC(0.0);
  }
  long long column() const { return gcol; }
  void begin_member(long long column) { begin(column); }
  long long member_column() const { return gcol; }
  real_t get(int n) const { return s[n]; }
  void set(int n, real_t v) { s[n] = v; }
#endif
  C2_HD void add(int n, real_t w, real_t v) {
    real_t p = w * v;
    C2_LAUNDER_V(p);
    set(n, get(n) + p);
  }
};

C2_HD long long colsum_off(GeomP g, ColsumTabP cs, long long gcol) {
  const long long ibl = gcol / g->nproma;
  return ibl * cs->stride + (gcol - ibl * g->nproma);
}

// one level's outputs into the sums of mask m: the pins in the order of store_out_sparse, then product and add per sum under its bit.
// (Reading all ten table entries of the level up front, whatever the mask -- ten scalar loads waited for once instead of one wait per
// conditional block -- was measured in the TL and reverse sweeps and is no gain: DESIGN.md 3.6.  So the row of an absent sum is not read.)
C2_HD void colsum_fold(ColsumAcc& acc, ColsumTabP cs, unsigned m, int nlev, int jk, LevelOut v) {
  C2_PIN_V(v.tent); C2_PIN_V(v.tenq); C2_PIN_V(v.tenl); C2_PIN_V(v.teni); C2_PIN_V(v.clc);
  C2_PIN_V(v.covptot); C2_PIN_V(v.fplsl); C2_PIN_V(v.fplsn); C2_PIN_V(v.fhpsl); C2_PIN_V(v.fhpsn);
  const ColsumRowP w = (ColsumRowP)cs->w + jk;
  const int r = nlev + 1;
  if (m & C2O_TENT) acc.add(0, w[0 * r], v.tent);
  if (m & C2O_TENQ) acc.add(1, w[1 * r], v.tenq);
  if (m & C2O_TENL) acc.add(2, w[2 * r], v.tenl);
  if (m & C2O_TENI) acc.add(3, w[3 * r], v.teni);
  if (m & C2O_CLC) acc.add(4, w[4 * r], v.clc);
  if (m & C2O_FPLSL) acc.add(5, w[5 * r + 1], v.fplsl);
  if (m & C2O_FPLSN) acc.add(6, w[6 * r + 1], v.fplsn);
  if (m & C2O_FHPSL) acc.add(7, w[7 * r + 1], v.fhpsl);
  if (m & C2O_FHPSN) acc.add(8, w[8 * r + 1], v.fhpsn);
  if (m & C2O_COVPTOT) acc.add(9, w[9 * r], v.covptot);
}

// after the last level: one row per sum present
C2_HD void colsum_store(const ColsumAcc& acc, ColsumTabP cs, unsigned m, long long ocs) {
  const OutPtrs y = cs->y;
  if (m & C2O_TENT) y.tent[ocs] = acc.get(0);
  if (m & C2O_TENQ) y.tenq[ocs] = acc.get(1);
  if (m & C2O_TENL) y.tenl[ocs] = acc.get(2);
  if (m & C2O_TENI) y.teni[ocs] = acc.get(3);
  if (m & C2O_CLC) y.clc[ocs] = acc.get(4);
  if (m & C2O_FPLSL) y.fplsl[ocs] = acc.get(5);
  if (m & C2O_FPLSN) y.fplsn[ocs] = acc.get(6);
  if (m & C2O_FHPSL) y.fhpsl[ocs] = acc.get(7);
  if (m & C2O_FHPSN) y.fhpsn[ocs] = acc.get(8);
  if (m & C2O_COVPTOT) y.covptot[ocs] = acc.get(9);
}

// the reverse sweep's cotangent of output n at a level: the rounded product of the table entry and the column's sum cotangent, as
// opaque as the load it replaces
C2_HD real_t colsum_cot(real_t w, real_t y) {
  real_t p = w * y;
  C2_LAUNDER_V(p);
  return p;
}

// ---------------------------------------------------------------------------------------------------------
// SATUR for one column
// ---------------------------------------------------------------------------------------------------------
struct SaturArgs {
  Consts c; Geom g; Strides s; const real_t* pap; const real_t* t; real_t* qsat;
};
typedef const C2_CONST_AS SaturArgs* SaturArgsP;

template <bool P>
C2_HD void satur_column(long long gcol, SaturArgsP a) {
  LaneOff o; bool active;
  if (!lane_setup(&a->g, &a->s, gcol, o, active)) return;
  if (!active) return;
  const int nlev = a->g.nlev, nproma = a->g.nproma;
  const real_t* pap = a->pap;
  const real_t* t = a->t;
  real_t* qsat = a->qsat;
  for (int jk = 0; jk < nlev; ++jk) {
    long long d = (long long)jk * nproma;
    stg(qsat, o.full + d, satur_point<P>(C2_CONSTS(a), ldg(pap, o.full + d), ldg(t, o.full + d)));
  }
}

// SATUR and its two partial derivatives as planes (cloudsc2_satur_lin_launch); qsat may be NULL: partials only
struct SaturLinArgs {
  Consts c; Geom g; Strides s; const real_t* pap; const real_t* t; real_t* qsat; real_t* dqs_dpap; real_t* dqs_dt;
};
typedef const C2_CONST_AS SaturLinArgs* SaturLinArgsP;

template <bool P>
C2_HD void satur_lin_column(long long gcol, SaturLinArgsP a) {
  LaneOff o; bool active;
  if (!lane_setup(&a->g, &a->s, gcol, o, active)) return;
  if (!active) return;
  const int nlev = a->g.nlev, nproma = a->g.nproma;
  const real_t* pap = a->pap;
  const real_t* t = a->t;
  real_t* qsat = a->qsat;
  real_t* dp = a->dqs_dpap;
  real_t* dt = a->dqs_dt;
  for (int jk = 0; jk < nlev; ++jk) {
    long long d = (long long)jk * nproma;
    real_t dqp, dqt;
    const real_t qs = satur_lin_point<P>(C2_CONSTS(a), ldg(pap, o.full + d), ldg(t, o.full + d), dqp, dqt);
    if (qsat) stg(qsat, o.full + d, qs);
    stg(dp, o.full + d, dqp);
    stg(dt, o.full + d, dqt);
  }
}

// Waves that share a SIMD are served oldest first: of the three NL waves on a SIMD the oldest runs as if alone and finishes a
// 160 000-column launch after 540 us, the second after 670, the youngest after 800 (tools/wave_times.py,
// profiles/r03_wave_times.txt) -- and the launch ends with its youngest waves, each alone on its SIMD and latency-bound, on a
// machine that has been half empty for 250 us.  With `fair` a wave's issue priority FALLS as it advances (s_setprio 3, 2, 1, 0,
// 3, ... per group of kPrioGroup levels), so a wave that has got ahead of its SIMD's other waves yields to them until they
// have caught up: the waves of a SIMD stay within about one group of each other and finish together, whatever their age and
// wherever the dispatcher put them.  It pays where a launch is ONE partial round of waves, i.e. the SIMDs carry unequal numbers
// of them (160 000 columns: 2500 waves on 1024 SIMDs, 2 or 3 each: -5 %); with equal loads or several rounds the age order is
// as good or better (waves of different age are naturally staggered), so the launcher sets it by launch size (nl launch).
constexpr int kPrioGroup = 8;
C2_HD void progress_priority(int jk, int fair) {
#if defined(__HIP_DEVICE_COMPILE__)
  if (fair && jk % kPrioGroup == 0) {
    switch ((jk / kPrioGroup) & 3) {  // (wave-uniform: scalar branches; s_setprio takes an immediate)
      case 0: __builtin_amdgcn_s_setprio(3); break;
      case 1: __builtin_amdgcn_s_setprio(2); break;
      case 2: __builtin_amdgcn_s_setprio(1); break;
      default: __builtin_amdgcn_s_setprio(0); break;
    }
  }
#else
  (void)jk; (void)fair;
#endif
}

// ---------------------------------------------------------------------------------------------------------
// NL: SATUR (optionally fused) + CLOUDSC2 for one column
// ---------------------------------------------------------------------------------------------------------
// CKPT: the sweep is the trajectory pass of the adjoint.  Rain and snow flux carries are the outputs PFPLSL5/PFPLSN5
// themselves; the one carry that is not an output (ZCOVPTOT5(JK-1)) is checkpointed -- only with the evaporation branch
// (EVAP), the one place that reads it.
template <unsigned F>
C2_HD void nl_column(long long gcol, NlArgsP a) {
  constexpr bool HAS_QSAT = (F & C2F_QSAT) != 0, PERT = (F & C2F_PERT) != 0, P = (F & C2F_PRECISE) != 0, CKPT = (F & C2F_CKPT) != 0, EVAP = (F & C2F_EVAP) != 0;
  constexpr bool OFF32 = (F & C2F_OFF32) != 0, LIN = (F & C2F_NOLIN) == 0;
  typedef typename std::conditional<OFF32, unsigned, long long>::type OT;
  static_assert(!(PERT && CKPT), "the adjoint's trajectory pass is never perturbed");
  static_assert(LIN || !CKPT, "CLOUDSC2AD's trajectory has the LPHYLIN form only");
  // COLSUM: no output plane is stored, the level's outputs are folded into the column's weighted sums (a is the head of an NlColsumArgs).
  // With CKPT the sweep keeps what the reverse sweep re-reads, in the bits of the trajectory pass: PFPLSL5 / PFPLSN5 and, with EVAP, the
  // cover checkpoint.  It is scheduled as the plain NL sweep is unless it is the one-wave-per-SIMD EVAP form.
  constexpr bool COLSUM = (F & C2F_COLSUM) != 0;
  static_assert(!COLSUM || (LIN && !PERT), "C2F_COLSUM: the LPHYLIN form, never perturbed");
  constexpr bool MEMBER = (F & C2F_MEMBER) != 0;  // (gcol is the column of an ensemble's member)
  static_assert(!MEMBER || COLSUM, "C2F_MEMBER: the column sums of an ensemble's member");
  constexpr bool ONEWAVE = CKPT && (!COLSUM || EVAP);
  constexpr bool PARMAP = (F & C2F_PARMAP) != 0;  // (a is the head of an NlParmapArgs)
  static_assert(!PARMAP || (LIN && !PERT && !COLSUM), "C2F_PARMAP: the LPHYLIN form, never perturbed, output planes");
  typedef typename std::conditional<PARMAP, LanePar, NoLane>::type LP;
  LaneOff o; bool active;
  if (!lane_setup(&a->g, &a->s, gcol, o, active)) return;
  const int nlev = a->g.nlev, nproma = a->g.nproma;
  const int fair = ONEWAVE ? 0 : a->g.fair;  // (the adjoint's trajectory pass runs one wave per SIMD: compiled without the priority code)
  const real_t lam = PERT ? a->lam : RC(0.0);
  real_t* zero_plane = a->zero_plane;
  long long ozero = 0;
  if (zero_plane) {
    long long ibl = gcol / nproma;
    ozero = ibl * a->zero_stride + (gcol - ibl * nproma);
  }
  if (!active) {
    if constexpr (COLSUM) return;  // (no covptot plane: the padded tail of the sums is not written)
    // padded tail of the last block: the driver zeroes the whole block's PCOVPTOT and CLD(:,:,NCLV)
    // (cloudsc_driver_mod.F90:87-88); nothing else is touched.
    real_t* cov = a->out.covptot;
    for (int jk = 0; jk < nlev; ++jk) {
      long long d = (long long)jk * nproma;
      cov[o.full + d] = RC(0.0);
      if (zero_plane) zero_plane[ozero + d] = RC(0.0);
    }
    return;
  }
  LevelTabP tab = (LevelTabP)a->tab;
  ConstsP c = C2_CONSTS(a);
  InPtrsP in = &a->in;
  OutPtrsP out = &a->out;
  real_t* ckpt = (CKPT && EVAP) ? a->ckpt : nullptr;
  const long long osc = (CKPT && EVAP) ? (gcol / nproma) * ((long long)nproma * nlev) + (gcol % nproma) : 0;

  // (ZTRPAUS is only read from the first band level on -- above it ZCRH2 = 1 whatever it is, cloudsc2.F90:391-399 -- so the pre-scan
  // could run when the sweep reaches the band instead of before level 1: measured equal at 160 000 columns and 1.5 % slower at 1 M,
  // like two other instruction-count candidates -- profiles/r03_b_nl_instruction_candidates_ab.txt.)
  real_t ztrpaus = tropopause<PERT>(c, tab, in, o, &a->g, lam);
  RhCrit rh;
  rhcrit_setup(ztrpaus, rh);
  [[maybe_unused]] LP lp;
  if constexpr (PARMAP) lane_load(lp, c, ((NlParmapArgsP)a)->ptsphy, ((NlParmapArgsP)a)->par, nullptr, a->g.ncols_pad, gcol);

  real_t paph_surf = RC(0.0);
  if (EVAP) {
    paph_surf = in->paph[o.half + (long long)nlev * nproma];
    if (PERT) paph_surf = pert(paph_surf, lam);
  }

  [[maybe_unused]] ColsumAcc acc;
  if constexpr (COLSUM) {
    if constexpr (MEMBER) acc.begin_member(gcol);
    else acc.begin(gcol);
    if (CKPT) {  // the kept flux planes' top half level (store_top's zeros)
      out->fplsl[o.half] = RC(0.0);
      out->fplsn[o.half] = RC(0.0);
    }
  } else {
    store_top(out, o, c);
  }

  Carry cy; C2_ZERO_CARRY(cy);
  real_t paph_k = in->paph[o.half];
  if (PERT) paph_k = pert(paph_k, lam);
  // offsets used inside the level loop, in the variant's offset type
  const LaneOffT<OT> ol = lane_off_as<OT>(o);
  const OT ozl = (OT)(ozero * (OFF32 ? (long long)sizeof(real_t) : 1)), oscl = (OT)(osc * (OFF32 ? (long long)sizeof(real_t) : 1));

  Pace pace;
  if (!ONEWAVE && (fair & 4)) pace.begin_light(&a->g);

  // one level: `cur` holds the raw inputs of level jk (requested one level ago), `nxt` receives those of level jk+1
  auto step = [&](int jk, RawLevel& cur, RawLevel& nxt) {
    const bool last = (jk == nlev - 1);
    if (!ONEWAVE) progress_priority(jk, fair & 1);
    NlArgsP ap = a;  // field pointers are re-read from the kernel-argument segment every level (transient SGPRs);
    C2_LAUNDER(ap);  // the physical constants stay resident
    // request everything level jk+1 needs now; nothing below touches `nxt` before the end of this level, so the
    // HBM latency is covered by the whole level's arithmetic
    if (!last) load_level<HAS_QSAT>(&ap->in, ol, nproma, nlev, jk + 1, nxt);
    if (!ONEWAVE) pace.nap();

    if (!HAS_QSAT) cur.qsat = satur_point<P>(c, cur.pap, cur.t);  // SATUR on the unperturbed PAP, PT
    if (PERT) perturb_raw(cur, lam);

    LevelCst k;
    level_cst(tab, jk, last, k);
    LevelIn x;
    make_level_in(cur, paph_k, paph_surf, x);
    if (CKPT && EVAP) stg(ckpt, oscl + level_off(OT(), jk, nproma), cy.covptot);  // ZCOVPTOT5(JK-1)
    LevelTraj tr;
    LevelOut lo;
    if constexpr (PARMAP) level_forward<P, EVAP, LIN, LP>(c, k, rh, x, cy, tr, lo, lp);
    else level_forward<P, EVAP, LIN>(c, k, rh, x, cy, tr, lo);
    C2_LAUNDER(ap);
    if constexpr (COLSUM) {
      const ColsumTabP cs = &((const C2_CONST_AS NlColsumArgs*)ap)->cs;
      colsum_fold(acc, cs, cs->mask, nlev, jk, lo);
      if (CKPT) {
        const OutPtrs p = ap->out;
        const OT d1 = level_off(OT(), jk, nproma) + row_off(OT(), nproma);
        stg(p.fplsl, ol.half + d1, lo.fplsl);
        stg(p.fplsn, ol.half + d1, lo.fplsn);
      }
    } else {
      store_out(&ap->out, ol, nproma, jk, lo);
      if (zero_plane) stg(zero_plane, ozl + level_off(OT(), jk, nproma), RC(0.0));
    }
    paph_k = cur.paph_k1;
  };

  // (round 3, with the waves of a SIMD kept abreast by progress_priority: a third register set for two levels of look-ahead -- 165
  // VGPRs, still three waves per SIMD -- 0.790 against 0.784 ms at 160 000 columns and 4.98 against 4.91 at 1 M: the latency a
  // deeper look-ahead would hide is not what is left.  Earlier:
  // two levels of look-ahead with three register sets in rotation need 208 VGPRs, i.e. two waves per SIMD: 0.93 instead of 0.81 ms
  // at 160 000 columns, equal at 1 M -- profiles/r02_ab_experiments.txt; with three waves it spills 148 bytes per lane.  TOUCHING the
  // rows of level jk+2 instead -- one plain 32-bit load per lane and plane, 16 dwords held for a level, 167 VGPRs, no spill -- so that
  // the lines are in L2 / the Infinity Cache when the real load comes: 0.92 instead of 0.82 ms, 5.94 instead of 4.90 ms at 1 M; the
  // sweep is limited by the requests it makes, not by their latency.  What the physics costs on top of its own memory pattern, with
  // the state placed alike (this sweep with level_forward replaced by a few adds, profiles/EXPERIMENTS.md section 2): 0.769 ms against
  // 0.818 at 160 000 columns (6 %), 4.93 against 4.98 at 1 M (1 %).)
  RawLevel ra, rb;
  load_level<HAS_QSAT>(in, ol, nproma, nlev, 0, ra);
  rb = ra;
#pragma clang loop unroll(disable)
  for (int jk = 0; jk < nlev; ++jk) {
    step(jk, ra, rb);
    ra = rb;
  }
  if constexpr (COLSUM) {
    const ColsumTabP cs = &((const C2_CONST_AS NlColsumArgs*)a)->cs;
    colsum_store(acc, cs, cs->mask, colsum_off(&a->g, cs, MEMBER ? acc.member_column() : acc.column()));
  }
}

// ---------------------------------------------------------------------------------------------------------
// Taylor test: the ten perturbed NL runs of CLOUDSC_DRIVER_TL and the level sums of its ERROR_NORM calls
// (cloudsc_driver_tl_mod.F90:21-31,197-244) in ONE sweep -- the lambdas lie on the lanes of the wave
// ---------------------------------------------------------------------------------------------------------
// A wave holds kTaylorCols columns x kTaylorLambdas lambdas: lane (c, k) runs the NL sweep of column c on the state perturbed by
// lambda_k = 10^-(k+1), exactly what nl_column<F | C2F_PERT> does, but stores nothing: it reads the BASE run's outputs of the
// level instead and keeps sum_levels(F - F5) of the ten compared fields in registers; the lane also sums TL output field k of its
// column (the denominators).  The ten lanes of a column request the same addresses (one 8-byte word per plane and level), so the
// state is read from HBM once for all ten runs instead of once per run, no perturbed outputs are written and re-read, and the
// code is the NL sweep's (one level_forward per lane and level; 60 of 64 lanes work).
//   colsum[(k*10 + f)*ncols_pad + g] = sum_levels(F_f - F5_f(lambda_k)) of column g     (k, f = 0..9; order of ERROR_NORM calls)
//   colsum[(100 + f)*ncols_pad + g]  = sum_levels(TL_f) of column g
constexpr int kTaylorLambdas = 10, kTaylorCols = 64 / kTaylorLambdas;
struct TenPtrs { const real_t* p[10]; long long stride[10]; int nlevx[10]; };  // the ten compared fields, cloudsc_driver_tl_mod.F90:233-242
struct TaylorArgs {
  NlArgs nl;      // nl.in: the unperturbed state; nl.out: the outputs of the BASE run (read here); nl.lam, zero_plane, ckpt unused
  TenPtrs tl;     // the TL outputs
  real_t lam[kTaylorLambdas];
  double* colsum;
};
typedef const C2_CONST_AS TaylorArgs* TaylorArgsP;

template <class OT>
C2_HD void load_out(OutPtrsP pp, const LaneOffT<OT>& o, int nproma, int jk, LevelOut& v) {
  const OutPtrs p = *pp;
  const OT d = level_off(OT(), jk, nproma);
  v.tent = ldx<false>(p.tent, o.loc + d);
  v.tenq = ldx<false>(p.tenq, o.loc + d);
  v.tenl = ldx<false>(p.tenl, o.loc + d);
  v.teni = ldx<false>(p.teni, o.loc + d);
  v.clc = ldx<false>(p.clc, o.full + d);
  v.covptot = ldx<false>(p.covptot, o.full + d);
  const OT d1 = d + row_off(OT(), nproma);
  v.fplsl = ldx<false>(p.fplsl, o.half + d1);
  v.fplsn = ldx<false>(p.fplsn, o.half + d1);
  v.fhpsl = ldx<false>(p.fhpsl, o.half + d1);
  v.fhpsn = ldx<false>(p.fhpsn, o.half + d1);
}

// column and lambda index of a thread: wave w holds columns [w*kTaylorCols, (w+1)*kTaylorCols), lane = k*kTaylorCols + c
C2_HD bool taylor_lane(long long gthread, long long& gcol, int& k) {
  const int lane = (int)(gthread & 63);
  k = lane / kTaylorCols;
  gcol = (gthread >> 6) * kTaylorCols + (lane - k * kTaylorCols);
  return k < kTaylorLambdas;
}

template <unsigned F>
C2_HD void taylor_column(long long gthread, TaylorArgsP ta) {
  constexpr bool HAS_QSAT = (F & C2F_QSAT) != 0, P = (F & C2F_PRECISE) != 0, EVAP = (F & C2F_EVAP) != 0, OFF32 = (F & C2F_OFF32) != 0;
  static_assert(!(F & (C2F_PERT | C2F_CKPT | C2F_NOLIN)), "flags of the Taylor sweep: QSAT, PRECISE, EVAP, OFF32");
  typedef typename std::conditional<OFF32, unsigned, long long>::type OT;
  long long gcol; int k;
  if (!taylor_lane(gthread, gcol, k)) return;
  NlArgsP a = &ta->nl;
  LaneOff o; bool active;
  if (!lane_setup(&a->g, &a->s, gcol, o, active) || !active) return;
  const int nlev = a->g.nlev, nproma = a->g.nproma;
  const real_t lam = ta->lam[k];
  LevelTabP tab = (LevelTabP)a->tab;
  ConstsP c = C2_CONSTS(a);
  InPtrsP in = &a->in;

  real_t ztrpaus = tropopause<true>(c, tab, in, o, &a->g, lam);
  RhCrit rh;
  rhcrit_setup(ztrpaus, rh);
  real_t paph_surf = RC(0.0);
  if (EVAP) paph_surf = pert(in->paph[o.half + (long long)nlev * nproma], lam);
  Carry cy; C2_ZERO_CARRY(cy);
  real_t paph_k = pert(in->paph[o.half], lam);
  const LaneOffT<OT> ol = lane_off_as<OT>(o);

  // TL output field k of this column (the fluxes live on half levels: level jk's flux is the one at jk+1, like LevelOut's;
  // their top value is zero in every run)
  const long long ibl = gcol / nproma;
  const real_t* tlk = ta->tl.p[k] + ibl * ta->tl.stride[k] + (gcol - ibl * nproma) + (ta->tl.nlevx[k] > nlev ? nproma : 0);
  double s[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, stl = 0.0;

  auto step = [&](int jk, RawLevel& cur, RawLevel& nxt) {
    const bool last = (jk == nlev - 1);
    NlArgsP ap = a;
    C2_LAUNDER(ap);
    if (!last) load_level<HAS_QSAT, OT, false>(&ap->in, ol, nproma, nlev, jk + 1, nxt);
    LevelOut base;
    load_out(&ap->out, ol, nproma, jk, base);
    const real_t tlv = tlk[(long long)jk * nproma];

    if (!HAS_QSAT) cur.qsat = satur_point<P>(c, cur.pap, cur.t);  // SATUR on the unperturbed PAP, PT
    perturb_raw(cur, lam);
    LevelCst kc;
    level_cst(tab, jk, last, kc);
    LevelIn x;
    make_level_in(cur, paph_k, paph_surf, x);
    LevelTraj tr;
    LevelOut lo;
    level_forward<P, EVAP, true>(c, kc, rh, x, cy, tr, lo);
    s[0] += (double)(base.tent - lo.tent); s[1] += (double)(base.tenq - lo.tenq);
    s[2] += (double)(base.tenl - lo.tenl); s[3] += (double)(base.teni - lo.teni);
    s[4] += (double)(base.clc - lo.clc);
    s[5] += (double)(base.fplsl - lo.fplsl); s[6] += (double)(base.fplsn - lo.fplsn);
    s[7] += (double)(base.fhpsl - lo.fhpsl); s[8] += (double)(base.fhpsn - lo.fhpsn);
    s[9] += (double)(base.covptot - lo.covptot);
    stl += (double)tlv;
    paph_k = cur.paph_k1;
  };

  RawLevel ra, rb;
  load_level<HAS_QSAT, OT, false>(in, ol, nproma, nlev, 0, ra);
  rb = ra;
#pragma clang loop unroll(disable)
  for (int jk = 0; jk < nlev; ++jk) {
    step(jk, ra, rb);
    ra = rb;
  }
  double* cs = ta->colsum;
  const long long np = a->g.ncols_pad;
#pragma unroll
  for (int f = 0; f < 10; ++f) cs[(long long)(k * 10 + f) * np + gcol] = s[f];
  cs[(long long)(100 + k) * np + gcol] = stl;
}

// The increments of the reference's test drivers: dx = 0.01*x for every input (ZSUPSAT: 0.01*PSUPSAT in the Taylor test, 0 in the
// adjoint test), taken from the trajectory inputs the sweep holds anyway.
C2_HD void self_increment(const RawLevel& r, real_t supsat_inc, RawLevel& d) {
  const real_t e = RC(0.01);
  d.paph_k1 = r.paph_k1 * e; d.pap = r.pap * e; d.q = r.q * e; d.qsat = r.qsat * e; d.t = r.t * e; d.l = r.l * e; d.i = r.i * e;
  d.lude = r.lude * e; d.lu_k1 = r.lu_k1 * e; d.mfu = r.mfu * e; d.mfd = r.mfd * e; d.gt = r.gt * e; d.gq = r.gq * e;
  d.gl = r.gl * e; d.gi = r.gi * e; d.supsat = r.supsat * supsat_inc;
}

// ---------------------------------------------------------------------------------------------------------
// TL: SATUR (optionally fused) + CLOUDSC2TL for one column
// ---------------------------------------------------------------------------------------------------------
template <unsigned F>
C2_HD void tl_column(long long gcol, TlArgsP a) {
  constexpr bool HAS_QSAT = (F & C2F_QSAT) != 0, P = (F & C2F_PRECISE) != 0, STORE_TRAJ = (F & C2F_TRAJ) != 0, EVAP = (F & C2F_EVAP) != 0;
  constexpr bool SELFINC = (F & C2F_SELFINC) != 0, SATLIN = (F & C2F_SATLIN) != 0, PARLIN = (F & C2F_PARLIN) != 0;
  constexpr bool SPARSE = (F & C2F_SPARSE) != 0, COLSUM = (F & C2F_COLSUM) != 0;
  static_assert(!COLSUM || SPARSE, "C2F_COLSUM: the sparse form's tangent loads (a is the head of a TlColsumArgs)");
  // PARLIN with SPARSE: the column sums of an ensemble's member (a is the head of a TlEnsColsumArgs; gcol is the member's column)
  constexpr bool MEMBER = (F & C2F_MEMBER) != 0;
  static_assert(MEMBER == (SPARSE && PARLIN) && (!MEMBER || COLSUM), "C2F_MEMBER: SPARSE | COLSUM | PARLIN, and only there");
  static_assert(!SATLIN || (!HAS_QSAT && !STORE_TRAJ && !SELFINC), "C2F_SATLIN: SATUR fused, no trajectory stores, increments given");
  static_assert(!SPARSE || ((HAS_QSAT != SATLIN) && !STORE_TRAJ && !SELFINC), "C2F_SPARSE: QSAT or SATLIN, no trajectory stores, increments given");
  static_assert(!PARLIN || ((HAS_QSAT != SATLIN) && !STORE_TRAJ && !SELFINC), "C2F_PARLIN: QSAT or SATLIN, no trajectory stores, increments given");
  constexpr bool PARMAP = (F & C2F_PARMAP) != 0;  // (a is the head of a TlParmapArgs)
  static_assert(!PARMAP || (PARLIN && !SPARSE), "C2F_PARMAP: the dense parameter form");
  typedef typename std::conditional<PARMAP, LanePar, NoLane>::type LP;
  typedef typename std::conditional<(F & C2F_OFF32) != 0, unsigned, long long>::type OT;
  LaneOff o, op; bool active;
  if (!lane_setup(&a->g, &a->s, gcol, o, active)) return;
  lane_setup(&a->g, &a->sp, gcol, op, active);
  if (!active) return;
  const int nlev = a->g.nlev, nproma = a->g.nproma;
  // only the fp32 variants that run three waves per SIMD (tl_kernel's launch bounds) share their SIMDs; the others -- all fp64
  // ones -- are compiled without the priority code (one more live SGPR costs the register-tight fp64 kernel 4 %)
  constexpr bool FAIRV = tl_waves_per_simd(F) == 3;
  const int fair = FAIRV ? a->g.fair : 0;
  LevelTabP tab = (LevelTabP)a->tab;
  ConstsP c = C2_CONSTS(a);
  InPtrsP in = &a->in, din = &a->din;
  OutPtrsP out = &a->out, dout = &a->dout;

  real_t ztrpaus = tropopause<false>(c, tab, in, o, &a->g, RC(0.0));
  RhCrit rh;
  rhcrit_setup(ztrpaus, rh);
  [[maybe_unused]] LP lp;
  if constexpr (PARMAP)
    lane_load(lp, c, ((TlParmapArgsP)a)->ptsphy, ((TlParmapArgsP)a)->par, ((TlParmapArgsP)a)->dpar, a->g.ncols_pad, gcol);

  real_t paph_surf = RC(0.0), dpaph_surf = RC(0.0);
  if (EVAP) {
    paph_surf = in->paph[o.half + (long long)nlev * nproma];
    if constexpr (SPARSE) dpaph_surf = (((TlSparseArgsP)a)->m.rd & C2I_PAPH) ? din->paph[op.half + (long long)nlev * nproma] : opaque_zero();
    else dpaph_surf = SELFINC ? paph_surf * RC(0.01) : din->paph[op.half + (long long)nlev * nproma];
  }

  if (STORE_TRAJ) store_top(out, o, c);
  [[maybe_unused]] ColsumAcc acc;
  if constexpr (MEMBER) acc.begin_member(gcol);
  else if constexpr (COLSUM) acc.begin(gcol);  // (no tangent plane is stored: the flux tangents' top zeros contribute nothing to a sum)
  else if constexpr (SPARSE) store_top_sparse(dout, ((TlSparseArgsP)a)->m.wr, op, c);  // (a is the head of a TlSparseArgs)
  else store_top(dout, op, c);

  Carry cy; C2_ZERO_CARRY(cy);
  Carry dcy; C2_ZERO_CARRY(dcy);
  RawLevel cur, nxt, dcur, dnxt;
  double yy = 0.0;  // SELFINC: <y,y> of the column (cloudsc_driver_ad_mod.F90:184-195; the fluxes' top values are zero)
  real_t paph_k = in->paph[o.half], dpaph_k;
  if constexpr (SPARSE) dpaph_k = (((TlSparseArgsP)a)->m.rd & C2I_PAPH) ? din->paph[op.half] : opaque_zero();
  else dpaph_k = SELFINC ? paph_k * RC(0.01) : din->paph[op.half];
  const LaneOffT<OT> ol = lane_off_as<OT>(o), opl = lane_off_as<OT>(op);  // offsets used inside the level loop
  load_level<HAS_QSAT>(in, ol, nproma, nlev, 0, cur);
  if constexpr (SPARSE) load_level_sparse<!SATLIN>(din, ((TlSparseArgsP)a)->m.rd, opl, nproma, nlev, 0, dcur);
  else if (!SELFINC) load_level<!SATLIN>(din, opl, nproma, nlev, 0, dcur);
  Pace pace;
  pace.begin(&a->g);

  // Both input sets of level jk+1 are requested at the top of level jk.  Measured alternatives (profiles/r02_ab_experiments.txt):
  // requesting the perturbation inputs at the top of their own level (no second register set for them: 280 instead of 311
  // registers) is 2 % slower, requesting the trajectory inputs between level_forward and level_tl 12 % slower, two levels of
  // look-ahead 3 % slower at 160 000 columns and equal at 1 M: the full level of distance is what hides HBM latency here.
  for (int jk = 0; jk < nlev; ++jk) {
    const bool last = (jk == nlev - 1);
    if (FAIRV) progress_priority(jk, fair);
    TlArgsP ap = a;
    C2_LAUNDER(ap);
    in = &ap->in; din = &ap->din;
    nxt = cur;
    if (!SELFINC) dnxt = dcur;
    if (!last) {
      load_level<HAS_QSAT>(in, ol, nproma, nlev, jk + 1, nxt);
      // (the masks are re-read from the kernel-argument segment where they are used, like the field pointers: transient SGPRs)
      if constexpr (SPARSE) load_level_sparse<!SATLIN>(din, ((TlSparseArgsP)ap)->m.rd, opl, nproma, nlev, jk + 1, dnxt);
      else if (!SELFINC) load_level<!SATLIN>(din, opl, nproma, nlev, jk + 1, dnxt);
    }
    pace.nap();  // (with the next level's loads in flight)
    if constexpr (SATLIN) {  // the tangent of qsat from those of pap and t: no qsat plane in either input set
      real_t dqs_dpap, dqs_dt;
      cur.qsat = satur_lin_point<P>(c, cur.pap, cur.t, dqs_dpap, dqs_dt);
      dcur.qsat = dqs_dpap * dcur.pap + dqs_dt * dcur.t;
    } else if (!HAS_QSAT) {
      cur.qsat = satur_point<P>(c, cur.pap, cur.t);
    }
    if (SELFINC) self_increment(cur, ap->supsat_inc, dcur);

    LevelCst k;
    level_cst(tab, jk, last, k);
    LevelIn x, dx;
    make_level_in(cur, paph_k, paph_surf, x);
    make_level_in(dcur, dpaph_k, dpaph_surf, dx);
    LevelTraj tr;
    LevelOut lo, dlo;
    if constexpr (PARMAP) level_forward<P, EVAP, true, LP>(c, k, rh, x, cy, tr, lo, lp);
    else level_forward<P, EVAP>(c, k, rh, x, cy, tr, lo);
    if constexpr (PARMAP) level_tl<true, LP>(c, k, x, tr, dx, dcy, dlo, nullptr, lp);
    else if constexpr (MEMBER) level_tl<true>(c, k, x, tr, dx, dcy, dlo, &((TlEnsColsumArgsP)ap)->par);
    else if constexpr (PARLIN) level_tl<true>(c, k, x, tr, dx, dcy, dlo, &((TlParArgsP)ap)->par);  // (a is the head of a TlParArgs)
    else level_tl(c, k, x, tr, dx, dcy, dlo);
    C2_LAUNDER(ap);
    out = &ap->out; dout = &ap->dout;
    if (STORE_TRAJ) store_out(out, ol, nproma, jk, lo);
    if constexpr (COLSUM) colsum_fold(acc, &((const C2_CONST_AS TlColsumArgs*)ap)->cs, ((TlSparseArgsP)ap)->m.wr, nlev, jk, dlo);
    else if constexpr (SPARSE) store_out_sparse(dout, ((TlSparseArgsP)ap)->m.wr, opl, nproma, jk, dlo);
    else store_out(dout, opl, nproma, jk, dlo);
    if (SELFINC) {
      yy += (double)dlo.tent * dlo.tent + (double)dlo.tenq * dlo.tenq + (double)dlo.tenl * dlo.tenl + (double)dlo.teni * dlo.teni +
            (double)dlo.clc * dlo.clc + (double)dlo.covptot * dlo.covptot + (double)dlo.fplsl * dlo.fplsl + (double)dlo.fplsn * dlo.fplsn +
            (double)dlo.fhpsl * dlo.fhpsl + (double)dlo.fhpsn * dlo.fhpsn;
    }
    paph_k = cur.paph_k1; dpaph_k = dcur.paph_k1;
    cur = nxt;
    if (!SELFINC) dcur = dnxt;
  }
  if (SELFINC) {
    double* p = a->yy;
    if (p) p[gcol] = yy;
  }
  if constexpr (COLSUM) {
    const ColsumTabP cs = &((const C2_CONST_AS TlColsumArgs*)a)->cs;
    colsum_store(acc, cs, ((TlSparseArgsP)a)->m.wr, colsum_off(&a->g, cs, MEMBER ? acc.member_column() : acc.column()));
  }
}

// ---------------------------------------------------------------------------------------------------------
// AD for one column.  Two passes: the trajectory pass is nl_column<.., CKPT=true> -- it writes the trajectory
// outputs and checkpoints the carries (rain and snow flux live in the outputs PFPLSL5/PFPLSN5 that have to be
// written anyway; the precipitation cover goes to the scratch plane when the evaporation branch, its only reader, is
// compiled in).  The reverse pass below re-evaluates each level's trajectory from its checkpoint and applies the
// transposed level.  It needs nothing from the trajectory pass but PFPLSL5/PFPLSN5 (and the cover plane with EVAP), so a
// caller that already has them -- any earlier NL or TL sweep over the same state -- can run it alone
// (cloudsc2_ad_launch_reverse).
//
// What both reverse sweeps read of a level is written once, below -- for ad_reverse_column (every reverse kernel but one) and for
// vjp_batch_column further down (NB cotangents over one trajectory, each the bits of ad_reverse_column<F | ASSIGN | VJP>):
//   load_reverse_traj    the trajectory side of a level: 16 inputs, PAPHP1(JK), the three checkpointed carries
//   C2_OUT_ADJOINTS      the list of a level's ten output adjoints as they are READ, in request order; its three sources:
//                        load_out_adjoint (planes), load_out_adjoint_sparse (planes under a mask), colsum_out_adjoint (column sums)
// A new carried value or trajectory plane is added there, once.  The prologue, the enthalpy fold, the dense list of input-adjoint stores
// and the assign form's stores after the loop are NOT shared: each column has its own text, as has the sparse form for its stores (it
// says why).  As functions they cost no arithmetic, but the fp64 dense sweep with the evaporation branch ran 0.6 % slower, and only
// with them written out are the kernels of both columns the earlier ones instruction for instruction (profiles/EXPERIMENTS.md,
// "Reverse sweeps: a level's loads and adjoint stores once").
// ---------------------------------------------------------------------------------------------------------
C2_HD double adjoint_norm3(double n1, double n2);  // (defined with the adjoint test's other norms at the end of this file)

// The trajectory side of a level.  cur.paph_k1 is NOT loaded: it is the paph_k of the level below, already in a register.  d, d1, last:
// the level's offset, that of the row below it and whether it is the bottom level, as the column has them (formed here once more from
// jk, the fp64 build spills one more SGPR in ten kernels: EXPERIMENTS.md, same section)
template <bool HAS_QSAT, bool EVAP, class OT>
C2_HD void load_reverse_traj(NlArgsP nl, const LaneOffT<OT>& o, OT osc, OT d, OT d1, bool last, RawLevel& cur, real_t& paph_k, Carry& cy) {
  const InPtrs p = nl->in;
  paph_k = ldg(p.paph, o.half + d);
  cur.lu_k1 = last ? RC(0.0) : ldg(p.lu, o.full + d1);
  cur.pap = ldg(p.pap, o.full + d);
  cur.q = ldg(p.q, o.full + d);
  cur.t = ldg(p.t, o.full + d);
  cur.l = ldg(p.l, o.clv + d);
  cur.i = ldg(p.i, o.clv + d);
  cur.lude = ldg(p.lude, o.full + d);
  cur.mfu = ldg(p.mfu, o.full + d);
  cur.mfd = ldg(p.mfd, o.full + d);
  cur.gt = ldg(p.gt, o.cml + d);
  cur.gq = ldg(p.gq, o.cml + d);
  cur.gl = ldg(p.gl, o.cml + d);
  cur.gi = ldg(p.gi, o.cml + d);
  cur.supsat = ldg(p.supsat, o.full + d);
  if (HAS_QSAT) cur.qsat = ldg(p.qsat, o.full + d);
  const OutPtrs po = nl->out;
  cy.rfl = ldg(po.fplsl, o.half + d);  // ZRFL5(JK) = PFPLSL5(JK)
  cy.sfl = ldg(po.fplsn, o.half + d);
  // the carried cover matters to the evaporation branch alone; without it any value gives the same results (0 here)
  cy.covptot = EVAP ? ldg(nl->ckpt, osc + d) : RC(0.0);
}

// The list of a level's output adjoints as the reverse sweeps read them, in request order (the non-VJP forms zero the planes after the
// level in the order of OutPtrs, written out in ad_reverse_column): X(C2O_* bit, OutPtrs member, its layout group,
// 1 on half levels (the level's flux is the one at jk + 1) / 0 on full levels, row of the column-sum table)
#define C2_OUT_ADJOINTS(X)                                                                                                  \
  X(C2O_TENT, tent, loc, 0, 0) X(C2O_TENQ, tenq, loc, 0, 1) X(C2O_TENL, tenl, loc, 0, 2) X(C2O_TENI, teni, loc, 0, 3)      \
  X(C2O_CLC, clc, full, 0, 4) X(C2O_COVPTOT, covptot, full, 0, 9) X(C2O_FPLSN, fplsn, half, 1, 6) X(C2O_FPLSL, fplsl, half, 1, 5) \
  X(C2O_FHPSN, fhpsn, half, 1, 8) X(C2O_FHPSL, fhpsl, half, 1, 7)

// d, d1: the offsets of level jk and of the row below it
template <class OT>
C2_HD void load_out_adjoint(OutPtrsP pp, const LaneOffT<OT>& oa, OT d, OT d1, LevelOut& ya) {
  const OutPtrs pa = *pp;
#define C2_X(bit, field, group, half_level, row) ya.field = ldg(pa.field, oa.group + (half_level ? d1 : d));
  C2_OUT_ADJOINTS(C2_X)
#undef C2_X
}
// SPARSE: an output adjoint is read under its bit of `rd`, else it is an opaque zero
template <class OT>
C2_HD void load_out_adjoint_sparse(OutPtrsP pp, unsigned rd, const LaneOffT<OT>& oa, OT d, OT d1, LevelOut& ya) {
  const OutPtrs pa = *pp;
#define C2_X(bit, field, group, half_level, row) ya.field = (rd & bit) ? ldg(pa.field, oa.group + (half_level ? d1 : d)) : opaque_zero();
  C2_OUT_ADJOINTS(C2_X)
#undef C2_X
}
// COLSUM (with SPARSE): the adjoint of output n is not a plane but weight x the column's sum cotangent (colsum_cot), under the same bit;
// the sum cotangents are re-read every level from their (nblocks, nproma) rows, which stay in cache
C2_HD void colsum_out_adjoint(ColsumTabP cs, unsigned rd, int nlev, int jk, long long ocs, LevelOut& ya) {
  const ColsumRowP w = (ColsumRowP)cs->w + jk;
  const int r = nlev + 1;
  const OutPtrs y = cs->y;
#define C2_X(bit, field, group, half_level, row) ya.field = (rd & bit) ? colsum_cot(w[row * r + half_level], y.field[ocs]) : opaque_zero();
  C2_OUT_ADJOINTS(C2_X)
#undef C2_X
}

// Everything the reverse pass reads for level jk: trajectory inputs, the three checkpointed carries, the output
// adjoints, and the OLD values of the input adjoints that are accumulated into.  (Written as `a[i] += x` after the
// compute, each read-modify-write would wait for its own HBM round trip: the compiler cannot move a load above a
// store that might alias.)
struct AdLevelLoads {
  RawLevel cur;   // trajectory inputs (load_reverse_traj)
  real_t paph_k;
  Carry cy;
  LevelOut ya;
  RawLevel xo;    // old input adjoints (PSUPSAT is assigned, not accumulated: not read)
};

// ap: the level's laundered argument block (COLSUM: the head of an AdColsumArgs); SPARSE and COLSUM assign: no old input adjoints
template <bool HAS_QSAT, bool ASSIGN, bool EVAP, class OT, bool SPARSE = false, bool COLSUM = false>
C2_HD void ad_load_level(AdArgsP ap, const LaneOffT<OT>& o, const LaneOffT<OT>& oa, OT osc, int nproma, int nlev, int jk,
                         AdLevelLoads& L, unsigned rd = 0u, [[maybe_unused]] long long ocs = 0) {
  static_assert(ASSIGN || !SPARSE, "the sparse reverse sweep assigns its input adjoints");
  static_assert(SPARSE || !COLSUM, "the column-sum reverse sweep is a sparse one");
  const bool last = (jk == nlev - 1);
  const OT d = level_off(OT(), jk, nproma);
  const OT d1 = d + row_off(OT(), nproma);
  load_reverse_traj<HAS_QSAT, EVAP>(&ap->nl, o, osc, d, d1, last, L.cur, L.paph_k, L.cy);
  if constexpr (COLSUM) colsum_out_adjoint(&((const C2_CONST_AS AdColsumArgs*)ap)->cs, rd, nlev, jk, ocs, L.ya);
  else if constexpr (SPARSE) load_out_adjoint_sparse(&ap->aout, rd, oa, d, d1, L.ya);
  else load_out_adjoint(&ap->aout, oa, d, d1, L.ya);
  if (ASSIGN) {
    // assign form: the old input adjoints are not read (16 planes of traffic less per level)
    L.xo.pap = L.xo.q = L.xo.qsat = L.xo.t = L.xo.l = L.xo.i = L.xo.lude = L.xo.mfu = L.xo.mfd = RC(0.0);
    L.xo.gt = L.xo.gq = L.xo.gl = L.xo.gi = L.xo.lu_k1 = L.xo.paph_k1 = RC(0.0);
    return;
  }
  const InPtrsRW px = ap->ain;
  L.xo.pap = ldg(px.pap, oa.full + d);
  L.xo.q = ldg(px.q, oa.full + d);
  L.xo.qsat = ldg(px.qsat, oa.full + d);
  L.xo.t = ldg(px.t, oa.full + d);
  L.xo.l = ldg(px.l, oa.clv + d);
  L.xo.i = ldg(px.i, oa.clv + d);
  L.xo.lude = ldg(px.lude, oa.full + d);
  L.xo.mfu = ldg(px.mfu, oa.full + d);
  L.xo.mfd = ldg(px.mfd, oa.full + d);
  L.xo.gt = ldg(px.gt, oa.cml + d);
  L.xo.gq = ldg(px.gq, oa.cml + d);
  L.xo.gl = ldg(px.gl, oa.cml + d);
  L.xo.gi = ldg(px.gi, oa.cml + d);
  L.xo.lu_k1 = last ? RC(0.0) : ldg(px.lu, oa.full + d1);
  L.xo.paph_k1 = last ? RC(0.0) : ldg(px.paph, oa.half + d1);
}

// reverse sweep (cloudsc2ad.F90:877-1740); the trajectory pass has run before
template <unsigned F>
C2_HD double ad_reverse_column(long long gcol, AdArgsP a) {  // returns |norm3| of the column with C2F_ADNORM (+inf for NaN), else 0
  constexpr bool HAS_QSAT = (F & C2F_QSAT) != 0, P = (F & C2F_PRECISE) != 0, EVAP = (F & C2F_EVAP) != 0;
  constexpr bool OFF32 = (F & C2F_OFF32) != 0, ASSIGN = (F & C2F_ASSIGN) != 0, ADNORM = (F & C2F_ADNORM) != 0;
  constexpr bool VJP = (F & C2F_VJP) != 0, SATLIN = (F & C2F_SATLIN) != 0, PARLIN = (F & C2F_PARLIN) != 0;
  static_assert(!SATLIN || (VJP && !HAS_QSAT), "C2F_SATLIN: the vector-Jacobian form with SATUR fused");
  static_assert(!PARLIN || (VJP && (HAS_QSAT != SATLIN)), "C2F_PARLIN: the vector-Jacobian form, QSAT or SATLIN");
  static_assert(!ADNORM || ASSIGN, "the fused norms are those of the adjoint test: assign form");
  static_assert(!VJP || (ASSIGN && !ADNORM), "the vector-Jacobian product assigns its input adjoints and forms no norms");
  constexpr bool SPARSE = (F & C2F_SPARSE) != 0, COLSUM = (F & C2F_COLSUM) != 0;
  static_assert(!SPARSE || (VJP && (HAS_QSAT != SATLIN)), "C2F_SPARSE: the vector-Jacobian form, QSAT or SATLIN");
  static_assert(!COLSUM || SPARSE, "C2F_COLSUM: the sparse form's gradient stores (a is the head of an AdColsumArgs)");
  // PARLIN with SPARSE: the column sums of an ensemble's member (a is the head of an AdEnsColsumArgs); the write mask may be empty
  constexpr bool MEMBER = SPARSE && PARLIN;
  static_assert(!MEMBER || COLSUM, "parameter adjoints of a sparse reverse sweep: the column-sum form of an ensemble");
  constexpr bool PARMAP = (F & C2F_PARMAP) != 0;  // (a is the head of an AdParmapArgs)
  static_assert(!PARMAP || (PARLIN && !SPARSE), "C2F_PARMAP: the dense parameter form");
  typedef typename std::conditional<PARMAP, LanePar, NoLane>::type LP;
  typedef typename std::conditional<OFF32, unsigned, long long>::type OT;
  LaneOff o, oa64; bool active;
  if (!lane_setup(&a->nl.g, &a->nl.s, gcol, o, active)) return 0.0;
  lane_setup(&a->nl.g, &a->sa, gcol, oa64, active);
  if (!active) return 0.0;
  const int nlev = a->nl.g.nlev, nproma = a->nl.g.nproma;
  LevelTabP tab = (LevelTabP)a->nl.tab;
  ConstsP c = C2_CONSTS(&a->nl);
  InPtrsP in = &a->nl.in;

  // scratch: (NPROMA, NLEV, NBLOCKS) contiguous
  const long long osc64 = (gcol / nproma) * ((long long)nproma * nlev) + (gcol % nproma);
  // offsets used inside the level loop, in the variant's offset type
  const LaneOffT<OT> ol = lane_off_as<OT>(o), oa = lane_off_as<OT>(oa64);
  const OT osc = (OT)(osc64 * (OFF32 ? (long long)sizeof(real_t) : 1));

  real_t ztrpaus = tropopause<false>(c, tab, in, o, &a->nl.g, RC(0.0));
  RhCrit rh;
  rhcrit_setup(ztrpaus, rh);
  [[maybe_unused]] LP lp;
  if constexpr (PARMAP) lane_load(lp, c, ((AdParmapArgsP)a)->ptsphy, ((AdParmapArgsP)a)->par, nullptr, a->nl.g.ncols_pad, gcol);
  const real_t paph_bottom = in->paph[o.half + (long long)nlev * nproma];
  const real_t paph_surf = EVAP ? paph_bottom : RC(0.0);

  Carry acy; C2_ZERO_CARRY(acy);
  real_t paph_pending = RC(0.0);  // contribution of level jk+1 to the PAPHP1 adjoint at half level jk+1
  real_t surf_acc = RC(0.0);      // PAPHP1(KLEV+1) adjoint, written once at the end
  real_t paph_k1 = paph_bottom;
  double n2 = 0.0;  // ADNORM: <x0, x_adj>, x0 = 0.01 * trajectory inputs, ZSUPSAT0 = 0 (cloudsc_driver_ad_mod.F90:139,240-256)
  AdLevelLoads L;
  [[maybe_unused]] long long ocs = 0;  // COLSUM: the column's place in the sum cotangents
  if constexpr (COLSUM) ocs = colsum_off(&a->nl.g, &((const C2_CONST_AS AdColsumArgs*)a)->cs, gcol);
  [[maybe_unused]] ParAcc pacc = {{0.0, 0.0, 0.0, 0.0}};  // PARLIN
  Pace pace;
  pace.begin(&a->nl.g);
  for (int jk = nlev - 1; jk >= 0; --jk) {
    const bool last = (jk == nlev - 1);
    pace.nap();
    const OT d = level_off(OT(), jk, nproma);
    const OT d1 = d + row_off(OT(), nproma);
    AdArgsP ap = a;
    C2_LAUNDER(ap);
    // all 44 loads of the level at its top; requesting the trajectory part (19 values) one level ahead was measured: +1.6 % time
    // at 160 000 columns, -1 % at 1 M (profiles/r02_ab_experiments.txt)
    // (SPARSE: the masks are re-read from the kernel-argument segment where they are used, like the field pointers; a is the head of
    // an AdSparseArgs)
    if constexpr (COLSUM) ad_load_level<HAS_QSAT, ASSIGN, EVAP, OT, true, true>(ap, ol, oa, osc, nproma, nlev, jk, L, ((AdSparseArgsP)ap)->m.rd, ocs);
    else if constexpr (SPARSE) ad_load_level<HAS_QSAT, ASSIGN, EVAP, OT, true>(ap, ol, oa, osc, nproma, nlev, jk, L, ((AdSparseArgsP)ap)->m.rd);
    else ad_load_level<HAS_QSAT, ASSIGN, EVAP>(ap, ol, oa, osc, nproma, nlev, jk, L);
    RawLevel& cur = L.cur;
    cur.paph_k1 = paph_k1;
    const RawLevel& xo = L.xo;
    LevelOut ya = L.ya;  // enthalpy-flux adjoints folded in below (cloudsc2ad.F90:914-921)

    [[maybe_unused]] real_t dqs_dpap = RC(0.0), dqs_dt = RC(0.0);
    if constexpr (SATLIN) {
      // (PAP and PT requested one level ahead, so that SATUR runs under the level's other loads: measured, no gain -- EXPERIMENTS.md 12)
      cur.qsat = satur_lin_point<P>(c, cur.pap, cur.t, dqs_dpap, dqs_dt);
    } else if (!HAS_QSAT) {
      cur.qsat = satur_point<P>(c, cur.pap, cur.t);
    }
    LevelCst k;
    level_cst(tab, jk, last, k);
    LevelIn x;
    make_level_in(cur, L.paph_k, paph_surf, x);
    LevelTraj tr;
    LevelOut lo;
    if constexpr (PARMAP) level_forward<P, EVAP, true, LP>(c, k, rh, x, L.cy, tr, lo, lp);
    else level_forward<P, EVAP>(c, k, rh, x, L.cy, tr, lo);

    ya.fplsn = ya.fplsn - ya.fhpsn * c->rlstt;
    ya.fplsl = ya.fplsl - ya.fhpsl * c->rlvtt;
    LevelIn ax;
    if constexpr (PARMAP) level_ad<true, LP>(c, k, x, tr, ya, acy, ax, nullptr, &pacc, lp);
    else if constexpr (MEMBER) level_ad<true>(c, k, x, tr, ya, acy, ax, &((AdEnsColsumArgsP)ap)->par, &pacc);
    else if constexpr (PARLIN) level_ad<true>(c, k, x, tr, ya, acy, ax, &((AdParArgsP)ap)->par, &pacc);  // (a is the head of an AdParArgs)
    else level_ad(c, k, x, tr, ya, acy, ax);
    if constexpr (SATLIN) {  // the adjoint of qsat goes to pap and t through SATUR's transpose; it has no plane of its own
      ax.pap += dqs_dpap * ax.qs;
      ax.t += dqs_dt * ax.qs;
    }

    C2_LAUNDER(ap);
    const InPtrsRW px = ap->ain;
    const OutPtrs pa = ap->aout;
    if constexpr (SPARSE) {
      // the dense form's values (xo + ax with xo = 0: a -0 becomes +0 exactly as there), each pinned in the level's straight line, then
      // stored under its bit; an absent plane's pointer is never formed into an address.  The pins stand where the dense sweep's stores
      // stand, in their order and in their blocks (PLU and PAPHP1 under !last): the SLP vectoriser starts its trees from the operands of
      // instructions without users, stores and these asm statements alike, in program order -- in another order, or with the two
      // !last values formed up here, the fp32 build packs other pairs and other products fuse (measured: DESIGN.md 3.6)
      const unsigned wr = ((AdSparseArgsP)ap)->m.wr;
      const real_t v_pap = xo.pap + ax.pap, v_q = xo.q + ax.q, v_t = xo.t + ax.t, v_l = xo.l + ax.l, v_i = xo.i + ax.i;
      const real_t v_lude = xo.lude + ax.lude, v_mfu = xo.mfu + ax.mfu, v_mfd = xo.mfd + ax.mfd, v_gt = xo.gt + ax.gt, v_gq = xo.gq + ax.gq;
      const real_t v_gl = xo.gl + ax.gl, v_gi = xo.gi + ax.gi, v_supsat = ax.q;
      [[maybe_unused]] real_t v_qsat = RC(0.0);
      if constexpr (!SATLIN) v_qsat = xo.qsat + ax.qs;
      C2_PIN_V(v_pap); C2_PIN_V(v_q);
      if constexpr (!SATLIN) C2_PIN_V(v_qsat);
      C2_PIN_V(v_t); C2_PIN_V(v_l); C2_PIN_V(v_i); C2_PIN_V(v_lude); C2_PIN_V(v_mfu); C2_PIN_V(v_mfd); C2_PIN_V(v_gt); C2_PIN_V(v_gq);
      C2_PIN_V(v_gl); C2_PIN_V(v_gi); C2_PIN_V(v_supsat);
      if (wr & C2I_PAP) stg(px.pap, oa.full + d, v_pap);
      if (wr & C2I_Q) stg(px.q, oa.full + d, v_q);
      if constexpr (!SATLIN) {
        if (wr & C2I_QSAT) stg(px.qsat, oa.full + d, v_qsat);
      }
      if (wr & C2I_T) stg(px.t, oa.full + d, v_t);
      if (wr & C2I_L) stg(px.l, oa.clv + d, v_l);
      if (wr & C2I_I) stg(px.i, oa.clv + d, v_i);
      if (wr & C2I_LUDE) stg(px.lude, oa.full + d, v_lude);
      if (wr & C2I_MFU) stg(px.mfu, oa.full + d, v_mfu);
      if (wr & C2I_MFD) stg(px.mfd, oa.full + d, v_mfd);
      if (wr & C2I_GT) stg(px.gt, oa.cml + d, v_gt);
      if (wr & C2I_GQ) stg(px.gq, oa.cml + d, v_gq);
      if (wr & C2I_GL) stg(px.gl, oa.cml + d, v_gl);
      if (wr & C2I_GI) stg(px.gi, oa.cml + d, v_gi);
      if (wr & C2I_SUPSAT) stg(px.supsat, oa.full + d, v_supsat);
      if (!last) {
        const real_t v_lu = xo.lu_k1 + ax.lu_k1;
        C2_PIN_V(v_lu);
        if (wr & C2I_LU) stg(px.lu, oa.full + d1, v_lu);
      }
      surf_acc += ax.paph_surf;
      if (last) {
        surf_acc += ax.paph_k1;
      } else {
        const real_t v_paph = xo.paph_k1 + (ax.paph_k1 + paph_pending);
        C2_PIN_V(v_paph);
        if (wr & C2I_PAPH) stg(px.paph, oa.half + d1, v_paph);
      }
    } else {
      // accumulate input adjoints (cloudsc2ad.F90:1723-1738; PSUPSAT assigned, :1733)
      stg(px.pap, oa.full + d, xo.pap + ax.pap);
      stg(px.q, oa.full + d, xo.q + ax.q);
      if constexpr (!SATLIN) stg(px.qsat, oa.full + d, xo.qsat + ax.qs);
      stg(px.t, oa.full + d, xo.t + ax.t);
      stg(px.l, oa.clv + d, xo.l + ax.l);
      stg(px.i, oa.clv + d, xo.i + ax.i);
      stg(px.lude, oa.full + d, xo.lude + ax.lude);
      stg(px.mfu, oa.full + d, xo.mfu + ax.mfu);
      stg(px.mfd, oa.full + d, xo.mfd + ax.mfd);
      stg(px.gt, oa.cml + d, xo.gt + ax.gt);
      stg(px.gq, oa.cml + d, xo.gq + ax.gq);
      stg(px.gl, oa.cml + d, xo.gl + ax.gl);
      stg(px.gi, oa.cml + d, xo.gi + ax.gi);
      // VJP: d(zqp1)/d(PSUPSAT) = 1 (cloudsc2tl.F90:345), so the PSUPSAT adjoint is zqp1's own (ax.q); ax.supsat = PTSPHY*zqp1 is the
      // reference's CLOUDSC2AD, which the other forms reproduce
      stg(px.supsat, oa.full + d, VJP ? ax.q : ax.supsat);
      if (!last) stg(px.lu, oa.full + d1, xo.lu_k1 + ax.lu_k1);
      surf_acc += ax.paph_surf;
      if (last) {
        surf_acc += ax.paph_k1;
      } else {
        stg(px.paph, oa.half + d1, xo.paph_k1 + (ax.paph_k1 + paph_pending));
      }
    }
    if (ADNORM) {  // (assign form: what has just been stored is ax itself)
      const double e = 0.01;
      n2 += ((double)cur.pap * e) * ax.pap + ((double)cur.q * e) * ax.q + ((double)cur.qsat * e) * ax.qs + ((double)cur.t * e) * ax.t +
            ((double)cur.l * e) * ax.l + ((double)cur.i * e) * ax.i + ((double)cur.lude * e) * ax.lude + ((double)cur.mfu * e) * ax.mfu +
            ((double)cur.mfd * e) * ax.mfd + ((double)cur.gt * e) * ax.gt + ((double)cur.gq * e) * ax.gq + ((double)cur.gl * e) * ax.gl +
            ((double)cur.gi * e) * ax.gi;
      if (!last) n2 += ((double)cur.lu_k1 * e) * ax.lu_k1 + ((double)cur.paph_k1 * e) * (ax.paph_k1 + paph_pending);
    }
    paph_pending = ax.paph_k;

    // output adjoints are consumed (cloudsc2ad.F90:917-919,955-966,1173,1572); VJP: they are the caller's, read only
    if constexpr (!VJP) {
      stg(pa.tent, oa.loc + d, RC(0.0));
      stg(pa.tenq, oa.loc + d, RC(0.0));
      stg(pa.tenl, oa.loc + d, RC(0.0));
      stg(pa.teni, oa.loc + d, RC(0.0));
      stg(pa.clc, oa.full + d, RC(0.0));
      stg(pa.covptot, oa.full + d, RC(0.0));
      stg(pa.fplsl, oa.half + d1, RC(0.0));
      stg(pa.fplsn, oa.half + d1, RC(0.0));
      stg(pa.fhpsl, oa.half + d1, RC(0.0));
      stg(pa.fhpsn, oa.half + d1, RC(0.0));
    }

    paph_k1 = L.paph_k;
  }
  InPtrsRWP ain = &a->ain;
  if constexpr (SPARSE) {  // the stores outside the level loop, each under its plane's bit
    const unsigned wr = ((AdSparseArgsP)a)->m.wr;
    if (wr & C2I_PAPH) {
      ain->paph[oa64.half] = paph_pending;
      ain->paph[oa64.half + (long long)nlev * nproma] = surf_acc;
    }
    if (wr & C2I_LU) ain->lu[oa64.full] = RC(0.0);
  } else if (ASSIGN) {
    ain->paph[oa64.half] = paph_pending;
    ain->paph[oa64.half + (long long)nlev * nproma] = surf_acc;
    ain->lu[oa64.full] = RC(0.0);
  } else {
    ain->paph[oa64.half] += paph_pending;
    ain->paph[oa64.half + (long long)nlev * nproma] += surf_acc;
  }
  if constexpr (PARLIN) {  // the lane's four sums: consecutive lanes, consecutive doubles of each row (gcol < ncols_pad: lane_setup)
    double* work;
    if constexpr (PARMAP) work = ((AdParmapArgsP)a)->apar;  // (the result itself)
    else if constexpr (MEMBER) work = ((AdEnsColsumArgsP)a)->work;
    else work = ((AdParArgsP)a)->work;
    const long long np = a->nl.g.ncols_pad;
#pragma unroll
    for (int i = 0; i < PAR_COUNT; ++i) work[i * np + gcol] = pacc.v[i];
  }
  // the adjoint of the (constant zero) top fluxes is discarded (cloudsc2ad.F90:1678-1679,917-919)
  if constexpr (!VJP) {
    OutPtrsP aout = &a->aout;
    aout->fplsl[oa64.half] = RC(0.0);
    aout->fplsn[oa64.half] = RC(0.0);
    aout->fhpsl[oa64.half] = RC(0.0);
    aout->fhpsn[oa64.half] = RC(0.0);
  }
  if (ADNORM) {
    // the two half levels the loop does not store: PAPHP1(1) (paph_k1 now holds the trajectory's value there) and PAPHP1(KLEV+1)
    n2 += ((double)paph_k1 * 0.01) * paph_pending + ((double)paph_bottom * 0.01) * surf_acc;
    double* norms = a->norms;
    const long long np = a->nl.g.ncols_pad;
    double n3 = adjoint_norm3(norms[gcol], n2);
    norms[np + gcol] = n2;
    norms[2 * np + gcol] = n3;
    n3 = fabs(n3);
    if (!(n3 == n3)) n3 = (double)INFINITY;  // NaN counts as failure
    return n3;
  }
  return 0.0;
}

// ---------------------------------------------------------------------------------------------------------
// Batched TL and reverse sweeps: several tangents / cotangents over ONE trajectory (cloudsc2_tl_launch_batch, cloudsc2_vjp_launch_batch)
// ---------------------------------------------------------------------------------------------------------
// A Jacobian block, a singular-vector iteration or an ensemble of perturbations push K directions through the TL or the reverse sweep
// over one state.  K launches read the 16 trajectory planes K times.  Here a lane reads the trajectory inputs of a level once and
// then runs the level for each of its NB <= kBatchMax directions, each with its own carries.  NB is a COMPILE-TIME count (one
// kernel per count, the launchers pick it): the direction loop is fully unrolled, the per-direction carries are registers (never
// a runtime-indexed array), and the inputs of direction b + 1 are requested under the arithmetic of direction b.  Every
// direction's results are the bits of the single-direction sweeps (tl_column without C2F_TRAJ / C2F_SELFINC,
// ad_reverse_column<F | C2F_ASSIGN | C2F_VJP>); launder_level below says what that takes.
constexpr int kBatchMax = 4;  // directions per launch: the fp64 kernels hold it without scratch at one wave per SIMD

// (the pointer sets from the launch's direction count on are not read)
struct TlBatchArgs {
  Consts c; Geom g; Strides s, sp; InPtrs in; InPtrs din[kBatchMax]; OutPtrs dout[kBatchMax]; const LevelTab* tab;
};
// (like AdArgs: the trajectory side is the NL sweep's block; nl.out: PFPLSL5 / PFPLSN5 are read, nl.ckpt with the evaporation branch)
struct VjpBatchArgs {
  NlArgs nl; Strides sa; InPtrsRW ain[kBatchMax]; OutPtrs aout[kBatchMax];
};
typedef const C2_CONST_AS TlBatchArgs* TlBatchArgsP;
typedef const C2_CONST_AS VjpBatchArgs* VjpBatchArgsP;

// Bit-equality with the single-direction sweeps is the contract of the batched ones, and the library is compiled with the device
// default contraction: which multiplies fuse into which adds depends on how many users a product has and on what the compiler
// knows around it.  Measured on the MI355X, each as last-place differences from the single sweeps in the cloud levels (a few
// hundred elements of a 100-column state), in some variants and on some states only:
//   - level_forward evaluated once and shared by the unrolled directions: its products, and the trajectory-only products inside
//     level_tl / level_ad that the compiler then evaluates once for all directions, have several users and fuse differently;
//   - the same with the LevelTraj made opaque per direction: the fusions of tl_column across level_forward and level_tl are lost;
//   - the direction loop behind a runtime guard `b < nb`: the compiler builds one level loop per count, each with its own fusions.
// What holds in every variant and on every state tried: every direction gets the single sweep's own straight line -- level_forward
// and level_tl / level_ad on ITS OWN opaque copy of the level's inputs, the carry and the constants' address (an empty asm
// statement per value: no instruction) -- under a compile-time direction count.  The compiler can then neither share anything
// between directions nor tell the copies from loaded values.  The trajectory is still READ once per launch, which is the saving:
// the sweeps wait for HBM, not for the level's arithmetic (measured: the launch runs at the byte ratio).
// (The host builds, compiled without contraction, need nothing.  C2_LAUNDER_V is defined with the sparse sweeps' helpers above.)
C2_HD void launder_level(LevelIn& x, LevelCst& k, Carry& cy) {  // (all of x but paph_surf, which is invariant over the levels)
  C2_LAUNDER_V(x.paph_k); C2_LAUNDER_V(x.paph_k1); C2_LAUNDER_V(x.pap); C2_LAUNDER_V(x.q); C2_LAUNDER_V(x.qs); C2_LAUNDER_V(x.t);
  C2_LAUNDER_V(x.l); C2_LAUNDER_V(x.i); C2_LAUNDER_V(x.lude); C2_LAUNDER_V(x.lu_k1); C2_LAUNDER_V(x.mfu); C2_LAUNDER_V(x.mfd);
  C2_LAUNDER_V(x.gt); C2_LAUNDER_V(x.gq); C2_LAUNDER_V(x.gl); C2_LAUNDER_V(x.gi); C2_LAUNDER_V(x.supsat);
  C2_LAUNDER(k.ceta); C2_LAUNDER(k.zscalm);
  C2_LAUNDER_V(cy.rfl); C2_LAUNDER_V(cy.sfl); C2_LAUNDER_V(cy.covptot);
}

// F: C2F_QSAT (always: the batched launchers require PQSAT) | C2F_PRECISE | C2F_EVAP | C2F_OFF32; NB: the directions of the launch
template <unsigned F, int NB>
C2_HD void tl_batch_column(long long gcol, TlBatchArgsP a) {
  static_assert(NB >= 1 && NB <= kBatchMax, "directions of one launch: 1..kBatchMax");
  constexpr bool P = (F & C2F_PRECISE) != 0, EVAP = (F & C2F_EVAP) != 0, AHEAD = !EVAP;
  static_assert((F & C2F_QSAT) && !(F & ~(C2F_QSAT | C2F_PRECISE | C2F_EVAP | C2F_OFF32)), "flags of the batched TL sweep: QSAT, PRECISE, EVAP, OFF32");
  typedef typename std::conditional<(F & C2F_OFF32) != 0, unsigned, long long>::type OT;
  LaneOff o, op; bool active;
  if (!lane_setup(&a->g, &a->s, gcol, o, active)) return;
  lane_setup(&a->g, &a->sp, gcol, op, active);
  if (!active) return;
  const int nlev = a->g.nlev, nproma = a->g.nproma;
  LevelTabP tab = (LevelTabP)a->tab;
  ConstsP c = C2_CONSTS(a);
  InPtrsP in = &a->in;

  // once per column, not once per direction: the tropopause pre-scan, the critical-humidity setup, the lane offsets, the loads
  real_t ztrpaus = tropopause<false>(c, tab, in, o, &a->g, RC(0.0));
  RhCrit rh;
  rhcrit_setup(ztrpaus, rh);
  real_t paph_surf = RC(0.0);
  if (EVAP) paph_surf = in->paph[o.half + (long long)nlev * nproma];

  Carry cy; C2_ZERO_CARRY(cy);
  Carry dcy[NB];
  real_t dpaph_k[NB], dpaph_surf[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    C2_ZERO_CARRY(dcy[b]);
    dpaph_surf[b] = RC(0.0);
    store_top(&a->dout[b], op, c);
    const real_t* dpaph = a->din[b].paph;
    dpaph_k[b] = dpaph[op.half];
    if (EVAP) dpaph_surf[b] = dpaph[op.half + (long long)nlev * nproma];
  }
  RawLevel cur, nxt;
  real_t paph_k = in->paph[o.half];
  const LaneOffT<OT> ol = lane_off_as<OT>(o), opl = lane_off_as<OT>(op);  // offsets used inside the level loop
  load_level<true>(in, ol, nproma, nlev, 0, cur);
  Pace pace;
  pace.begin(&a->g);

  // The trajectory inputs of level jk+1 are requested at the top of level jk, as in tl_column.  The direction inputs are requested
  // one direction ahead: those of direction 0 at the top of their own level, those of direction b + 1 under the arithmetic of
  // direction b -- two register sets for them whatever NB is.  In the evaporation variants, the
  // register-tightest (an earlier form of this sweep spilled 20-28 bytes per lane there with the second set), direction b > 0 asks
  // for its inputs at its own top; not measured against the look-ahead in the present form.
  for (int jk = 0; jk < nlev; ++jk) {
    const bool last = (jk == nlev - 1);
    TlBatchArgsP ap = a;
    C2_LAUNDER(ap);
    nxt = cur;
    if (!last) load_level<true>(&ap->in, ol, nproma, nlev, jk + 1, nxt);
    RawLevel dcur;
    load_level<true>(&ap->din[0], opl, nproma, nlev, jk, dcur);
    pace.nap();  // (with the loads in flight)

    LevelCst k;
    level_cst(tab, jk, last, k);
    LevelIn x;
    make_level_in(cur, paph_k, paph_surf, x);
    Carry cy_out = cy;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      if (!AHEAD && b > 0) load_level<true>(&ap->din[b], opl, nproma, nlev, jk, dcur);
      RawLevel dnxt = dcur;
      if (AHEAD && b + 1 < NB) load_level<true>(&ap->din[b + 1 < NB ? b + 1 : b], opl, nproma, nlev, jk, dnxt);
      // this direction's own straight line (launder_level says why): every direction leaves the same trajectory carry
      LevelIn xb = x;
      LevelCst kb = k;
      RhCrit rhb = rh;
      cy_out = cy;
      launder_level(xb, kb, cy_out);
      C2_LAUNDER_V(xb.paph_surf); C2_LAUNDER_V(rhb.zeta3); C2_LAUNDER_V(rhb.zrh2); C2_LAUNDER_V(rhb.zdeta1);
      ConstsP cb = c;  // (and its own view of the constants: a product of two of them is shared otherwise)
      C2_LAUNDER(cb);
      LevelTraj tr;
      LevelOut lo;
      level_forward<P, EVAP>(cb, kb, rhb, xb, cy_out, tr, lo);
      LevelIn dx;
      make_level_in(dcur, dpaph_k[b], dpaph_surf[b], dx);
      LevelOut dlo;
      level_tl(cb, kb, xb, tr, dx, dcy[b], dlo);
      C2_LAUNDER(ap);
      store_out(&ap->dout[b], opl, nproma, jk, dlo);
      dpaph_k[b] = dcur.paph_k1;
      dcur = dnxt;
    }
    cy = cy_out;
    paph_k = cur.paph_k1;
    cur = nxt;
  }
}

// ---------------------------------------------------------------------------------------------------------
// The parameter Jacobian in one sweep: d out / d rkconv ... rpecons over ONE trajectory (cloudsc2_tl_launch_parjac)
// ---------------------------------------------------------------------------------------------------------
// A calibration of the tunable parameters by Gauss-Newton needs every column of d out / d p, which forward mode gives as one
// tl_column<F | C2F_PARLIN> launch per parameter with a unit tangent -- each reading the 16 trajectory planes and 16 tangent planes
// that hold nothing but zeros.  The parameter directions are special: the field tangents are identically zero and there are at most
// kBatchMax of them.  This sweep is tl_batch_column with the direction inputs replaced by zeros in registers: the trajectory is read
// once, no tangent plane is read, and direction b runs level_tl<true> with its own ParLin par[b] (the host's make_parlin of the unit
// tangent of parameter b).  Every direction is the bits of tl_column<F | C2F_PARLIN> on zero-filled planes: its own straight line as in
// tl_batch_column (launder_level), and zeros the compiler cannot tell from loaded values (an empty asm statement on each).
// The direction count belongs to the flag word: without the evaporation branch nothing depends on rpecons and its direction is not run.
constexpr int parjac_directions(unsigned f) { return (f & C2F_EVAP) ? PAR_COUNT : PAR_COUNT - 1; }
static_assert(PAR_COUNT <= kBatchMax && PAR_RPECONS == PAR_COUNT - 1, "the parameter directions fit one launch, rpecons last");

// (dout and par from the launch's direction count on are not read)
struct TlParJacArgs {
  Consts c; Geom g; Strides s, sp; InPtrs in; OutPtrs dout[kBatchMax]; ParLin par[kBatchMax]; const LevelTab* tab;
};
typedef const C2_CONST_AS TlParJacArgs* TlParJacArgsP;

// the zero field tangents of one level, opaque (tl_column reads them from its tangent planes; without the evaporation branch its
// surface-pressure tangent is the literal zero it is here)
template <bool EVAP>
C2_HD void zero_level_in(LevelIn& dx) {
  dx.paph_k = dx.paph_k1 = dx.pap = dx.q = dx.qs = dx.t = dx.l = dx.i = dx.lude = dx.lu_k1 = dx.mfu = dx.mfd = dx.gt = dx.gq = dx.gl =
      dx.gi = dx.supsat = dx.paph_surf = RC(0.0);
  C2_LAUNDER_V(dx.paph_k); C2_LAUNDER_V(dx.paph_k1); C2_LAUNDER_V(dx.pap); C2_LAUNDER_V(dx.q); C2_LAUNDER_V(dx.qs); C2_LAUNDER_V(dx.t);
  C2_LAUNDER_V(dx.l); C2_LAUNDER_V(dx.i); C2_LAUNDER_V(dx.lude); C2_LAUNDER_V(dx.lu_k1); C2_LAUNDER_V(dx.mfu); C2_LAUNDER_V(dx.mfd);
  C2_LAUNDER_V(dx.gt); C2_LAUNDER_V(dx.gq); C2_LAUNDER_V(dx.gl); C2_LAUNDER_V(dx.gi); C2_LAUNDER_V(dx.supsat);
  if (EVAP) C2_LAUNDER_V(dx.paph_surf);
}

// The level loop of the three parameter sweeps (tl_parjac_column here, parnormal_column and parcolsum_column below), written once:
// the trajectory side, the NP laundered straight lines and the carry hand-over are the skeleton's; what a family does with a
// direction's sensitivities is its End, a plain struct of per-lane state whose hooks are called at fixed points:
//   setup(a, gcol, active)                 after the first lane_setup, before the inactive lanes leave
//   begin(a, c)                            before the level loop
//   level_top(ap, nproma, jk)              at the top of a level, with the look-ahead loads of level jk+1 issued
//   direction(ap, b, nproma, nlev, jk, v)  after level_tl of direction b: v = its sensitivities of level jk (ap: the loop's laundered
//                                          argument block, by reference, so that an End launders THAT pointer again before it stores)
//   level_end()                            after the level's last direction
//   column_end(a, gcol)                    after the last level
// and whose PaceT says at compile time whether the sweep is paced (Pace) or not (NoPace).
struct NoPace {
  C2_HD void begin(GeomP) {}
  C2_HD void nap() {}
};

// F: C2F_QSAT (otherwise the trajectory's SATUR is evaluated in the sweep) | C2F_PRECISE | C2F_EVAP | C2F_OFF32 (| bits of the End's own)
// ArgsP: pointer to an argument block with c g s in par tab
template <unsigned F, class ArgsP, class End>
C2_HD void par_sweep(long long gcol, ArgsP a, End& e) {
  constexpr bool HAS_QSAT = (F & C2F_QSAT) != 0, P = (F & C2F_PRECISE) != 0, EVAP = (F & C2F_EVAP) != 0;
  constexpr int NP = parjac_directions(F);
  typedef typename std::conditional<(F & C2F_OFF32) != 0, unsigned, long long>::type OT;
  LaneOff o; bool active;
  if (!lane_setup(&a->g, &a->s, gcol, o, active)) return;
  e.setup(a, gcol, active);
  if (!active) return;
  const int nlev = a->g.nlev, nproma = a->g.nproma;
  LevelTabP tab = (LevelTabP)a->tab;
  ConstsP c = C2_CONSTS(a);
  InPtrsP in = &a->in;

  // once per column, not once per direction: the tropopause pre-scan, the critical-humidity setup, the lane offsets, the loads
  real_t ztrpaus = tropopause<false>(c, tab, in, o, &a->g, RC(0.0));
  RhCrit rh;
  rhcrit_setup(ztrpaus, rh);
  real_t paph_surf = RC(0.0);
  if (EVAP) paph_surf = in->paph[o.half + (long long)nlev * nproma];

  Carry cy; C2_ZERO_CARRY(cy);
  Carry dcy[NP];
#pragma unroll
  for (int b = 0; b < NP; ++b) C2_ZERO_CARRY(dcy[b]);
  e.begin(a, c);
  RawLevel cur, nxt;
  real_t paph_k = in->paph[o.half];
  const LaneOffT<OT> ol = lane_off_as<OT>(o);  // offsets used inside the level loop
  load_level<HAS_QSAT>(in, ol, nproma, nlev, 0, cur);
  typename End::PaceT pace;
  pace.begin(&a->g);

  // The trajectory inputs of level jk+1 are requested at the top of level jk, as in tl_column; what else a level reads is its End's.
  for (int jk = 0; jk < nlev; ++jk) {
    const bool last = (jk == nlev - 1);
    ArgsP ap = a;
    C2_LAUNDER(ap);
    nxt = cur;
    if (!last) load_level<HAS_QSAT>(&ap->in, ol, nproma, nlev, jk + 1, nxt);
    e.level_top(ap, nproma, jk);
    pace.nap();  // (with the loads in flight)
    if (!HAS_QSAT) cur.qsat = satur_point<P>(c, cur.pap, cur.t);  // (once per level: every direction gets its own opaque copy)

    LevelCst k;
    level_cst(tab, jk, last, k);
    LevelIn x;
    make_level_in(cur, paph_k, paph_surf, x);
    Carry cy_out = cy;
#pragma unroll
    for (int b = 0; b < NP; ++b) {
      // this direction's own straight line (launder_level says why): every direction leaves the same trajectory carry
      LevelIn xb = x;
      LevelCst kb = k;
      RhCrit rhb = rh;
      cy_out = cy;
      launder_level(xb, kb, cy_out);
      C2_LAUNDER_V(xb.paph_surf); C2_LAUNDER_V(rhb.zeta3); C2_LAUNDER_V(rhb.zrh2); C2_LAUNDER_V(rhb.zdeta1);
      ConstsP cb = c;  // (and its own view of the constants: a product of two of them is shared otherwise)
      C2_LAUNDER(cb);
      LevelTraj tr;
      LevelOut lo;
      level_forward<P, EVAP>(cb, kb, rhb, xb, cy_out, tr, lo);
      LevelIn dx;
      zero_level_in<EVAP>(dx);
      LevelOut dlo;
      C2_LAUNDER(ap);
      level_tl<true>(cb, kb, xb, tr, dx, dcy[b], dlo, &ap->par[b]);
      e.direction(ap, b, nproma, nlev, jk, dlo);
    }
    e.level_end();
    cy = cy_out;
    paph_k = cur.paph_k1;
    cur = nxt;
  }
  e.column_end(a, gcol);
}

// the Jacobian's End: direction b's sensitivities of a level go to its planes dout[b], addressed with the block strides sp
template <unsigned F>
struct ParJacEnd {
  typedef Pace PaceT;
  typedef typename std::conditional<(F & C2F_OFF32) != 0, unsigned, long long>::type OT;
  LaneOff op;
  LaneOffT<OT> opl;  // (op as used inside the level loop)
  C2_HD void setup(TlParJacArgsP a, long long gcol, bool& active) { lane_setup(&a->g, &a->sp, gcol, op, active); }
  C2_HD void begin(TlParJacArgsP a, ConstsP c) {
#pragma unroll
    for (int b = 0; b < parjac_directions(F); ++b) store_top(&a->dout[b], op, c);
    opl = lane_off_as<OT>(op);
  }
  C2_HD void level_top(TlParJacArgsP, int, int) {}
  C2_HD void direction(TlParJacArgsP& ap, int b, int nproma, int, int jk, const LevelOut& dlo) {
    C2_LAUNDER(ap);
    store_out(&ap->dout[b], opl, nproma, jk, dlo);
  }
  C2_HD void level_end() {}
  C2_HD void column_end(TlParJacArgsP, long long) {}
};

template <unsigned F>
C2_HD void tl_parjac_column(long long gcol, TlParJacArgsP a) {
  static_assert(!(F & ~(C2F_QSAT | C2F_PRECISE | C2F_EVAP | C2F_OFF32)), "flags of the parameter-Jacobian sweep: QSAT, PRECISE, EVAP, OFF32");
  ParJacEnd<F> e;
  par_sweep<F>(gcol, a, e);
}

// ---------------------------------------------------------------------------------------------------------
// The Gauss-Newton normal equations of the parameters in one sweep: H = J^T W J and g = J^T W r (cloudsc2_parnormal_launch)
// ---------------------------------------------------------------------------------------------------------
// A Gauss-Newton or Levenberg-Marquardt step needs the 4 x 4 matrix H and the 4-vector g, never J = d out / d p itself.  This sweep
// is tl_parjac_column's (par_sweep) with the stores replaced by sums: the NP sensitivities of a level stay in registers, the level's residual r
// (model - observation) and diagonal weight w of every observed output are read, and the lane accumulates, in double in both
// builds, H[a][b] += (w J_a) J_b for a <= b and g[a] += (w J_a) r.  The order of every sum is fixed -- levels outermost, outputs in
// the order of struct cloudsc2_outputs -- and a lane's sums go to row `normal_row` of `work`, which a second kernel folds over the
// columns in a fixed order (par_fold_kernel's): the same bits from run to run, no atomics.
// An output is observed when its residual pointer is not NULL; a NULL weight pointer is weight 1.  Both are wave-uniform run-time
// branches on the argument block, not variants.  clc and covptot depend on none of the parameters: their sensitivities are exact
// zeros, so their planes are not read at all.  Half level 0 of the four fluxes is the zero flux of the model top (store_top): its
// sensitivity is zero and its residual and weight are not read either.
constexpr int normal_sums(int np) { return np * (np + 1) / 2 + np; }
// row of H[a][b] (a <= b) and of g[a] in `work` and in the result: the upper triangle of the PAR_COUNT x PAR_COUNT matrix row by row,
// then g -- whatever the sweep's direction count, so that without the evaporation branch the rows with rpecons are simply not written
constexpr int normal_row_h(int a, int b) { return a * PAR_COUNT - a * (a - 1) / 2 + (b - a); }
constexpr int normal_row_g(int a) { return PAR_COUNT * (PAR_COUNT + 1) / 2 + a; }
constexpr int kNormalObs = 8;  // the outputs that depend on a parameter: tent tenq tenl teni fplsl fplsn fhpsl fhpsn
// THE list of them, in the order of struct cloudsc2_outputs: X(index, C2O_* bit, OutPtrs member, 1 on half levels (half level 0 is
// store_top's zero) / 0 on full levels, row of the column-sum table).  Every list of these outputs below expands from it.
#define C2_PAR_OUTPUTS(X)                                                                                 \
  X(0, C2O_TENT, tent, 0, 0) X(1, C2O_TENQ, tenq, 0, 1) X(2, C2O_TENL, tenl, 0, 2) X(3, C2O_TENI, teni, 0, 3) \
  X(4, C2O_FPLSL, fplsl, 1, 5) X(5, C2O_FPLSN, fplsn, 1, 6) X(6, C2O_FHPSL, fhpsl, 1, 7) X(7, C2O_FHPSN, fhpsn, 1, 8)

// (par from the launch's direction count on is not read; resid / weight: read only, NULL members as above; sr: their block strides)
struct ParNormalArgs {
  Consts c; Geom g; Strides s, sr; InPtrs in; OutPtrs resid, weight; ParLin par[kBatchMax]; const LevelTab* tab;
  double* work;  // (normal_sums(PAR_COUNT), ncols_pad) doubles: every active lane's sums (the padded tail is not written)
};
typedef const C2_CONST_AS ParNormalArgs* ParNormalArgsP;

// residual and weight of one level, in the order of kNormalObs; an unobserved output's pair is not read
struct ObsLevel {
  real_t r[kNormalObs], w[kNormalObs];
};
C2_HD void load_obs_one(const real_t* r, const real_t* w, long long i, real_t& rv, real_t& wv) {
  rv = RC(0.0);
  wv = RC(1.0);
  if (r) {
    rv = ldg(r, i);
    if (w) wv = ldg(w, i);
  }
}
C2_HD void load_obs(ParNormalArgsP ap, const LaneOff& o, int nproma, int jk, ObsLevel& v) {
  const OutPtrs r = ap->resid, w = ap->weight;
  const long long d = level_off(0LL, jk, nproma), d1 = d + row_off(0LL, nproma);
#define C2_X(n, bit, field, half_level, row) load_obs_one(r.field, w.field, half_level ? o.half + d1 : o.loc + d, v.r[n], v.w[n]);
  C2_PAR_OUTPUTS(C2_X)
#undef C2_X
}

// one lane's sums: the upper triangle of its NP x NP block row by row, and g
template <int NP>
struct NormalAcc {
  double h[NP * (NP + 1) / 2], g[NP];
  C2_HD void zero() {
#pragma unroll
    for (int b = 0; b < NP; ++b) g[b] = 0.0;
#pragma unroll
    for (int i = 0; i < NP * (NP + 1) / 2; ++i) h[i] = 0.0;
  }
  // the lane's sums to `work`: consecutive lanes, consecutive doubles of each row (col < ngptot <= ncols_pad = np)
  C2_HD void store(double* work, long long np, long long col) const {
#pragma unroll
    for (int ia = 0; ia < NP; ++ia) {
#pragma unroll
      for (int ib = ia; ib < NP; ++ib) work[normal_row_h(ia, ib) * np + col] = h[ia * NP - ia * (ia - 1) / 2 + (ib - ia)];
      work[normal_row_g(ia) * np + col] = g[ia];
    }
  }
};
// one output of one level: j[a] = its sensitivity to parameter a.  The operands are converted before the products (fp32 build).
template <int NP>
C2_HD void normal_add(NormalAcc<NP>& acc, const real_t (&j)[NP], real_t r, real_t w) {
  double jd[NP];
#pragma unroll
  for (int a = 0; a < NP; ++a) jd[a] = (double)j[a];
  const double rd = (double)r, wd = (double)w;
#pragma unroll
  for (int a = 0; a < NP; ++a) {
    const double wj = wd * jd[a];
#pragma unroll
    for (int b = a; b < NP; ++b) acc.h[a * NP - a * (a - 1) / 2 + (b - a)] += wj * jd[b];
    acc.g[a] += wj * rd;
  }
}

// The sensitivities of one direction, opaque: the empty asm statements are ordered among themselves, so a direction's eight results
// exist before the next direction's inputs are laundered.  Without this the compiler interleaves the NP straight lines, which have no
// store between them here, and holds their intermediate values all at once (fp64: scratch in six of the eight forms).
C2_HD void launder_sens(LevelOut& v) {
  C2_LAUNDER_V(v.tent); C2_LAUNDER_V(v.tenq); C2_LAUNDER_V(v.tenl); C2_LAUNDER_V(v.teni);
  C2_LAUNDER_V(v.fplsl); C2_LAUNDER_V(v.fplsn); C2_LAUNDER_V(v.fhpsl); C2_LAUNDER_V(v.fhpsn);
}

// the normal equations' End (par_sweep).  The residuals and weights of level jk are requested at its top, with the trajectory inputs of
// level jk+1: they are used after the level's NP directions and are in flight under that arithmetic.
template <unsigned F>
struct ParNormalEnd {
  static constexpr int NP = parjac_directions(F);
  typedef NoPace PaceT;
  LaneOff orw;
  unsigned obs;  // which outputs are observed, bit n of C2_PAR_OUTPUTS (wave-uniform: the pointers are the argument block's)
  ObsLevel ob;
  LevelOut dlo[NP];
  NormalAcc<NP> acc;
  C2_HD void setup(ParNormalArgsP a, long long gcol, bool& active) { lane_setup(&a->g, &a->sr, gcol, orw, active); }
  C2_HD void begin(ParNormalArgsP a, ConstsP) {
    const OutPtrs r = a->resid;
#define C2_X(n, bit, field, half_level, row) | (r.field ? 1u << n : 0u)
    obs = 0u C2_PAR_OUTPUTS(C2_X);
#undef C2_X
    acc.zero();
  }
  C2_HD void level_top(ParNormalArgsP ap, int nproma, int jk) { load_obs(ap, orw, nproma, jk, ob); }
  C2_HD void direction(ParNormalArgsP&, int b, int, int, int, const LevelOut& v) {
    dlo[b] = v;
    launder_sens(dlo[b]);
  }
  // the level's contributions, output by output in the order of struct cloudsc2_outputs (clc and covptot: exact zeros, skipped)
  C2_HD void level_end() {
#define C2_X(n, bit, field, half_level, row)                            \
  if (obs & (1u << n)) {                                                \
    real_t j[NP];                                                       \
    _Pragma("unroll") for (int b = 0; b < NP; ++b) j[b] = dlo[b].field; \
    normal_add<NP>(acc, j, ob.r[n], ob.w[n]);                           \
  }
    C2_PAR_OUTPUTS(C2_X)
#undef C2_X
  }
  C2_HD void column_end(ParNormalArgsP a, long long gcol) { acc.store(a->work, a->g.ncols_pad, gcol); }
};

// F: C2F_QSAT (otherwise the trajectory's SATUR is evaluated in the sweep) | C2F_PRECISE | C2F_EVAP; 64-bit offsets always
template <unsigned F>
C2_HD void parnormal_column(long long gcol, ParNormalArgsP a) {
  static_assert(!(F & ~(C2F_QSAT | C2F_PRECISE | C2F_EVAP)), "flags of the normal-equations sweep: QSAT, PRECISE, EVAP");
  ParNormalEnd<F> e;
  par_sweep<F>(gcol, a, e);
}

// ---------------------------------------------------------------------------------------------------------
// The parameter Jacobian and the normal equations of the COLUMN SUMS in one sweep (cloudsc2_parjac_launch_colsum,
// cloudsc2_parnormal_launch_colsum)
// ---------------------------------------------------------------------------------------------------------
// A cloud scheme is confronted with column sums y_n[c] = sum_k w_n[k] out_n[k, c] (surface rain and snow, column-integrated heating).
// Their sensitivities s[a][n][c] = sum_k w_n[k] (d out_n / d p_a)[k, c] need nothing but tl_parjac_column's level loop: this sweep is
// that loop (par_sweep) with store_out replaced by a fold of direction a's sensitivities into the lane's accumulators acc[a][n], the fold of
// ColsumAcc::add to the bit: acc = fl(acc + fl(w_n[k] J)), the level's sensitivities pinned before the fold and the product laundered
// before its add, half level 0 of a flux skipped.  No sensitivity plane exists.  clc and covptot depend on no parameter: they have no
// accumulator and their rows of the table are not read.  The accumulators live in LDS, one slot per lane, direction and sum (up to
// 4 x 8 fp64 values: kept in registers the kernels take 45-55 registers more, in LDS fewer than tl_parjac_kernel; neither form uses
// scratch -- DESIGN.md 3.6): a lane touches its own slots only, so there is no barrier.  The host builds keep them in an array.
// The end of the column has two forms (C2F_NORMAL):
//   sums form    s[a][n] stored for every run parameter a and every sum n of the mask into (nblocks, nproma) arrays addressed as in
//                colsum_off (y[a]); the padded tail is not written; a clc or covptot array present receives its exact zero.
//   normal form  the column's residual r_n[c] and diagonal weight of every observed sum are read from (nblocks, nproma) arrays (y[0],
//                y[1]; a NULL weight is weight 1) and normal_add<NP> is called with j[a] = s[a][n] for the observed n in the order of
//                OutPtrs; the 14 (or 9) doubles go to `work` as in parnormal_column, for the same fold over the columns.
constexpr unsigned C2F_NORMAL = 8u;  // this sweep only: the normal-equations end of the column
// (par and y from the launch's direction count on are not read)
struct ParColsumArgs {
  Consts c; Geom g; Strides s; InPtrs in; ParLin par[kBatchMax]; const LevelTab* tab;
  ColsumTab cs;          // w: the table; y: not used; stride: the block stride of every (nblocks, nproma) array; mask: the sums present / observed
  OutPtrs y[kBatchMax];  // sums form: the sums of direction b, written; normal form: y[0] the residuals, y[1] the weights, read only
  double* work;          // normal form: (normal_sums(PAR_COUNT), ncols_pad) doubles, as ParNormalArgs::work
};
typedef const C2_CONST_AS ParColsumArgs* ParColsumArgsP;

template <int NP>
struct ParColsumAcc {
#if defined(__HIP_DEVICE_COMPILE__)
  real_t* s;  // this lane's slot of (direction 0, sum 0); (b, n) is (b * kNormalObs + n) * kColsumLanes further
  __device__ __forceinline__ void begin() {
    __shared__ real_t slots[NP * kNormalObs * kColsumLanes];
    s = slots + threadIdx.x;
#pragma unroll
    for (int i = 0; i < NP * kNormalObs; ++i) s[i * kColsumLanes] = RC(0.0);
  }
  // the lane's column once more after the level loop, as ColsumAcc::column(): no register holds it through the loop
  __device__ __forceinline__ long long column(long long) const { return (long long)blockIdx.x * kColsumLanes + threadIdx.x; }
  __device__ __forceinline__ real_t get(int b, int n) const { return s[(b * kNormalObs + n) * kColsumLanes]; }
  __device__ __forceinline__ void set(int b, int n, real_t v) { s[(b * kNormalObs + n) * kColsumLanes] = v; }
#else
  real_t s[NP * kNormalObs];
  void begin() {
    for (int i = 0; i < NP * kNormalObs; ++i) s[i] = RC(0.0);
  }
  long long column(long long gcol) const { return gcol; }
  real_t get(int b, int n) const { return s[b * kNormalObs + n]; }
  void set(int b, int n, real_t v) { s[b * kNormalObs + n] = v; }
#endif
  C2_HD void add(int b, int n, real_t w, real_t v) {  // (ColsumAcc::add)
    real_t p = w * v;
    C2_LAUNDER_V(p);
    set(b, n, get(b, n) + p);
  }
};

// one level's sensitivities of direction b into its sums of mask m: colsum_fold without the two outputs that depend on no parameter
template <int NP>
C2_HD void parcolsum_fold(ParColsumAcc<NP>& acc, int b, ColsumTabP cs, unsigned m, int nlev, int jk, LevelOut v) {
  C2_PIN_V(v.tent); C2_PIN_V(v.tenq); C2_PIN_V(v.tenl); C2_PIN_V(v.teni); C2_PIN_V(v.clc);
  C2_PIN_V(v.covptot); C2_PIN_V(v.fplsl); C2_PIN_V(v.fplsn); C2_PIN_V(v.fhpsl); C2_PIN_V(v.fhpsn);
  const ColsumRowP w = (ColsumRowP)cs->w + jk;
  const int r = nlev + 1;
#define C2_X(n, bit, field, half_level, row) if (m & bit) acc.add(b, n, w[row * r + half_level], v.field);
  C2_PAR_OUTPUTS(C2_X)
#undef C2_X
}

// the column sums' End (par_sweep): nothing but the trajectory is read in the level loop
template <unsigned F>
struct ParColsumEnd {
  static constexpr int NP = parjac_directions(F);
  typedef NoPace PaceT;
  ParColsumAcc<NP> acc;
  C2_HD void setup(ParColsumArgsP, long long, bool&) {}
  C2_HD void begin(ParColsumArgsP, ConstsP) { acc.begin(); }
  C2_HD void level_top(ParColsumArgsP, int, int) {}
  C2_HD void direction(ParColsumArgsP& ap, int b, int, int nlev, int jk, const LevelOut& dlo) {
    C2_LAUNDER(ap);
    parcolsum_fold<NP>(acc, b, &ap->cs, ap->cs.mask, nlev, jk, dlo);
  }
  C2_HD void level_end() {}
  C2_HD void column_end(ParColsumArgsP a, long long gcol) {
    const unsigned m = a->cs.mask;
    const long long col = acc.column(gcol);
    const long long ocs = colsum_off(&a->g, &a->cs, col);
    if constexpr (!(F & C2F_NORMAL)) {
      // one row per run parameter and sum present (clc, covptot: the exact zero)
#pragma unroll
      for (int b = 0; b < NP; ++b) {
        const OutPtrs y = a->y[b];
#define C2_X(n, bit, field, half_level, row) if (m & bit) y.field[ocs] = acc.get(b, n);
        C2_PAR_OUTPUTS(C2_X)
#undef C2_X
        if (m & C2O_CLC) y.clc[ocs] = RC(0.0);
        if (m & C2O_COVPTOT) y.covptot[ocs] = RC(0.0);
      }
    } else {
      NormalAcc<NP> na;
      na.zero();
      const OutPtrs r = a->y[0], w = a->y[1];
      // the observed sums in the order of struct cloudsc2_outputs (clc and covptot: exact zeros, their residuals are not read)
#define C2_X(n, bit, field, half_level, row)                              \
  if (m & bit) {                                                          \
    real_t j[NP], rv, wv;                                                 \
    _Pragma("unroll") for (int b = 0; b < NP; ++b) j[b] = acc.get(b, n);  \
    load_obs_one(r.field, w.field, ocs, rv, wv);                          \
    normal_add<NP>(na, j, rv, wv);                                        \
  }
      C2_PAR_OUTPUTS(C2_X)
#undef C2_X
      na.store(a->work, a->g.ncols_pad, col);
    }
  }
};

// F: C2F_QSAT (otherwise the trajectory's SATUR is evaluated in the sweep) | C2F_PRECISE | C2F_EVAP | C2F_OFF32 | C2F_NORMAL
template <unsigned F>
C2_HD void parcolsum_column(long long gcol, ParColsumArgsP a) {
  static_assert(!(F & ~(C2F_QSAT | C2F_PRECISE | C2F_EVAP | C2F_OFF32 | C2F_NORMAL)),
                "flags of the parameter column-sum sweep: QSAT, PRECISE, EVAP, OFF32, NORMAL");
  ParColsumEnd<F> e;
  par_sweep<F>(gcol, a, e);
}

// F: C2F_QSAT (always) | C2F_PRECISE | C2F_EVAP | C2F_OFF32; the form is ad_reverse_column's C2F_ASSIGN | C2F_VJP: input adjoints
// assigned, output adjoints read only, the PSUPSAT adjoint ax.q, the PLU(1) adjoint zero, the padded tail untouched
template <unsigned F, int NB>
C2_HD void vjp_batch_column(long long gcol, VjpBatchArgsP a) {
  static_assert(NB >= 1 && NB <= kBatchMax, "directions of one launch: 1..kBatchMax");
  constexpr bool P = (F & C2F_PRECISE) != 0, EVAP = (F & C2F_EVAP) != 0, OFF32 = (F & C2F_OFF32) != 0;
  static_assert((F & C2F_QSAT) && !(F & ~(C2F_QSAT | C2F_PRECISE | C2F_EVAP | C2F_OFF32)), "flags of the batched reverse sweep: QSAT, PRECISE, EVAP, OFF32");
  typedef typename std::conditional<OFF32, unsigned, long long>::type OT;
  LaneOff o, oa64; bool active;
  if (!lane_setup(&a->nl.g, &a->nl.s, gcol, o, active)) return;
  lane_setup(&a->nl.g, &a->sa, gcol, oa64, active);
  if (!active) return;
  const int nlev = a->nl.g.nlev, nproma = a->nl.g.nproma;
  LevelTabP tab = (LevelTabP)a->nl.tab;
  ConstsP c = C2_CONSTS(&a->nl);
  InPtrsP in = &a->nl.in;

  const long long osc64 = (gcol / nproma) * ((long long)nproma * nlev) + (gcol % nproma);  // scratch: (NPROMA, NLEV, NBLOCKS) contiguous
  const LaneOffT<OT> ol = lane_off_as<OT>(o), oa = lane_off_as<OT>(oa64);
  const OT osc = (OT)(osc64 * (OFF32 ? (long long)sizeof(real_t) : 1));

  real_t ztrpaus = tropopause<false>(c, tab, in, o, &a->nl.g, RC(0.0));
  RhCrit rh;
  rhcrit_setup(ztrpaus, rh);
  const real_t paph_bottom = in->paph[o.half + (long long)nlev * nproma];
  const real_t paph_surf = EVAP ? paph_bottom : RC(0.0);

  Carry acy[NB];
  real_t paph_pending[NB], surf_acc[NB];  // as in ad_reverse_column, per direction
  // what is invariant over the levels is laundered per direction HERE, not per level: ad_reverse_column's compiler knows it to be
  // invariant too, and forms what depends on it alone before the level loop
  RhCrit rh_b[NB];
  real_t paph_surf_b[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    C2_ZERO_CARRY(acy[b]);
    paph_pending[b] = RC(0.0); surf_acc[b] = RC(0.0);
    rh_b[b] = rh; paph_surf_b[b] = paph_surf;
    C2_LAUNDER_V(rh_b[b].zeta3); C2_LAUNDER_V(rh_b[b].zrh2); C2_LAUNDER_V(rh_b[b].zdeta1); C2_LAUNDER_V(paph_surf_b[b]);
  }
  real_t paph_k1 = paph_bottom;
  // the assign form adds its results to old values that are zero (ad_load_level: xo); 0 + x is x except for x = -0, which becomes +0:
  // the add is kept so that the bits are ad_reverse_column's
  const real_t zero = RC(0.0);
  Pace pace;
  pace.begin(&a->nl.g);
  for (int jk = nlev - 1; jk >= 0; --jk) {
    const bool last = (jk == nlev - 1);
    pace.nap();
    const OT d = level_off(OT(), jk, nproma);
    const OT d1 = d + row_off(OT(), nproma);
    VjpBatchArgsP ap = a;
    C2_LAUNDER(ap);
    // the trajectory loads of the level and the first direction's output adjoints at its top, as in ad_reverse_column; the output
    // adjoints of direction b + 1 under level_ad of direction b
    RawLevel cur;
    real_t paph_k;
    Carry cy;
    load_reverse_traj<true, EVAP>(&ap->nl, ol, osc, d, d1, last, cur, paph_k, cy);
    LevelOut ycur;
    load_out_adjoint(&ap->aout[0], oa, d, d1, ycur);
    cur.paph_k1 = paph_k1;

    LevelCst k;
    level_cst(tab, jk, last, k);
    LevelIn x;
    make_level_in(cur, paph_k, paph_surf, x);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      {
        LevelOut ynxt = ycur;
        if (b + 1 < NB) load_out_adjoint(&ap->aout[b + 1 < NB ? b + 1 : b], oa, d, d1, ynxt);
        // this direction's own straight line (launder_level says why)
        LevelIn xb = x;
        LevelCst kb = k;
        RhCrit rhb = rh_b[b];
        Carry cyb = cy;
        launder_level(xb, kb, cyb);
        xb.paph_surf = paph_surf_b[b];
        ConstsP cb = c;  // (and its own view of the constants: a product of two of them is shared otherwise)
        C2_LAUNDER(cb);
        LevelTraj tr;
        LevelOut lo;
        level_forward<P, EVAP>(cb, kb, rhb, xb, cyb, tr, lo);
        LevelOut ya = ycur;  // enthalpy-flux adjoints folded in (cloudsc2ad.F90:914-921)
        ya.fplsn = ya.fplsn - ya.fhpsn * cb->rlstt;
        ya.fplsl = ya.fplsl - ya.fhpsl * cb->rlvtt;
        LevelIn ax;
        level_ad(cb, kb, xb, tr, ya, acy[b], ax);

        C2_LAUNDER(ap);
        const InPtrsRW px = ap->ain[b];
        stg(px.pap, oa.full + d, zero + ax.pap);
        stg(px.q, oa.full + d, zero + ax.q);
        stg(px.qsat, oa.full + d, zero + ax.qs);
        stg(px.t, oa.full + d, zero + ax.t);
        stg(px.l, oa.clv + d, zero + ax.l);
        stg(px.i, oa.clv + d, zero + ax.i);
        stg(px.lude, oa.full + d, zero + ax.lude);
        stg(px.mfu, oa.full + d, zero + ax.mfu);
        stg(px.mfd, oa.full + d, zero + ax.mfd);
        stg(px.gt, oa.cml + d, zero + ax.gt);
        stg(px.gq, oa.cml + d, zero + ax.gq);
        stg(px.gl, oa.cml + d, zero + ax.gl);
        stg(px.gi, oa.cml + d, zero + ax.gi);
        stg(px.supsat, oa.full + d, ax.q);  // the true derivative (C2F_VJP)
        if (!last) stg(px.lu, oa.full + d1, zero + ax.lu_k1);
        surf_acc[b] += ax.paph_surf;
        if (last) {
          surf_acc[b] += ax.paph_k1;
        } else {
          stg(px.paph, oa.half + d1, zero + (ax.paph_k1 + paph_pending[b]));
        }
        paph_pending[b] = ax.paph_k;
        ycur = ynxt;
      }
    }
    paph_k1 = paph_k;
  }
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    {
      const InPtrsRW px = a->ain[b];
      px.paph[oa64.half] = paph_pending[b];
      px.paph[oa64.half + (long long)nlev * nproma] = surf_acc[b];
      px.lu[oa64.full] = RC(0.0);  // PLU(1) has no adjoint contribution
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// Adjoint-test norms per column (cloudsc_driver_ad_mod.F90:184-195,240-264)
// ---------------------------------------------------------------------------------------------------------
// norm1 = <y,y>, field by field like the reference's SUMs (:185-194)
C2_HD double adjoint_norm1_column(int nlev, int nproma, const LaneOff& oa, const OutPtrs& y) {
  double st = 0, sq = 0, sl = 0, si = 0, sc = 0, sfl = 0, sfn = 0, shl = 0, shn = 0, scv = 0;
  for (int jk = 0; jk < nlev; ++jk) {
    long long d = (long long)jk * nproma;
    double v;
    v = y.tent[oa.loc + d]; st += v * v;
    v = y.tenq[oa.loc + d]; sq += v * v;
    v = y.tenl[oa.loc + d]; sl += v * v;
    v = y.teni[oa.loc + d]; si += v * v;
    v = y.clc[oa.full + d]; sc += v * v;
    v = y.covptot[oa.full + d]; scv += v * v;
  }
  for (int jk = 0; jk <= nlev; ++jk) {
    long long d = (long long)jk * nproma;
    double v;
    v = y.fplsl[oa.half + d]; sfl += v * v;
    v = y.fplsn[oa.half + d]; sfn += v * v;
    v = y.fhpsl[oa.half + d]; shl += v * v;
    v = y.fhpsn[oa.half + d]; shn += v * v;
  }
  return st + sq + sl + si + sc + sfl + sfn + shl + shn + scv;
}

// norm2 = <x0, x_adj> with x0 = 0.01 * trajectory inputs; ZSUPSAT0 = 0 (:139,157) so that term vanishes
C2_HD double adjoint_norm2_column(int nlev, int nproma, const LaneOff& o, const LaneOff& oa, long long oq, const InPtrs& in,
                                  const real_t* qsat, const InPtrs& xa) {
  double s_aph = 0, s_ap = 0, s_q = 0, s_qs = 0, s_t = 0, s_l = 0, s_i = 0, s_lude = 0, s_lu = 0, s_mfu = 0, s_mfd = 0, s_gt = 0,
         s_gq = 0, s_gl = 0, s_gi = 0;
  for (int jk = 0; jk <= nlev; ++jk) {
    long long d = (long long)jk * nproma;
    s_aph += (in.paph[o.half + d] * 0.01) * xa.paph[oa.half + d];
  }
  for (int jk = 0; jk < nlev; ++jk) {
    long long d = (long long)jk * nproma;
    s_ap += (in.pap[o.full + d] * 0.01) * xa.pap[oa.full + d];
    s_q += (in.q[o.full + d] * 0.01) * xa.q[oa.full + d];
    s_qs += (qsat[oq + d] * 0.01) * xa.qsat[oa.full + d];
    s_t += (in.t[o.full + d] * 0.01) * xa.t[oa.full + d];
    s_l += (in.l[o.clv + d] * 0.01) * xa.l[oa.clv + d];
    s_i += (in.i[o.clv + d] * 0.01) * xa.i[oa.clv + d];
    s_lude += (in.lude[o.full + d] * 0.01) * xa.lude[oa.full + d];
    s_lu += (in.lu[o.full + d] * 0.01) * xa.lu[oa.full + d];
    s_mfu += (in.mfu[o.full + d] * 0.01) * xa.mfu[oa.full + d];
    s_mfd += (in.mfd[o.full + d] * 0.01) * xa.mfd[oa.full + d];
    s_gt += (in.gt[o.cml + d] * 0.01) * xa.gt[oa.cml + d];
    s_gq += (in.gq[o.cml + d] * 0.01) * xa.gq[oa.cml + d];
    s_gl += (in.gl[o.cml + d] * 0.01) * xa.gl[oa.cml + d];
    s_gi += (in.gi[o.cml + d] * 0.01) * xa.gi[oa.cml + d];
  }
  return s_aph + s_ap + s_q + s_qs + s_t + s_l + s_i + s_lude + s_lu + s_mfu + s_mfd + s_gt + s_gq + s_gl + s_gi + 0.0;
}

// "machine precision is defined here as strictly 64bits" (cloudsc_driver_ad_mod.F90:258-264): EPSILON(1._8) whatever
// JPRB is, so the fp32 build reports its error in the same unit as the reference's -DSINGLE binary does.
C2_HD double adjoint_norm3(double n1, double n2) {
  const double eps = 2.220446049250313e-16;  // EPSILON(1._8)
  if (n2 == 0.0) return fabs(n1 - n2) / eps;
  return fabs(n1 - n2) / eps / n2;
}

}  // namespace cloudsc2
