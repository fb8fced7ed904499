// TEST-ONLY: the column sums of an ensemble's members (C2F_MEMBER: what cloudsc2_nl_launch_ens_colsum / cloudsc2_tl_launch_ens_colsum /
// cloudsc2_vjp_launch_ens_colsum run) compiled for the HOST, on top of hostcheck_colsum.hip, whose column-sum sweeps -- and, below it,
// the dense and sparse ones -- are the references of the same library.  The members' blocks are made by ens_member_args from one
// template, exactly as ens_args_kernel makes them.  An absent sum, gradient or tangent is a NULL pointer; the reverse sweep may be given
// NO gradient plane at all (the parameter adjoints alone): a guard that is missing in the column functions dereferences NULL here, on the
// CPU.  Like hostcheck.hip, never loaded by the package.
#include "hostcheck_colsum.hip"

template <unsigned F> struct HcEnsColsumNl {
  static void run(long long gc, const NlColsumArgs* a) {
    if constexpr ((F & ~(C2F_QSAT | C2F_PRECISE | C2F_EVAP | C2F_CKPT | C2F_OFF32)) == 0 && hc_sparse_built((F & C2F_OFF32) ? 8u : 0u))
      nl_column<F | C2F_COLSUM | C2F_MEMBER>(gc, &a->a);
  }
};
template <unsigned I> struct HcEnsColsumTl {
  static void run(long long gc, const TlEnsColsumArgs* a) {
    if constexpr (hc_sparse_built(I) && (I & 16u)) tl_column<hc_sparse_flags(I) | C2F_COLSUM | C2F_PARLIN | C2F_MEMBER>(gc, &a->a.a.a);
  }
};
template <unsigned I> struct HcEnsColsumVjp {
  static void run(long long gc, const AdEnsColsumArgs* a) {
    if constexpr (hc_sparse_built(I) && (I & 16u))
      ad_reverse_column<hc_sparse_flags(I) | C2F_ASSIGN | C2F_VJP | C2F_COLSUM | C2F_PARLIN>(gc, &a->a.a.a);
  }
};

static EnsStrides hc_ens_strides(const long long* in, const long long* out, const long long* in2, const long long* out2, long long ckpt) {
  EnsStrides ms;
  for (int i = 0; i < kNumIn; ++i) { ms.in[i] = in ? in[i] : 0; ms.in2[i] = in2 ? in2[i] : 0; }
  for (int i = 0; i < kNumOut; ++i) { ms.out[i] = out ? out[i] : 0; ms.out2[i] = out2 ? out2[i] : 0; }
  ms.ckpt = ckpt;
  return ms;
}

extern "C" {

// params: (members, 4) doubles; *_mstride: member strides in elements per field (NULL: shared); keep NULL: the lean form
int hostcheck_enscolsum_nl(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, int members, const double* params,
                           const cloudsc2_inputs* in, const long long* in_mstride, const cloudsc2_real* weights, const cloudsc2_outputs* sums,
                           const long long* sums_mstride, const cloudsc2_outputs* keep, const long long* keep_mstride, cloudsc2_real* scratch,
                           long long scratch_mstride) {
  NlColsumArgs ca;
  memset(&ca, 0, sizeof(ca));
  NlArgs& a = ca.a;
  a.g = hc_geom(nproma, nlev, ngptot);
  a.c = hc_consts(*prm, ptsphy);
  LevelTab tab; hc_tables(*prm, tab, a.g);
  a.tab = &tab;
  hc_in(*in, a.s, a.in);
  if (!hc_colsum_tab(weights, *sums, ca.cs)) return -1;
  if (keep) { a.out.fplsl = keep->fplsl.ptr; a.out.fplsn = keep->fplsn.ptr; }
  a.ckpt = (keep && a.c.evap) ? scratch : nullptr;
  const unsigned f = (in->qsat.ptr ? C2F_QSAT : 0u) | (g_hc_precise ? C2F_PRECISE : 0u) | (a.c.evap ? C2F_EVAP : 0u) |
                     (keep ? C2F_CKPT : 0u) | (g_hc_off32 ? C2F_OFF32 : 0u);
  const EnsStrides ms = hc_ens_strides(in_mstride, keep ? keep_mstride : nullptr, nullptr, sums_mstride, scratch_mstride);
  for (int k = 0; k < members; ++k) {
    NlColsumArgs mk;
    ens_member_args(mk, ca, ms, ptsphy, k, params + k * PAR_COUNT, nullptr);
    for (long long gc = 0; gc < a.g.ncols_pad; ++gc) hc_dispatch<HcEnsColsumNl, 64>(f, gc, &mk);
  }
  return 0;
}

// dparams: (members, 4) parameter tangents; the field tangents given are the non-NULL fields of din (possibly none)
int hostcheck_enscolsum_tl(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, int satur, int members,
                           const double* params, const double* dparams, const cloudsc2_inputs* in, const long long* in_mstride,
                           const cloudsc2_inputs* din, const long long* din_mstride, const cloudsc2_real* weights,
                           const cloudsc2_outputs* dsums, const long long* sums_mstride) {
  TlEnsColsumArgs ea;
  memset(&ea, 0, sizeof(ea));
  TlColsumArgs& ca = ea.a;
  TlSparseArgs& sa = ca.a;
  TlArgs& a = sa.a;
  a.g = hc_geom(nproma, nlev, ngptot);
  a.c = hc_consts(*prm, ptsphy);
  LevelTab tab; hc_tables(*prm, tab, a.g);
  a.tab = &tab;
  hc_in(*in, a.s, a.in);
  const cloudsc2_outputs none = {};
  unsigned none_mask;
  if (resolve_sparse(*din, none, 'o', a.sp, a.din, a.dout, sa.m.rd, none_mask)) return -1;
  if (!(sa.m.wr = hc_colsum_tab(weights, *dsums, ca.cs))) return -1;
  ea.par = make_parlin(a.c, nullptr);
  const unsigned f = hc_sparse_index(a.c, satur, 1);
  const EnsStrides ms = hc_ens_strides(in_mstride, nullptr, din_mstride, sums_mstride, 0);
  for (int k = 0; k < members; ++k) {
    TlEnsColsumArgs mk;
    ens_member_args(mk, ea, ms, ptsphy, k, params + k * PAR_COUNT, dparams + k * PAR_COUNT);
    for (long long gc = 0; gc < a.g.ncols_pad; ++gc) hc_dispatch<HcEnsColsumTl, 32>(f, gc, &mk);
  }
  return 0;
}

// the gradients wanted are the non-NULL fields of ain (possibly NONE); work: (members, 4, ncols_pad) doubles, written for the active
// columns only; par_adj: (members, 4), the active columns' sums in column order
int hostcheck_enscolsum_vjp(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, int satur, int members,
                            const double* params, const cloudsc2_inputs* in, const long long* in_mstride, const cloudsc2_outputs* out,
                            const long long* out_mstride, const cloudsc2_inputs* ain, const long long* ain_mstride,
                            const cloudsc2_real* weights, const cloudsc2_outputs* ysums, const long long* sums_mstride, cloudsc2_real* scratch,
                            long long scratch_mstride, double* work, double* par_adj) {
  AdEnsColsumArgs ea;
  memset(&ea, 0, sizeof(ea));
  AdColsumArgs& ca = ea.a;
  AdSparseArgs& sa = ca.a;
  AdArgs& a = sa.a;
  a.nl.g = hc_geom(nproma, nlev, ngptot);
  a.nl.c = hc_consts(*prm, ptsphy);
  LevelTab tab; hc_tables(*prm, tab, a.nl.g);
  a.nl.tab = &tab;
  hc_in(*in, a.nl.s, a.nl.in); hc_out(*out, a.nl.s, a.nl.out);
  const cloudsc2_outputs none = {};
  InPtrs ain_c;
  unsigned none_mask;
  if (resolve_sparse(*ain, none, 'i', a.sa, ain_c, a.aout, sa.m.wr, none_mask)) return -1;
  if (!(sa.m.rd = hc_colsum_tab(weights, *ysums, ca.cs))) return -1;
  a.ain = writable(*ain);
  a.nl.ckpt = scratch;
  ea.par = make_parlin(a.nl.c, nullptr);
  ea.work = work;
  const unsigned f = hc_sparse_index(a.nl.c, satur, 1);
  const EnsStrides ms = hc_ens_strides(in_mstride, out_mstride, ain_mstride, sums_mstride, scratch_mstride);
  const long long np = a.nl.g.ncols_pad;
  for (int k = 0; k < members; ++k) {
    AdEnsColsumArgs mk;
    ens_member_args(mk, ea, ms, ptsphy, k, params + k * PAR_COUNT, nullptr);
    if (mk.work != work + (long long)k * PAR_COUNT * np) return -2;
    for (long long gc = 0; gc < np; ++gc) hc_dispatch<HcEnsColsumVjp, 32>(f, gc, &mk);
    for (int i = 0; i < PAR_COUNT; ++i) {
      double s = 0.0;
      for (long long gc = 0; gc < ngptot; ++gc) s += mk.work[i * np + gc];
      par_adj[k * PAR_COUNT + i] = s;
    }
  }
  return 0;
}

// ens_colsum_locate for every thread of a launch of members x wgs_per_member workgroups, in (workgroup, thread) order
void hostcheck_enscolsum_locate(unsigned members, unsigned wgs_per_member, unsigned block, unsigned* member, long long* column) {
  for (unsigned wg = 0; wg < members * wgs_per_member; ++wg)
    for (unsigned t = 0; t < block; ++t)
      ens_colsum_locate(wg, wgs_per_member, members * wgs_per_member, t, block, member[(size_t)wg * block + t], column[(size_t)wg * block + t]);
}

}  // extern "C"
