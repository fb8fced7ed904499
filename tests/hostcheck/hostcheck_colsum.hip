// TEST-ONLY: the column-sum sweeps (C2F_COLSUM: what cloudsc2_nl_launch_colsum / cloudsc2_tl_launch_colsum / cloudsc2_vjp_launch_colsum
// run) compiled for the HOST, on top of hostcheck_sparse.hip, whose dense and sparse sweeps are the references of the same library.
// An absent sum, gradient or tangent is a NULL pointer, and without `keep` every output pointer of the NL block is NULL: a guard that
// is missing in the column functions dereferences it here, on the CPU.  Like hostcheck.hip, never loaded by the package.
#include "hostcheck_sparse.hip"

// the table and the block of sums as the launchers resolve them (one stride, the mask of the fields given)
static unsigned hc_colsum_tab(const cloudsc2_real* weights, const cloudsc2_outputs& sums, ColsumTab& cs) {
  const cloudsc2_field* f = fields_of(sums);
  unsigned mask = 0u;
  cs.w = weights; cs.stride = 0;
  for (int k = 0; k < kNumOut; ++k) {
    reinterpret_cast<real_t**>(&cs.y)[k] = f[k].ptr;
    if (f[k].ptr) { mask |= 1u << k; cs.stride = f[k].block_stride; }
  }
  cs.mask = mask;
  return mask;
}

// NL: F = QSAT | PRECISE | EVAP | CKPT (the keep form) | OFF32
template <unsigned F> struct HcColsumNl {
  static void run(long long gc, const NlColsumArgs* a) {
    if constexpr ((F & ~(C2F_QSAT | C2F_PRECISE | C2F_EVAP | C2F_CKPT | C2F_OFF32)) == 0 && hc_sparse_built((F & C2F_OFF32) ? 8u : 0u))
      nl_column<F | C2F_COLSUM>(gc, &a->a);
  }
};
// TL / reverse sweep: the compact index of hostcheck_sparse.hip (bit 4, SPARSE, always on)
template <unsigned I> struct HcColsumTl {
  static void run(long long gc, const TlColsumArgs* a) {
    if constexpr (hc_sparse_built(I) && (I & 16u)) tl_column<hc_sparse_flags(I) | C2F_COLSUM>(gc, &a->a.a);
  }
};
template <unsigned I> struct HcColsumVjp {
  static void run(long long gc, const AdColsumArgs* a) {
    if constexpr (hc_sparse_built(I) && (I & 16u)) ad_reverse_column<hc_sparse_flags(I) | C2F_ASSIGN | C2F_VJP | C2F_COLSUM>(gc, &a->a.a);
  }
};

extern "C" {

// keep NULL: the lean form (every output pointer NULL, scratch not touched); else its fplsl / fplsn planes and, with the evaporation
// branch, the cover checkpoints in `scratch`
int hostcheck_colsum_nl(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, const cloudsc2_inputs* in,
                        const cloudsc2_real* weights, const cloudsc2_outputs* sums, const cloudsc2_outputs* keep, cloudsc2_real* scratch) {
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
  for (long long gc = 0; gc < a.g.ncols_pad; ++gc) hc_dispatch<HcColsumNl, 64>(f, gc, &ca);
  return 0;
}

// the tangents given are the non-NULL fields of din; dsums receives the sums of the output tangents
int hostcheck_colsum_tl(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, int satur, const cloudsc2_inputs* in,
                        const cloudsc2_inputs* din, const cloudsc2_real* weights, const cloudsc2_outputs* dsums) {
  TlColsumArgs ca;
  memset(&ca, 0, sizeof(ca));
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
  const unsigned f = hc_sparse_index(a.c, satur, 1);
  for (long long gc = 0; gc < a.g.ncols_pad; ++gc) hc_dispatch<HcColsumTl, 32>(f, gc, &ca);
  return 0;
}

// the gradients wanted are the non-NULL fields of ain; ysums gives the cotangents of the sums (read only)
int hostcheck_colsum_vjp(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, int satur, const cloudsc2_inputs* in,
                         const cloudsc2_outputs* out, const cloudsc2_inputs* ain, const cloudsc2_real* weights, const cloudsc2_outputs* ysums,
                         cloudsc2_real* scratch) {
  AdColsumArgs ca;
  memset(&ca, 0, sizeof(ca));
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
  if (!(sa.m.rd = hc_colsum_tab(weights, *ysums, ca.cs)) || !sa.m.wr) return -1;
  a.ain = writable(*ain);
  a.nl.ckpt = scratch;
  const unsigned f = hc_sparse_index(a.nl.c, satur, 1);
  for (long long gc = 0; gc < a.nl.g.ncols_pad; ++gc) hc_dispatch<HcColsumVjp, 32>(f, gc, &ca);
  return 0;
}

}  // extern "C"
