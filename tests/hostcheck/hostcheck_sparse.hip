// TEST-ONLY: the sparse TL and reverse sweeps (C2F_SPARSE: what cloudsc2_tl_launch_sparse / cloudsc2_vjp_launch_sparse run) compiled for
// the HOST next to their dense twins (tl_column<F> without trajectory stores, ad_reverse_column<F | ASSIGN | VJP>, each with qsat as a
// plane or with C2F_SATLIN), on top of the helpers of hostcheck.hip.  A field of the derivative blocks with a NULL ptr is absent: a guard
// that is missing in the column functions dereferences it here, on the CPU.  Like hostcheck.hip, never loaded by the package.
#include "hostcheck.hip"
#include "../../dwarf_p_cloudsc2_tl_ad_amd/csrc/cloudsc2_fields.hpp"

namespace cloudsc2 {
int fail(int code, const char*) { return code; }  // (cloudsc2_fields.hpp: a test program brings its own)
}

// compact index of a variant -> its flag word: bit 0 SATLIN (else QSAT), 1 PRECISE, 2 EVAP, 3 OFF32, 4 SPARSE (else the dense twin)
constexpr unsigned hc_sparse_flags(unsigned i) {
  return ((i & 1u) ? C2F_SATLIN : C2F_QSAT) | ((i & 2u) ? C2F_PRECISE : 0u) | ((i & 4u) ? C2F_EVAP : 0u) | ((i & 8u) ? C2F_OFF32 : 0u) |
         ((i & 16u) ? C2F_SPARSE : 0u);
}
// -DHC_SPARSE_OFF64_ONLY (the sanitizer program, whose build time goes with the number of variants): the 32-bit-offset forms are not built
#ifdef HC_SPARSE_OFF64_ONLY
constexpr bool hc_sparse_built(unsigned i) { return (i & 8u) == 0; }
#else
constexpr bool hc_sparse_built(unsigned) { return true; }
#endif
template <unsigned I> struct HcSparseTl {
  static void run(long long gc, const TlSparseArgs* a) {
    if constexpr (hc_sparse_built(I)) tl_column<hc_sparse_flags(I)>(gc, &a->a);
  }
};
template <unsigned I> struct HcSparseVjp {
  static void run(long long gc, const AdSparseArgs* a) {
    if constexpr (hc_sparse_built(I)) ad_reverse_column<hc_sparse_flags(I) | C2F_ASSIGN | C2F_VJP>(gc, &a->a);
  }
};
template <unsigned F> struct HcSparseFwd {
  static void run(long long gc, const NlArgs* a) {
    if constexpr ((F & ~(C2F_QSAT | C2F_PRECISE | C2F_EVAP)) == 0) nl_column<F | ((F & C2F_EVAP) ? C2F_CKPT : 0u)>(gc, a);
  }
};

static unsigned hc_sparse_index(const Consts& c, int satur, int sparse) {
  return (satur ? 1u : 0u) | (g_hc_precise ? 2u : 0u) | (c.evap ? 4u : 0u) | (g_hc_off32 ? 8u : 0u) | (sparse ? 16u : 0u);
}

extern "C" {

// the trajectory pass: traj_out (PFPLSL5 / PFPLSN5 among it) and, with the evaporation branch, the cover checkpoints in `scratch`
int hostcheck_sparse_forward(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, const cloudsc2_inputs* in,
                             const cloudsc2_outputs* out, cloudsc2_real* scratch) {
  NlArgs a;
  memset(&a, 0, sizeof(a));
  a.g = hc_geom(nproma, nlev, ngptot);
  a.c = hc_consts(*prm, ptsphy);
  LevelTab tab; hc_tables(*prm, tab, a.g);
  a.tab = &tab;
  hc_in(*in, a.s, a.in); hc_out(*out, a.s, a.out);
  a.ckpt = scratch;
  const unsigned f = (in->qsat.ptr ? C2F_QSAT : 0u) | (g_hc_precise ? C2F_PRECISE : 0u) | (a.c.evap ? C2F_EVAP : 0u);
  for (long long gc = 0; gc < a.g.ncols_pad; ++gc) hc_dispatch<HcSparseFwd, 8>(f, gc, &a);
  return 0;
}

// sparse != 0: tl_column<F | C2F_SPARSE>, NULL fields of din / dout absent; sparse = 0: the dense twin, every field required
int hostcheck_sparse_tl(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, int satur, int sparse,
                        const cloudsc2_inputs* in, const cloudsc2_inputs* din, const cloudsc2_outputs* dout) {
  TlSparseArgs sa;
  memset(&sa, 0, sizeof(sa));
  TlArgs& a = sa.a;
  a.g = hc_geom(nproma, nlev, ngptot);
  a.c = hc_consts(*prm, ptsphy);
  LevelTab tab; hc_tables(*prm, tab, a.g);
  a.tab = &tab;
  hc_in(*in, a.s, a.in);
  if (resolve_sparse(*din, *dout, 'o', a.sp, a.din, a.dout, sa.m.rd, sa.m.wr)) return -1;
  if (!sparse && (sa.m.rd != (satur ? (C2I_ALL & ~C2I_QSAT) : C2I_ALL) || sa.m.wr != C2O_ALL)) return -2;
  const unsigned f = hc_sparse_index(a.c, satur, sparse);
  for (long long gc = 0; gc < a.g.ncols_pad; ++gc) hc_dispatch<HcSparseTl, 32>(f, gc, &sa);
  return 0;
}

// sparse != 0: ad_reverse_column<F | ASSIGN | VJP | C2F_SPARSE>, NULL fields of ain / aout absent; sparse = 0: the dense twin
int hostcheck_sparse_vjp(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, int satur, int sparse,
                         const cloudsc2_inputs* in, const cloudsc2_outputs* out, const cloudsc2_inputs* ain, const cloudsc2_outputs* aout,
                         cloudsc2_real* scratch) {
  AdSparseArgs sa;
  memset(&sa, 0, sizeof(sa));
  AdArgs& a = sa.a;
  a.nl.g = hc_geom(nproma, nlev, ngptot);
  a.nl.c = hc_consts(*prm, ptsphy);
  LevelTab tab; hc_tables(*prm, tab, a.nl.g);
  a.nl.tab = &tab;
  hc_in(*in, a.nl.s, a.nl.in); hc_out(*out, a.nl.s, a.nl.out);
  InPtrs ain_c;
  if (resolve_sparse(*ain, *aout, 'i', a.sa, ain_c, a.aout, sa.m.wr, sa.m.rd)) return -1;
  if (!sparse && (sa.m.wr != (satur ? (C2I_ALL & ~C2I_QSAT) : C2I_ALL) || sa.m.rd != C2O_ALL)) return -2;
  a.ain = writable(*ain);
  a.nl.ckpt = scratch;
  const unsigned f = hc_sparse_index(a.nl.c, satur, sparse);
  for (long long gc = 0; gc < a.nl.g.ncols_pad; ++gc) hc_dispatch<HcSparseVjp, 32>(f, gc, &sa);
  return 0;
}

}  // extern "C"
