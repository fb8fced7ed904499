// TEST-ONLY: a stand-alone program (its own main, no Python) that runs the host build of the parameter column-sum sweep
// (hostcheck_parcolsum.hip) under the host sanitizers: tests/test_parcolsum_asan.py compiles it with -fsanitize=address,undefined and
// runs it.  Every array that is present is a malloc of exactly its extent -- the input planes, the (nblocks, nproma) sums, residuals
// and weights, the 10 x (nlev + 1) table, the workspace -- and every absent one a NULL pointer.  So an access through an absent pointer,
// past a row of sums or past the workspace is a sanitizer report.  Each sum is also compared with the fold over hostcheck_tl_parjac's
// planes (hostcheck_parjac.hip's sweep, included here), and the normal form with the contraction of those sums in the sweep's order.
//
//   parcolsum_asan_main <case file>  the file (written by the test): int32 nproma, nlev, ngptot, ncases; per case the bytes of a
//                                    cloudsc2_params and a double ptsphy; then the 16 input planes (nblocks, nlevx, nproma) in the
//                                    order of cloudsc2_inputs, in the build's precision
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "hostcheck_parcolsum.hip"

#include "hostcheck_parjac.hip"

namespace {

constexpr int kIn = 16, kOut = 10;
int g_nproma, g_nlev, g_ngptot, g_nb;
const bool kHalfOut[kOut] = {false, false, false, false, false, true, true, true, true, false};
const bool kParSum[kOut] = {true, true, true, true, false, true, true, true, true, false};

size_t extent(bool half) { return (size_t)g_nb * (g_nlev + (half ? 1 : 0)) * g_nproma; }

struct Array {  // a malloc of exactly n elements, or nothing
  cloudsc2_real* p = nullptr;
  size_t n = 0;
  Array() {}
  Array(const Array&) = delete;
  Array& operator=(const Array&) = delete;
  ~Array() { free(p); }
  void reset(size_t count, const cloudsc2_real* src, cloudsc2_real fill) {  // a copy of src, or `fill` everywhere
    free(p);
    n = count;
    p = (cloudsc2_real*)malloc(n * sizeof(cloudsc2_real));
    for (size_t i = 0; i < n; ++i) p[i] = src ? src[i] : fill;
  }
};

template <class Block, int N>
struct Arrays {  // the arrays of one argument block: planes, or (nblocks, nproma) arrays
  Array a[N];
  Block blk;
  Arrays() { memset(&blk, 0, sizeof(blk)); }
  void plane(int k, bool half, const cloudsc2_real* src, cloudsc2_real fill) {
    a[k].reset(extent(half), src, fill);
    cloudsc2_field* f = reinterpret_cast<cloudsc2_field*>(&blk) + k;
    f->ptr = a[k].p;
    f->block_stride = (long long)(g_nlev + (half ? 1 : 0)) * g_nproma;
  }
  void sum(int k, const cloudsc2_real* src, cloudsc2_real fill) {
    a[k].reset((size_t)g_nb * g_nproma, src, fill);
    cloudsc2_field* f = reinterpret_cast<cloudsc2_field*>(&blk) + k;
    f->ptr = a[k].p;
    f->block_stride = g_nproma;
  }
};
typedef Arrays<cloudsc2_inputs, kIn> InArrays;
typedef Arrays<cloudsc2_outputs, kOut> OutArrays;

int fail_at(const char* what, int icase, int satur, int precise, unsigned msum) {
  fprintf(stderr, "parcolsum_asan_main: %s (case %d, qsat %s, precise %d, sums 0x%x)\n", what, icase, satur ? "NULL" : "given", precise, msum);
  return 1;
}

bool active(int ibl, int jl) { return (long long)ibl * g_nproma + jl < g_ngptot; }

// the parent's planes: hostcheck_tl_parjac
void parjac(const cloudsc2_params* prm, double ptsphy, const cloudsc2_inputs* in, OutArrays* dout, int np) {
  cloudsc2_outputs blocks[4];
  memset(blocks, 0, sizeof(blocks));
  for (int b = 0; b < np; ++b) blocks[b] = dout[b].blk;
  hostcheck_tl_parjac(prm, ptsphy, g_nproma, g_nlev, g_ngptot, in, blocks);
}

// the contract: acc = +0; acc = fl(acc + fl(w[k] * plane[k]))
cloudsc2_real fold(const cloudsc2_real* w, const cloudsc2_real* plane, bool half, int ibl, int jl) {
  const int nlevx = g_nlev + (half ? 1 : 0);
  cloudsc2_real acc = 0;
  for (int jk = 0; jk < nlevx; ++jk) {
    const cloudsc2_real p = w[jk] * plane[((size_t)ibl * nlevx + jk) * g_nproma + jl];
    acc = acc + p;
  }
  return acc;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: parcolsum_asan_main <case file>\n"); return 2; }
  FILE* fp = fopen(argv[1], "rb");
  if (!fp) { fprintf(stderr, "parcolsum_asan_main: cannot open %s\n", argv[1]); return 2; }
  int32_t head[4];
  if (fread(head, sizeof(int32_t), 4, fp) != 4) return 2;
  g_nproma = head[0]; g_nlev = head[1]; g_ngptot = head[2];
  const int ncases = head[3];
  g_nb = (g_ngptot + g_nproma - 1) / g_nproma;
  std::vector<cloudsc2_params> prms((size_t)ncases);
  std::vector<double> ptsphy((size_t)ncases);
  for (int c = 0; c < ncases; ++c)
    if (fread(&prms[c], sizeof(cloudsc2_params), 1, fp) != 1 || fread(&ptsphy[c], sizeof(double), 1, fp) != 1) return 2;
  std::vector<std::vector<cloudsc2_real>> state(kIn);
  for (int k = 0; k < kIn; ++k) {
    state[k].resize(extent(k == 0));
    if (fread(state[k].data(), sizeof(cloudsc2_real), state[k].size(), fp) != state[k].size()) return 2;
  }
  fclose(fp);
  const cloudsc2_real nan = (cloudsc2_real)NAN;
  const int row = g_nlev + 1;
  const size_t ncols = (size_t)g_nb * g_nproma;

  // the table: negative entries, exact zeros, both ends non-zero; the unused last entry of a full-level row is NaN
  std::vector<cloudsc2_real> wts((size_t)kOut * row);
  uint64_t s = 77;
  auto next = [&]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) / 9007199254740992.0; };
  for (int n = 0; n < kOut; ++n)
    for (int k = 0; k < row; ++k) {
      cloudsc2_real w = (cloudsc2_real)(2.0 * next() - 1.0);
      if ((s >> 7) % 5 == 0) w = 0;
      const int last = kHalfOut[n] ? g_nlev : g_nlev - 1;
      if (k == 0) w = (cloudsc2_real)-0.75;
      if (k == last) w = (cloudsc2_real)0.625;
      if (k > last) w = nan;
      wts[(size_t)n * row + k] = w;
    }
  // residuals and weights per column and sum: NaN in the padded tail
  std::vector<cloudsc2_real> res((size_t)kOut * ncols), wgt((size_t)kOut * ncols);
  for (int n = 0; n < kOut; ++n)
    for (int ibl = 0; ibl < g_nb; ++ibl)
      for (int jl = 0; jl < g_nproma; ++jl) {
        const size_t i = (size_t)n * ncols + (size_t)ibl * g_nproma + jl;
        res[i] = active(ibl, jl) ? (cloudsc2_real)(2.0 * next() - 1.0) : nan;
        wgt[i] = active(ibl, jl) ? (cloudsc2_real)(0.5 + 1.5 * next()) : nan;
      }
  // the sums of a launch: all ten, each alone, the surface fluxes, tent + tenq
  std::vector<unsigned> masks = {C2O_ALL, C2O_FPLSL | C2O_FPLSN, C2O_TENT | C2O_TENQ};
  for (int n = 0; n < kOut; ++n) masks.push_back(1u << n);

  long long runs = 0;
  for (int c = 0; c < ncases; ++c)
    for (int satur = 0; satur < 2; ++satur)
      for (int precise = 0; precise < 2; ++precise) {
        hostcheck_set_precise(precise);
        const cloudsc2_params* prm = &prms[c];
        const bool evap = prm->levapls2 || prm->ldrain1d;
        const int np = evap ? 4 : 3;
        InArrays x;
        for (int k = 0; k < kIn; ++k)
          if (!(satur && k == 3)) x.plane(k, k == 0, state[k].data(), 0);  // (k = 3: qsat; absent: SATUR in the sweep)
        OutArrays sens[4];
        for (int b = 0; b < np; ++b)
          for (int n = 0; n < kOut; ++n) sens[b].plane(n, kHalfOut[n], nullptr, 0);
        parjac(prm, ptsphy[c], &x.blk, sens, np);
        for (unsigned m : masks) {
          Array table;
          table.reset((size_t)kOut * row, wts.data(), 0);
          for (int n = 0; n < kOut; ++n)  // the rows of absent sums, and of the two that depend on no parameter, must not be read: NaN
            if (!(m & (1u << n)) || !kParSum[n])
              for (int k = 0; k < row; ++k) table.p[(size_t)n * row + k] = nan;
          {  // the sums form: np blocks (the fourth absent without the evaporation branch)
            OutArrays y[4];
            cloudsc2_outputs blocks[4];
            memset(blocks, 0, sizeof(blocks));
            for (int b = 0; b < np; ++b) {
              for (int n = 0; n < kOut; ++n)
                if (m & (1u << n)) y[b].sum(n, nullptr, nan);
              blocks[b] = y[b].blk;
            }
            if (hostcheck_parjac_colsum(prm, ptsphy[c], g_nproma, g_nlev, g_ngptot, &x.blk, table.p, blocks))
              return fail_at("the sums form refused its arguments", c, satur, precise, m);
            for (int b = 0; b < np; ++b)
              for (int n = 0; n < kOut; ++n) {
                if (!(m & (1u << n))) continue;
                for (int ibl = 0; ibl < g_nb; ++ibl)
                  for (int jl = 0; jl < g_nproma; ++jl) {
                    const cloudsc2_real got = y[b].a[n].p[(size_t)ibl * g_nproma + jl];
                    if (!active(ibl, jl)) {
                      if (got == got) return fail_at("the padded tail of a sum was written", c, satur, precise, m);
                      continue;
                    }
                    const cloudsc2_real want = kParSum[n] ? fold(wts.data() + (size_t)n * row, sens[b].a[n].p, kHalfOut[n], ibl, jl) : (cloudsc2_real)0;
                    if (memcmp(&got, &want, sizeof(want)) != 0)
                      return fail_at("a sum differs from the fold over the parameter Jacobian's plane", c, satur, precise, m);
                  }
              }
            ++runs;
          }
          for (int weighted = 0; weighted < 3; ++weighted) {  // the normal form: no weight block, every weight, the first weight only
            OutArrays r, w;
            bool first = true;
            for (int n = 0; n < kOut; ++n) {
              if (!(m & (1u << n))) continue;
              r.sum(n, res.data() + (size_t)n * ncols, 0);
              if (weighted == 1 || (weighted == 2 && first)) w.sum(n, wgt.data() + (size_t)n * ncols, 0);
              first = false;
            }
            const size_t nwork = (size_t)CLOUDSC2_NNORMAL * ncols;
            double* work = (double*)malloc(nwork * sizeof(double));
            for (size_t i = 0; i < nwork; ++i) work[i] = NAN;
            int bad = hostcheck_parnormal_colsum(prm, ptsphy[c], g_nproma, g_nlev, g_ngptot, &x.blk, table.p, &r.blk, weighted ? &w.blk : nullptr, work);
            for (int ibl = 0; ibl < g_nb && !bad; ++ibl)
              for (int jl = 0; jl < g_nproma && !bad; ++jl) {
                const size_t col = (size_t)ibl * g_nproma + jl;
                double h[4][4] = {}, g[4] = {};
                for (int n = 0; n < kOut; ++n) {  // the sweep's order: the observed sums in the order of cloudsc2_outputs
                  if (!(m & (1u << n)) || !kParSum[n]) continue;
                  double j[4];
                  for (int a = 0; a < np; ++a) j[a] = (double)fold(wts.data() + (size_t)n * row, sens[a].a[n].p, kHalfOut[n], ibl, jl);
                  const double wd = w.a[n].p ? (double)w.a[n].p[col] : 1.0, rd = (double)r.a[n].p[col];
                  for (int a = 0; a < np && active(ibl, jl); ++a) {
                    const double wj = wd * j[a];
                    for (int b = a; b < np; ++b) h[a][b] += wj * j[b];
                    g[a] += wj * rd;
                  }
                }
                for (int a = 0; a < 4; ++a) {
                  for (int b = a; b < 4; ++b) {
                    const double got = work[(size_t)normal_row_h(a, b) * ncols + col];
                    const bool written = active(ibl, jl) && b < np;
                    if (written ? memcmp(&got, &h[a][b], sizeof(double)) != 0 : got == got) bad = 2;
                  }
                  const double got = work[(size_t)normal_row_g(a) * ncols + col];
                  if ((active(ibl, jl) && a < np) ? memcmp(&got, &g[a], sizeof(double)) != 0 : got == got) bad = 2;
                }
              }
            free(work);
            if (bad) return fail_at(bad == 2 ? "the normal form differs from the contraction of the folded sums, or wrote a row or column it must not"
                                             : "the normal form refused its arguments", c, satur, precise, m);
            ++runs;
          }
        }
      }
  hostcheck_set_precise(0);
  printf("parcolsum_asan_main: %lld sweeps, every sum the fold's bits and every normal form the contraction's\n", runs);
  return 0;
}
