// TEST-ONLY: a stand-alone program (its own main, no Python) that runs the host build of the column-sum sweeps (hostcheck_colsum.hip)
// under the host sanitizers: tests/test_colsum_asan.py compiles it with -fsanitize=address,undefined and runs it.  Every array that is
// present is a malloc of exactly its extent -- the planes, the (nblocks, nproma) sums, the 10 x (nlev + 1) table -- and every absent one
// a NULL pointer; the lean forward is given no output plane at all.  So an access through an absent pointer, past a sum's row or past a
// half-level / full-level extent is a sanitizer report.  Each result is also compared with the fold over the dense planes and with the
// sparse reverse sweep fed the product planes.
//
//   colsum_asan_main <case file>     the file (written by the test): int32 nproma, nlev, ngptot, ncases; per case the bytes of a
//                                    cloudsc2_params and a double ptsphy; then the 16 input planes (nblocks, nlevx, nproma) in the
//                                    order of cloudsc2_inputs, in the build's precision
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#define HC_SPARSE_OFF64_ONLY
#include "hostcheck_colsum.hip"

namespace {

int g_nproma, g_nlev, g_ngptot, g_nb;
const bool kHalfIn[kNumIn] = {true, false, false, false, false, false, false, false, false, false, false, false, false, false, false, false};
const bool kHalfOut[kNumOut] = {false, false, false, false, false, true, true, true, true, false};

size_t extent(bool half) { return (size_t)g_nb * (g_nlev + (half ? 1 : 0)) * g_nproma; }

struct Array {  // a malloc of exactly n elements, or nothing
  cloudsc2_real* p = nullptr;
  size_t n = 0;
  Array() {}
  Array(size_t count, const cloudsc2_real* src, cloudsc2_real fill) { reset(count, src, fill); }
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
struct Arrays {  // the arrays of one argument block: planes, or (nblocks, nproma) sums
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
typedef Arrays<cloudsc2_inputs, kNumIn> InArrays;
typedef Arrays<cloudsc2_outputs, kNumOut> OutArrays;

int fail_at(const char* what, const char* sweep, int icase, int satur, int precise, unsigned msum, unsigned min) {
  fprintf(stderr, "colsum_asan_main: %s (%s, case %d, satur %d, precise %d, sums 0x%x, inputs 0x%x)\n", what, sweep, icase, satur, precise, msum,
          min);
  return 1;
}

bool active(int ibl, int jl) { return (long long)ibl * g_nproma + jl < g_ngptot; }

// the contract: acc = +0; acc = fl(acc + fl(w[k] * plane[k])); the padded tail still NaN
bool sum_ok(const Array& got, const cloudsc2_real* w, const cloudsc2_real* plane, bool half) {
  const int nlevx = g_nlev + (half ? 1 : 0);
  for (int ibl = 0; ibl < g_nb; ++ibl)
    for (int jl = 0; jl < g_nproma; ++jl) {
      const cloudsc2_real g = got.p[(size_t)ibl * g_nproma + jl];
      if (!active(ibl, jl)) {
        if (g == g) return false;
        continue;
      }
      cloudsc2_real acc = 0;
      for (int jk = 0; jk < nlevx; ++jk) {
        const cloudsc2_real p = w[jk] * plane[((size_t)ibl * nlevx + jk) * g_nproma + jl];
        acc = acc + p;
      }
      if (memcmp(&g, &acc, sizeof(acc)) != 0) return false;
    }
  return true;
}

// the active columns of a written plane: all written (no NaN left), `want`'s bits; the padded tail still NaN
bool plane_ok(const Array& got, const Array& want, bool half) {
  const int nlevx = g_nlev + (half ? 1 : 0);
  for (int ibl = 0; ibl < g_nb; ++ibl)
    for (int jk = 0; jk < nlevx; ++jk)
      for (int jl = 0; jl < g_nproma; ++jl) {
        const size_t i = ((size_t)ibl * nlevx + jk) * g_nproma + jl;
        if (active(ibl, jl) ? memcmp(&got.p[i], &want.p[i], sizeof(cloudsc2_real)) != 0 : got.p[i] == got.p[i]) return false;
      }
  return true;
}

struct Pattern { unsigned sums, in; };

std::vector<Pattern> patterns(int satur) {
  const unsigned all_in = satur ? (C2I_ALL & ~C2I_QSAT) : C2I_ALL;
  std::vector<Pattern> p;
  p.push_back({C2O_ALL, all_in});
  for (int k = 0; k < kNumOut; ++k) p.push_back({1u << k, C2I_Q | C2I_T});  // each sum alone
  p.push_back({C2O_FPLSL | C2O_FPLSN, C2I_Q | C2I_T});                      // the narrow case
  p.push_back({C2O_TENT | C2O_TENQ, C2I_PAPH | C2I_LU});                    // the planes with accesses outside the level loop
  uint64_t s = 20261020u + (unsigned)satur;
  for (int k = 0; k < 4;) {  // seeded random patterns
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    const unsigned in = (unsigned)(s >> 20) & all_in, sums = (unsigned)(s >> 40) & C2O_ALL;
    if (in && sums) { p.push_back({sums, in}); ++k; }
  }
  return p;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: colsum_asan_main <case file>\n"); return 2; }
  FILE* fp = fopen(argv[1], "rb");
  if (!fp) { fprintf(stderr, "colsum_asan_main: cannot open %s\n", argv[1]); return 2; }
  int32_t head[4];
  if (fread(head, sizeof(int32_t), 4, fp) != 4) return 2;
  g_nproma = head[0]; g_nlev = head[1]; g_ngptot = head[2];
  const int ncases = head[3];
  g_nb = (g_ngptot + g_nproma - 1) / g_nproma;
  std::vector<cloudsc2_params> prms((size_t)ncases);
  std::vector<double> ptsphy((size_t)ncases);
  for (int c = 0; c < ncases; ++c)
    if (fread(&prms[c], sizeof(cloudsc2_params), 1, fp) != 1 || fread(&ptsphy[c], sizeof(double), 1, fp) != 1) return 2;
  std::vector<std::vector<cloudsc2_real>> state(kNumIn);
  for (int k = 0; k < kNumIn; ++k) {
    state[k].resize(extent(kHalfIn[k]));
    if (fread(state[k].data(), sizeof(cloudsc2_real), state[k].size(), fp) != state[k].size()) return 2;
  }
  fclose(fp);
  const cloudsc2_real nan = (cloudsc2_real)NAN;
  const int row = g_nlev + 1;

  // the table: negative entries, exact zeros, both ends non-zero; the unused last entry of a full-level row is NaN
  std::vector<cloudsc2_real> wts((size_t)kNumOut * row);
  uint64_t s = 77;
  for (int n = 0; n < kNumOut; ++n)
    for (int k = 0; k < row; ++k) {
      s = s * 6364136223846793005ull + 1442695040888963407ull;
      const double u = (double)(s >> 11) / 9007199254740992.0;
      cloudsc2_real w = (cloudsc2_real)(2.0 * u - 1.0);
      if ((s >> 7) % 5 == 0) w = 0;
      const int last = kHalfOut[n] ? g_nlev : g_nlev - 1;
      if (k == 0) w = (cloudsc2_real)-0.75;
      if (k == last) w = (cloudsc2_real)0.625;
      if (k > last) w = nan;
      wts[(size_t)n * row + k] = w;
    }
  std::vector<cloudsc2_real> ybar((size_t)kNumOut * g_nb * g_nproma);
  for (auto& e : ybar) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    e = (cloudsc2_real)(2.0 * ((double)(s >> 11) / 9007199254740992.0) - 1.0);
  }

  long long runs = 0;
  for (int c = 0; c < ncases; ++c)
    for (int satur = 0; satur < 2; ++satur)
      for (int precise = 0; precise < 2; ++precise) {
        hostcheck_set_precise(precise);
        const cloudsc2_params* prm = &prms[c];
        const bool evap = prm->levapls2 || prm->ldrain1d;
        const unsigned all_in = satur ? (C2I_ALL & ~C2I_QSAT) : C2I_ALL;
        InArrays x;
        for (int k = 0; k < kNumIn; ++k)
          if (all_in & (1u << k)) x.plane(k, kHalfIn[k], state[k].data(), 0);
        OutArrays traj;
        for (int k = 0; k < kNumOut; ++k) traj.plane(k, kHalfOut[k], nullptr, 0);
        Array scratch(extent(false), nullptr, 0);
        if (hostcheck_sparse_forward(prm, ptsphy[c], g_nproma, g_nlev, g_ngptot, &x.blk, &traj.blk, scratch.p)) return 1;
        std::vector<std::vector<cloudsc2_real>> v(kNumIn);
        for (int k = 0; k < kNumIn; ++k) {
          v[k] = state[k];
          for (auto& e : v[k]) e *= (cloudsc2_real)0.01;
        }
        for (const Pattern& pt : patterns(satur)) {
          Array table((size_t)kNumOut * row, wts.data(), 0);
          for (int n = 0; n < kNumOut; ++n)  // the rows of absent sums must not be read: NaN
            if (!(pt.sums & (1u << n)))
              for (int k = 0; k < row; ++k) table.p[(size_t)n * row + k] = nan;
          {  // NL, lean: no output plane anywhere
            OutArrays y;
            for (int n = 0; n < kNumOut; ++n)
              if (pt.sums & (1u << n)) y.sum(n, nullptr, nan);
            if (hostcheck_colsum_nl(prm, ptsphy[c], g_nproma, g_nlev, g_ngptot, &x.blk, table.p, &y.blk, nullptr, nullptr))
              return fail_at("the sweep refused its arguments", "NL", c, satur, precise, pt.sums, 0);
            for (int n = 0; n < kNumOut; ++n)
              if ((pt.sums & (1u << n)) && !sum_ok(y.a[n], table.p + (size_t)n * row, traj.a[n].p, kHalfOut[n]))
                return fail_at("a sum differs from the fold over the dense plane, or its tail was written", "NL", c, satur, precise, pt.sums, 0);
            ++runs;
          }
          {  // NL with keep: the two flux planes, and the checkpoints only with the evaporation branch (else no scratch at all)
            OutArrays y, keep;
            for (int n = 0; n < kNumOut; ++n)
              if (pt.sums & (1u << n)) y.sum(n, nullptr, nan);
            keep.plane(5, true, nullptr, nan);
            keep.plane(6, true, nullptr, nan);
            Array ck;
            if (evap) ck.reset(extent(false), nullptr, nan);
            if (hostcheck_colsum_nl(prm, ptsphy[c], g_nproma, g_nlev, g_ngptot, &x.blk, table.p, &y.blk, &keep.blk, ck.p))
              return fail_at("the sweep refused its arguments", "NL keep", c, satur, precise, pt.sums, 0);
            for (int n = 0; n < kNumOut; ++n)
              if ((pt.sums & (1u << n)) && !sum_ok(y.a[n], table.p + (size_t)n * row, traj.a[n].p, kHalfOut[n]))
                return fail_at("a sum differs from the fold over the dense plane, or its tail was written", "NL keep", c, satur, precise, pt.sums, 0);
            if (!plane_ok(keep.a[5], traj.a[5], true) || !plane_ok(keep.a[6], traj.a[6], true) || (evap && !plane_ok(ck, scratch, false)))
              return fail_at("a kept plane differs from the trajectory pass", "NL keep", c, satur, precise, pt.sums, 0);
            ++runs;
          }
          {  // TL: tangents pt.in read; the sums of the sparse TL sweep's planes
            InArrays dx;
            OutArrays dy, ds;
            for (int k = 0; k < kNumIn; ++k)
              if (pt.in & (1u << k)) dx.plane(k, kHalfIn[k], v[k].data(), 0);
            for (int n = 0; n < kNumOut; ++n) {
              dy.plane(n, kHalfOut[n], nullptr, 0);
              if (pt.sums & (1u << n)) ds.sum(n, nullptr, nan);
            }
            if (hostcheck_sparse_tl(prm, ptsphy[c], g_nproma, g_nlev, g_ngptot, satur, 1, &x.blk, &dx.blk, &dy.blk) ||
                hostcheck_colsum_tl(prm, ptsphy[c], g_nproma, g_nlev, g_ngptot, satur, &x.blk, &dx.blk, table.p, &ds.blk))
              return fail_at("a sweep refused its arguments", "TL", c, satur, precise, pt.sums, pt.in);
            for (int n = 0; n < kNumOut; ++n)
              if ((pt.sums & (1u << n)) && !sum_ok(ds.a[n], table.p + (size_t)n * row, dy.a[n].p, kHalfOut[n]))
                return fail_at("a tangent sum differs from the fold over the sparse sweep's plane, or its tail was written", "TL", c, satur,
                               precise, pt.sums, pt.in);
            runs += 2;
          }
          {  // reverse sweep: gradients pt.in written; the sparse sweep fed the planes w[k] * ybar[c]
            InArrays xa, xw;
            OutArrays yb, yp;
            for (int k = 0; k < kNumIn; ++k)
              if (pt.in & (1u << k)) { xa.plane(k, kHalfIn[k], nullptr, nan); xw.plane(k, kHalfIn[k], nullptr, nan); }
            for (int n = 0; n < kNumOut; ++n) {
              if (!(pt.sums & (1u << n))) continue;
              const cloudsc2_real* yn = ybar.data() + (size_t)n * g_nb * g_nproma;
              yb.sum(n, yn, 0);
              yp.plane(n, kHalfOut[n], nullptr, 0);
              const int nlevx = g_nlev + (kHalfOut[n] ? 1 : 0);
              for (int ibl = 0; ibl < g_nb; ++ibl)
                for (int jk = 0; jk < nlevx; ++jk)
                  for (int jl = 0; jl < g_nproma; ++jl)
                    yp.a[n].p[((size_t)ibl * nlevx + jk) * g_nproma + jl] = table.p[(size_t)n * row + jk] * yn[(size_t)ibl * g_nproma + jl];
            }
            if (hostcheck_colsum_vjp(prm, ptsphy[c], g_nproma, g_nlev, g_ngptot, satur, &x.blk, &traj.blk, &xa.blk, table.p, &yb.blk, scratch.p) ||
                hostcheck_sparse_vjp(prm, ptsphy[c], g_nproma, g_nlev, g_ngptot, satur, 1, &x.blk, &traj.blk, &xw.blk, &yp.blk, scratch.p))
              return fail_at("a sweep refused its arguments", "reverse", c, satur, precise, pt.sums, pt.in);
            for (int k = 0; k < kNumIn; ++k)
              if ((pt.in & (1u << k)) && !plane_ok(xa.a[k], xw.a[k], kHalfIn[k]))
                return fail_at("a gradient differs from the sparse sweep fed the product planes, has an unwritten active element or a "
                               "written tail", "reverse", c, satur, precise, pt.sums, pt.in);
            runs += 2;
          }
        }
      }
  hostcheck_set_precise(0);
  printf("colsum_asan_main: %lld sweeps, every sum the fold's bits and every gradient the sparse sweep's\n", runs);
  return 0;
}
