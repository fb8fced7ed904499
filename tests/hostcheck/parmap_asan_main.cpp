// TEST-ONLY: a stand-alone program (its own main, no Python) that runs the host build of the three parameter-map sweeps
// (hostcheck_parmap.hip) under the host sanitizers: tests/test_parmap_asan.py compiles it with -fsanitize=address,undefined and runs
// it.  Every table -- values, tangents, adjoints: (4, ncols_pad) doubles -- and every plane is a malloc of exactly its extent, an absent
// plane (qsat with SATUR in the sweep, the cover checkpoint without the evaporation branch) a NULL pointer.  So an access through an
// absent pointer, past a table's last column or past a plane is a sanitizer report.  Every array the sweeps write is prefilled with NaN:
// the program also checks that every active element was written and that the padded tail was not (PCOVPTOT's is zeroed).
//
//   parmap_asan_main <case file>  the file (written by the test): int32 nproma, nlev, ngptot, ncases; per case the bytes of a
//                                 cloudsc2_params and a double ptsphy; then the 16 input planes (nblocks, nlevx, nproma) in the order
//                                 of cloudsc2_inputs, in the build's precision
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "hostcheck_parmap.hip"

namespace {

constexpr int kIn = 16, kOut = 10, kQsat = 3;
int g_nproma, g_nlev, g_ngptot, g_nb;
const bool kHalfOut[kOut] = {false, false, false, false, false, true, true, true, true, false};

size_t extent(bool half) { return (size_t)g_nb * (g_nlev + (half ? 1 : 0)) * g_nproma; }

template <class T>
struct Array {  // a malloc of exactly n elements, or nothing
  T* p = nullptr;
  size_t n = 0;
  Array() {}
  Array(const Array&) = delete;
  Array& operator=(const Array&) = delete;
  ~Array() { free(p); }
  void reset(size_t count, const T* src, T fill, T scale = 1) {  // scale * src, or `fill` everywhere
    free(p);
    n = count;
    p = (T*)malloc(n * sizeof(T));
    for (size_t i = 0; i < n; ++i) p[i] = src ? scale * src[i] : fill;
  }
};

template <class Block, int N>
struct Arrays {  // the planes of one argument block
  Array<cloudsc2_real> a[N];
  Block blk;
  Arrays() { memset(&blk, 0, sizeof(blk)); }
  void plane(int k, bool half, const cloudsc2_real* src, cloudsc2_real fill, cloudsc2_real scale = 1) {
    a[k].reset(extent(half), src, fill, scale);
    cloudsc2_field* f = reinterpret_cast<cloudsc2_field*>(&blk) + k;
    f->ptr = a[k].p;
    f->block_stride = (long long)(g_nlev + (half ? 1 : 0)) * g_nproma;
  }
};
typedef Arrays<cloudsc2_inputs, kIn> InArrays;
typedef Arrays<cloudsc2_outputs, kOut> OutArrays;

int fail_at(const char* what, int icase, int satur, int precise) {
  fprintf(stderr, "parmap_asan_main: %s (case %d, qsat %s, precise %d)\n", what, icase, satur ? "NULL" : "given", precise);
  return 1;
}

// every active element written, the padded tail still NaN (or zero: PCOVPTOT of the NL sweep)
bool written(const cloudsc2_real* p, bool half, bool tail_zero = false) {
  const int nlevx = g_nlev + (half ? 1 : 0);
  for (int ibl = 0; ibl < g_nb; ++ibl)
    for (int jk = 0; jk < nlevx; ++jk)
      for (int jl = 0; jl < g_nproma; ++jl) {
        const cloudsc2_real v = p[((size_t)ibl * nlevx + jk) * g_nproma + jl];
        const bool active = (long long)ibl * g_nproma + jl < g_ngptot;
        if (active ? v != v : (tail_zero ? v != 0 : v == v)) return false;
      }
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: parmap_asan_main <case file>\n"); return 2; }
  FILE* fp = fopen(argv[1], "rb");
  if (!fp) { fprintf(stderr, "parmap_asan_main: cannot open %s\n", argv[1]); return 2; }
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

  const size_t ncp = (size_t)g_nb * g_nproma;
  const double nan = NAN;
  int runs = 0;
  for (int icase = 0; icase < ncases; ++icase) {
    const cloudsc2_params& prm = prms[icase];
    const bool evap = prm.levapls2 || prm.ldrain1d;
    for (int satur = 0; satur < 2; ++satur)
      for (int precise = 0; precise < 2; ++precise) {
        hostcheck_set_precise(precise);
        // the tables: a value and a tangent of its own per column and parameter; NaN in the padded tail (never read)
        Array<double> par, dpar, apar;
        par.reset(4 * ncp, nullptr, nan); dpar.reset(4 * ncp, nullptr, nan); apar.reset(4 * ncp, nullptr, nan);
        const double own[4] = {prm.rkconv, prm.rclcrit, prm.rlptrc, prm.rpecons};
        for (int i = 0; i < 4; ++i)
          for (long long c = 0; c < g_ngptot; ++c) {
            const double f = 0.01 * (double)((7 * c + 3 * i) % 41 - 20);  // -0.2 .. 0.2
            par.p[i * ncp + c] = i == 2 ? own[i] + 10.0 * f : own[i] * (1.0 + f);
            dpar.p[i * ncp + c] = 0.01 * own[i] * (1.0 + f);
          }
        InArrays in, din, ain;
        OutArrays out, dout;
        for (int k = 0; k < kIn; ++k) {
          if (k == kQsat && satur) continue;  // absent: NULL
          in.plane(k, k == 0, state[k].data(), 0);
          din.plane(k, k == 0, state[k].data(), 0, (cloudsc2_real)0.01);
          ain.plane(k, k == 0, nullptr, (cloudsc2_real)nan);
        }
        for (int k = 0; k < kOut; ++k) {
          out.plane(k, kHalfOut[k], nullptr, (cloudsc2_real)nan);
          dout.plane(k, kHalfOut[k], nullptr, (cloudsc2_real)nan);
        }
        Array<cloudsc2_real> scratch;
        if (evap) scratch.reset(extent(false), nullptr, (cloudsc2_real)nan);  // absent without the branch: NULL

        if (hostcheck_parmap_nl(&prm, ptsphy[icase], g_nproma, g_nlev, g_ngptot, par.p, &in.blk, &out.blk, scratch.p))
          return fail_at("the NL sweep refused", icase, satur, precise);
        for (int k = 0; k < kOut; ++k)
          if (!written(out.a[k].p, kHalfOut[k], k == kOut - 1)) return fail_at("NL: an output's active part or padded tail", icase, satur, precise);
        if (evap && !written(scratch.p, false)) return fail_at("NL: the cover checkpoint", icase, satur, precise);

        if (hostcheck_parmap_tl(&prm, ptsphy[icase], g_nproma, g_nlev, g_ngptot, satur, par.p, dpar.p, &in.blk, &din.blk, &dout.blk))
          return fail_at("the TL sweep refused", icase, satur, precise);
        for (int k = 0; k < kOut; ++k)
          if (!written(dout.a[k].p, kHalfOut[k])) return fail_at("TL: a tangent's active part or padded tail", icase, satur, precise);

        // the cotangent: the TL outputs themselves (NaN in the padded tail), read only
        if (hostcheck_parmap_vjp(&prm, ptsphy[icase], g_nproma, g_nlev, g_ngptot, satur, par.p, &in.blk, &out.blk, &ain.blk, &dout.blk, scratch.p,
                                 apar.p))
          return fail_at("the reverse sweep refused", icase, satur, precise);
        for (int k = 0; k < kIn; ++k)
          if (!(k == kQsat && satur) && !written(ain.a[k].p, k == 0)) return fail_at("VJP: an adjoint's active part or padded tail", icase, satur, precise);
        for (int i = 0; i < 4; ++i)
          for (size_t c = 0; c < ncp; ++c) {
            const double v = apar.p[i * ncp + c];
            if ((long long)c < g_ngptot ? v != v : v == v) return fail_at("VJP: the adjoint table's active part or padded tail", icase, satur, precise);
          }
        ++runs;
      }
  }
  printf("parmap_asan_main: %d runs of the three sweeps: every active element written, every padded tail untouched\n", runs);
  return 0;
}
