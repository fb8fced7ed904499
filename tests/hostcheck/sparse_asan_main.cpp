// TEST-ONLY: a stand-alone program (its own main, no Python) that runs the host build of the sparse TL and reverse sweeps
// (hostcheck_sparse.hip) under the host sanitizers: tests/test_sparse_asan.py compiles it with -fsanitize=address,undefined and runs it.
// Every plane that is present is a malloc of exactly its extent, every absent plane a NULL pointer, so an access through an absent
// plane's pointer or past a half-level / full-level extent is a sanitizer report.  The mask patterns are those of
// tests/sparse_patterns.py in kind (everything, each field alone on either side, the narrow case, seeded random ones); each sparse
// result is also compared with the dense twin on zero planes.
//
//   sparse_asan_main <case file>     the file (written by the test): int32 nproma, nlev, ngptot, ncases; per case the bytes of a
//                                    cloudsc2_params and a double ptsphy; then the 16 input planes (nblocks, nlevx, nproma) in the
//                                    order of cloudsc2_inputs, in the build's precision
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#define HC_SPARSE_OFF64_ONLY
#include "hostcheck_sparse.hip"

namespace {

int g_nproma, g_nlev, g_ngptot, g_nb;
const bool kHalfIn[kNumIn] = {true, false, false, false, false, false, false, false, false, false, false, false, false, false, false, false};
const bool kHalfOut[kNumOut] = {false, false, false, false, false, true, true, true, true, false};

size_t extent(bool half) { return (size_t)g_nb * (g_nlev + (half ? 1 : 0)) * g_nproma; }

struct Plane {  // a malloc of exactly the plane's extent, or nothing
  cloudsc2_real* p = nullptr;
  size_t n = 0;
  Plane() {}
  Plane(bool half, const cloudsc2_real* src, cloudsc2_real fill) { reset(half, src, fill); }
  Plane(const Plane&) = delete;
  Plane& operator=(const Plane&) = delete;
  ~Plane() { free(p); }
  void reset(bool half, const cloudsc2_real* src, cloudsc2_real fill) {  // a copy of src, or `fill` everywhere
    free(p);
    n = extent(half);
    p = (cloudsc2_real*)malloc(n * sizeof(cloudsc2_real));
    for (size_t i = 0; i < n; ++i) p[i] = src ? src[i] : fill;
  }
};

template <class Block, int N>
struct Planes {  // the planes of one argument block
  Plane pl[N];
  Block blk;
  Planes() { memset(&blk, 0, sizeof(blk)); }
  void set(int k, bool half, const cloudsc2_real* src, cloudsc2_real fill) {
    pl[k].reset(half, src, fill);
    cloudsc2_field* f = reinterpret_cast<cloudsc2_field*>(&blk) + k;
    f->ptr = pl[k].p;
    f->block_stride = (long long)(g_nlev + (half ? 1 : 0)) * g_nproma;
  }
};
typedef Planes<cloudsc2_inputs, kNumIn> InPlanes;
typedef Planes<cloudsc2_outputs, kNumOut> OutPlanes;

int fail_at(const char* what, const char* sweep, int icase, int satur, int precise, unsigned mi, unsigned mo) {
  fprintf(stderr, "sparse_asan_main: %s (%s, case %d, satur %d, precise %d, input mask 0x%x, output mask 0x%x)\n", what, sweep, icase, satur,
          precise, mi, mo);
  return 1;
}

// the active columns of a written plane: all written (no NaN left), the dense twin's bits; the padded tail still NaN
bool plane_ok(const Plane& got, const Plane& want, bool half) {
  const int nlevx = g_nlev + (half ? 1 : 0);
  for (int ibl = 0; ibl < g_nb; ++ibl)
    for (int jk = 0; jk < nlevx; ++jk)
      for (int jl = 0; jl < g_nproma; ++jl) {
        const size_t i = ((size_t)ibl * nlevx + jk) * g_nproma + jl;
        const bool active = (long long)ibl * g_nproma + jl < g_ngptot;
        if (active ? memcmp(&got.p[i], &want.p[i], sizeof(cloudsc2_real)) != 0 : got.p[i] == got.p[i]) return false;
      }
  return true;
}

struct Pattern { unsigned in, out; };

std::vector<Pattern> patterns(int satur) {
  const unsigned all_in = satur ? (C2I_ALL & ~C2I_QSAT) : C2I_ALL;
  std::vector<Pattern> p;
  p.push_back({all_in, C2O_ALL});
  for (int k = 0; k < kNumOut; ++k) p.push_back({all_in, 1u << k});
  for (int k = 0; k < kNumIn; ++k)
    if (all_in & (1u << k)) p.push_back({1u << k, C2O_ALL});
  p.push_back({C2I_Q | C2I_T, C2O_FPLSL | C2O_FPLSN});  // the narrow case
  uint64_t s = 20261019u + (unsigned)satur;
  for (int k = 0; k < 8;) {  // seeded random patterns
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    const unsigned in = (unsigned)(s >> 20) & all_in, out = (unsigned)(s >> 40) & C2O_ALL;
    if (in && out) { p.push_back({in, out}); ++k; }
  }
  return p;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: sparse_asan_main <case file>\n"); return 2; }
  FILE* fp = fopen(argv[1], "rb");
  if (!fp) { fprintf(stderr, "sparse_asan_main: cannot open %s\n", argv[1]); return 2; }
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

  long long runs = 0;
  for (int c = 0; c < ncases; ++c)
    for (int satur = 0; satur < 2; ++satur)
      for (int precise = 0; precise < 2; ++precise) {
        hostcheck_set_precise(precise);
        const cloudsc2_params* prm = &prms[c];
        const unsigned all_in = satur ? (C2I_ALL & ~C2I_QSAT) : C2I_ALL;
        // the trajectory: complete
        InPlanes x;
        for (int k = 0; k < kNumIn; ++k)
          if (all_in & (1u << k)) x.set(k, kHalfIn[k], state[k].data(), 0);
        OutPlanes traj;
        for (int k = 0; k < kNumOut; ++k) traj.set(k, kHalfOut[k], nullptr, 0);
        Plane scratch(false, nullptr, 0);
        if (hostcheck_sparse_forward(prm, ptsphy[c], g_nproma, g_nlev, g_ngptot, &x.blk, &traj.blk, scratch.p)) return 1;
        // the full tangent v = 0.01 x and the cotangent u = TL v
        std::vector<std::vector<cloudsc2_real>> v(kNumIn);
        for (int k = 0; k < kNumIn; ++k) {
          v[k] = state[k];
          for (auto& e : v[k]) e *= (cloudsc2_real)0.01;
        }
        OutPlanes u;
        {
          InPlanes dx;
          for (int k = 0; k < kNumIn; ++k)
            if (all_in & (1u << k)) dx.set(k, kHalfIn[k], v[k].data(), 0);
          for (int k = 0; k < kNumOut; ++k) u.set(k, kHalfOut[k], nullptr, 0);
          if (hostcheck_sparse_tl(prm, ptsphy[c], g_nproma, g_nlev, g_ngptot, satur, 0, &x.blk, &dx.blk, &u.blk)) return 1;
        }
        for (const Pattern& pt : patterns(satur)) {
          {  // TL: tangents pt.in read, output tangents pt.out stored
            InPlanes dx, dz;
            OutPlanes dy, dw;
            for (int k = 0; k < kNumIn; ++k) {
              if (!(all_in & (1u << k))) continue;
              if (pt.in & (1u << k)) dx.set(k, kHalfIn[k], v[k].data(), 0);
              dz.set(k, kHalfIn[k], (pt.in & (1u << k)) ? v[k].data() : nullptr, 0);  // the twin's: zero planes for the absent
            }
            for (int k = 0; k < kNumOut; ++k) {
              if (pt.out & (1u << k)) dy.set(k, kHalfOut[k], nullptr, nan);
              dw.set(k, kHalfOut[k], nullptr, nan);
            }
            if (hostcheck_sparse_tl(prm, ptsphy[c], g_nproma, g_nlev, g_ngptot, satur, 1, &x.blk, &dx.blk, &dy.blk) ||
                hostcheck_sparse_tl(prm, ptsphy[c], g_nproma, g_nlev, g_ngptot, satur, 0, &x.blk, &dz.blk, &dw.blk))
              return fail_at("a sweep refused its arguments", "TL", c, satur, precise, pt.in, pt.out);
            for (int k = 0; k < kNumOut; ++k)
              if ((pt.out & (1u << k)) && !plane_ok(dy.pl[k], dw.pl[k], kHalfOut[k]))
                return fail_at("a stored plane differs from the dense twin, has an unwritten active element or a written tail", "TL", c, satur,
                               precise, pt.in, pt.out);
            runs += 2;
          }
          {  // reverse sweep: cotangents pt.out read, gradients pt.in written
            InPlanes xa, xw;
            OutPlanes y, yz;
            for (int k = 0; k < kNumIn; ++k) {
              if (!(all_in & (1u << k))) continue;
              if (pt.in & (1u << k)) xa.set(k, kHalfIn[k], nullptr, nan);
              xw.set(k, kHalfIn[k], nullptr, nan);
            }
            for (int k = 0; k < kNumOut; ++k) {
              if (pt.out & (1u << k)) y.set(k, kHalfOut[k], u.pl[k].p, 0);
              yz.set(k, kHalfOut[k], (pt.out & (1u << k)) ? u.pl[k].p : nullptr, 0);
            }
            if (hostcheck_sparse_vjp(prm, ptsphy[c], g_nproma, g_nlev, g_ngptot, satur, 1, &x.blk, &traj.blk, &xa.blk, &y.blk, scratch.p) ||
                hostcheck_sparse_vjp(prm, ptsphy[c], g_nproma, g_nlev, g_ngptot, satur, 0, &x.blk, &traj.blk, &xw.blk, &yz.blk, scratch.p))
              return fail_at("a sweep refused its arguments", "reverse", c, satur, precise, pt.in, pt.out);
            for (int k = 0; k < kNumIn; ++k)
              if ((pt.in & (1u << k)) && !plane_ok(xa.pl[k], xw.pl[k], kHalfIn[k]))
                return fail_at("a stored plane differs from the dense twin, has an unwritten active element or a written tail", "reverse", c,
                               satur, precise, pt.in, pt.out);
            runs += 2;
          }
        }
      }
  hostcheck_set_precise(0);
  printf("sparse_asan_main: %lld sweeps, every present plane the dense twin's bits\n", runs);
  return 0;
}
