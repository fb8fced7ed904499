// cloudsc2_launch.hip -- the launchers of the CLOUDSC2 NL/TL/AD engine's C ABI (include/cloudsc2_hip.h), what they check and share,
// and the small kernels only they launch.
//
// Mapping: one lane = one grid column, lanes run over the global column index g = ibl*NPROMA + jl of the
// reference's (NPROMA, NLEV, NBLOCKS) layout, so a wave64 reads 64 consecutive doubles (512 B) of every
// input plane per level: fully coalesced for any NPROMA (for NPROMA in {64,128,256} and blockDim = NPROMA one
// thread block is exactly one NPROMA block).  The 137-level sweep is sequential per lane with three carried
// scalars; inputs of level JK+1 are requested before level JK is computed (register double buffer).
// There is no MFMA (pointwise physics) and no inter-lane traffic in the kernels proper; wave/LDS reductions
// appear only in the two test-norm kernels.

#include "cloudsc2_host.hpp"
#ifdef C2_SINGLE_TU  // one translation unit (experiment / diagnostic builds): every row's table here, in place of the family units
namespace cloudsc2 {
C2_KERNEL_TABLES(C2_DEFINE_VARIANT)
}  // namespace cloudsc2
#endif

using namespace cloudsc2;

namespace {

// ---------------------------------------------------------------------------------------------------------
// kernels: the sweeps' __global__ wrappers and the table of their variant tables are cloudsc2_sweep_kernels.hpp, the tables themselves
// the family units (cloudsc2_kern.hip per name of the Makefile's FAMILIES); here: SATUR as a kernel of its own, the data-format kernels and the test-norm kernels
// ---------------------------------------------------------------------------------------------------------
template <bool P>
__global__ void __launch_bounds__(kBlock) satur_kernel(SaturArgs args) {
  C2_KERNEL_BODY(satur_column<P>(global_column(), kernarg<SaturArgs>()));
}
template <bool P>
__global__ void __launch_bounds__(kBlock) satur_lin_kernel(SaturLinArgs args) {
  C2_KERNEL_BODY(satur_lin_column<P>(global_column(), kernarg<SaturLinArgs>()));
}

// The second kernel of cloudsc2_vjp_launch_par: row blockIdx.x of the reverse sweep's workspace (the active columns' sums of one
// parameter) folded into one double in a fixed order -- thread t adds columns t, t + 1024, ... in turn, then a fixed tree over the
// threads -- so the result is the same bits from run to run.  Columns from ngptot on (the padded tail) were not written and are not read.
constexpr int kParFoldBlock = 1024;
__device__ __forceinline__ void fold_row(const double* __restrict__ work, long long ncols_pad, long long ngptot, double* __restrict__ sums) {
  __shared__ double red[kParFoldBlock];
  const double* row = work + (long long)blockIdx.x * ncols_pad;
  double v = 0.0;
  for (long long g = threadIdx.x; g < ngptot; g += kParFoldBlock) v += row[g];
  red[threadIdx.x] = v;
  __syncthreads();
  for (int off = kParFoldBlock / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) sums[blockIdx.x] = red[0];
}
__global__ void __launch_bounds__(kParFoldBlock)
par_fold_kernel(const double* __restrict__ work, long long ncols_pad, long long ngptot, double* __restrict__ par_adj) {
  fold_row(work, ncols_pad, ngptot, par_adj);
}
// Its sibling for a workspace some of whose rows were not written (cloudsc2_parnormal_launch without the evaporation branch: the rows
// with rpecons): a row whose bit is set in `unwritten` is not read and its sum is stored as the exact zero it stands for.
__global__ void __launch_bounds__(kParFoldBlock)
par_fold_rows_kernel(const double* __restrict__ work, long long ncols_pad, long long ngptot, unsigned unwritten, double* __restrict__ sums) {
  if ((unwritten >> blockIdx.x) & 1u) {  // (block-uniform)
    if (threadIdx.x == 0) sums[blockIdx.x] = 0.0;
    return;
  }
  fold_row(work, ncols_pad, ngptot, sums);
}
// The fold of cloudsc2_vjp_launch_ens: grid (PAR_COUNT, members), member blockIdx.y's rows folded like par_fold_kernel folds them.
__global__ void __launch_bounds__(kParFoldBlock)
par_fold_ens_kernel(const double* __restrict__ work, long long ncols_pad, long long ngptot, double* __restrict__ par_adj) {
  fold_row(work + (long long)blockIdx.y * PAR_COUNT * ncols_pad, ncols_pad, ngptot, par_adj + (long long)blockIdx.y * PAR_COUNT);
}

// The first kernel of every ensemble launcher: thread k writes member k's argument block to the workspace (ens_member_args: the template
// block with its pointers advanced and its constants derived from row k of `params`, and of `dparams` if given; plain stores).
constexpr int kEnsArgsBlock = 64;
template <class Args>
__global__ void __launch_bounds__(kEnsArgsBlock)
ens_args_kernel(Args tmpl, EnsStrides ms, double ptsphy, int members, const double* __restrict__ params,
                const double* __restrict__ dparams, Args* __restrict__ blocks) {
  const long long k = (long long)blockIdx.x * kEnsArgsBlock + threadIdx.x;
  if (k >= members) return;
  ens_member_args(blocks[k], tmpl, ms, ptsphy, k, params + k * PAR_COUNT, dparams ? dparams + k * PAR_COUNT : nullptr);
}
static_assert(sizeof(AdParArgs) + sizeof(EnsStrides) + 64 <= 4096 && sizeof(TlParArgs) + sizeof(EnsStrides) + 64 <= 4096 &&
                  sizeof(AdEnsColsumArgs) + sizeof(EnsStrides) + 64 <= 4096 && sizeof(TlEnsColsumArgs) + sizeof(EnsStrides) + 64 <= 4096,
              "ens_args_kernel's arguments fit the kernel-argument segment");

// ---------------------------------------------------------------------------------------------------------
// Data-format kernels either side of the path: the input file holds KLON (=100) columns,
// the model state is their periodic tiling into NPROMA blocks (expand_mod.F90:270-335), and the validator compares
// the outputs with a KLON-column reference (validate_mod.F90:165-261).  Both work from the small table on the
// device, so a 1M-column state never exists on the host and the reference is never expanded at all.
// ---------------------------------------------------------------------------------------------------------
// field(jl, jk, jm, ibl) = table((start + (ibl*NPROMA + jl) mod period) mod KLON, jk, jm) for active columns, 0 for the
// padded tail of the last block: the rank's table slice START..END (get_offsets, expand_mod.F90:30-46) tiled with period
// SIZE (load_and_expand + expand_r2, :101-116,283-296).  The outer mod KLON never acts for those pairs (start + period <= KLON);
// it lets period = KLON with any start >= 0 express "the periodic tiling continues at global column `start`".
__global__ void __launch_bounds__(256)
expand_kernel(const real_t* __restrict__ table, int klon, int period, long long start, int nlevx, int ndim, int nproma,
              long long ngptot, long long nblocks, real_t* __restrict__ field, long long block_stride) {
  const long long per_block = (long long)nproma * nlevx * ndim;
  const long long total = per_block * nblocks;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const long long ibl = e / per_block;
    const long long r = e - ibl * per_block;
    const int jl = (int)(r % nproma);
    const long long lev = r / nproma;  // jk + nlevx*jm
    const long long g = ibl * nproma + jl;
    real_t v = 0;
    if (g < ngptot) v = table[(start + g % period) % klon + (long long)klon * lev];
    field[ibl * block_stride + r] = v;
  }
}

// Per-workgroup partial statistics of VALIDATE_R2/R3 (validate_mod.F90:165-261): min and max of FIELD over whole
// blocks (padding included, like MINVAL(FIELD(:,:,B))), max |FIELD-REF|, sum |FIELD-REF|, sum |REF| over the active
// columns.  part[5*blockIdx.x + {0..4}]; a second launch folds the partials in a fixed order (deterministic sums).
__global__ void __launch_bounds__(256)
validate_partial_kernel(const real_t* __restrict__ table, int klon, int period, long long start, int nlevx, int ndim,
                        int nproma, long long ngptot, long long nblocks, const real_t* __restrict__ field,
                        long long block_stride, double* __restrict__ part, long long ncols_minmax) {
  const long long per_block = (long long)nproma * nlevx * ndim;
  const long long total = per_block * nblocks;
  double vmin = INFINITY, vmax = -INFINITY, emax = 0.0, esum = 0.0, rsum = 0.0;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const long long ibl = e / per_block;
    const long long r = e - ibl * per_block;
    const int jl = (int)(r % nproma);
    const long long lev = r / nproma;
    const long long g = ibl * nproma + jl;
    const double f = field[ibl * block_stride + r];
    if (g < ncols_minmax) {  // MINVAL / MAXVAL run over whole blocks of the CALLER's blocking (resident states may be blocked otherwise)
      vmin = fmin(vmin, f);
      vmax = fmax(vmax, f);
    }
    if (g < ngptot) {
      const double ref = table[(start + g % period) % klon + (long long)klon * lev];
      const double d = fabs(f - ref);
      emax = fmax(emax, d);
      esum += d;
      rsum += fabs(ref);
    }
  }
  __shared__ double red[5][4];
  for (int off = 32; off > 0; off >>= 1) {
    vmin = fmin(vmin, __shfl_down(vmin, off, 64));
    vmax = fmax(vmax, __shfl_down(vmax, off, 64));
    emax = fmax(emax, __shfl_down(emax, off, 64));
    esum += __shfl_down(esum, off, 64);
    rsum += __shfl_down(rsum, off, 64);
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[0][w] = vmin; red[1][w] = vmax; red[2][w] = emax; red[3][w] = esum; red[4][w] = rsum; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < 4; ++i) {
      red[0][0] = fmin(red[0][0], red[0][i]); red[1][0] = fmax(red[1][0], red[1][i]); red[2][0] = fmax(red[2][0], red[2][i]);
      red[3][0] += red[3][i]; red[4][0] += red[4][i];
    }
    for (int k = 0; k < 5; ++k) part[5 * (long long)blockIdx.x + k] = red[k][0];
  }
}

// fold_zero: the caller's blocking has padded columns the field's own blocking does not hold (caller NPROMA 100 pads 256 columns to
// 300, the device's 2 x 128 blocks have none): they are zero in the caller's arrays and MINVAL / MAXVAL(FIELD(:,:,B)) include them
__global__ void validate_final_kernel(const double* __restrict__ part, int nparts, double* __restrict__ stats, int fold_zero) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double vmin = fold_zero ? 0.0 : INFINITY, vmax = fold_zero ? 0.0 : -INFINITY, emax = 0.0, esum = 0.0, rsum = 0.0;
  for (int i = 0; i < nparts; ++i) {
    vmin = fmin(vmin, part[5 * i + 0]); vmax = fmax(vmax, part[5 * i + 1]); emax = fmax(emax, part[5 * i + 2]);
    esum += part[5 * i + 3]; rsum += part[5 * i + 4];
  }
  stats[0] = vmin; stats[1] = vmax; stats[2] = emax; stats[3] = esum; stats[4] = rsum;
}

// ---------------------------------------------------------------------------------------------------------
// Test-norm kernels
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool lane_setup_v(const Geom& g, const Strides& s, long long gcol, LaneOff& o, bool& active) {
  if (gcol >= g.ncols_pad) return false;
  long long ibl = gcol / g.nproma;
  long long jl = gcol - ibl * g.nproma;
  o.full = ibl * s.full + jl; o.half = ibl * s.half + jl; o.cml = ibl * s.cml + jl; o.clv = ibl * s.clv + jl;
  o.loc = ibl * s.loc + jl;
  active = gcol < g.ngptot;
  return true;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// ERROR_NORM sums (cloudsc_driver_tl_mod.F90:21-31): one thread block per NPROMA block, lanes stride the
// block's active columns, per-lane level sums, wave shuffles, then one LDS stage.
// sums[(ibl*10 + f)*2 + {0,1}] = { sum(F - F5), sum(TL*lambda) }.
// (TenPtrs: cloudsc2_column.hpp)

// The 256 threads of a workgroup are laid over the block as (column, level slice): all of them work whatever NPROMA is -- with one
// thread per column only, the README's NPROMA 32 left 7 of 8 lanes idle.  (For ONE lambda and perturbed outputs that are in memory;
// the Taylor driver itself runs all ten lambdas in one sweep that stores nothing, taylor_kernel + taylor_reduce_kernel.)
__global__ void __launch_bounds__(256) taylor_sums_kernel(int nproma, int nlev, int ngptot, TenPtrs f, TenPtrs f5, TenPtrs tl,
                                                          double lambda, double* sums) {
  (void)nlev;
  const int ibl = blockIdx.x;
  const int icend = min(nproma, ngptot - ibl * nproma);
  const int ncolt = min(nproma, (int)blockDim.x);    // threads along the columns
  const int nslice = (int)blockDim.x / ncolt;        // level slices (>= 1)
  const int jl0 = threadIdx.x % ncolt, slice = threadIdx.x / ncolt;
  __shared__ double red[2][4];
  for (int fi = 0; fi < 10; ++fi) {
    double s0 = 0.0, s1 = 0.0;
    const int nl = f.nlevx[fi];
    if (slice < nslice) {
      for (int jl = jl0; jl < icend; jl += ncolt) {
        const real_t* a = f.p[fi] + (long long)ibl * f.stride[fi] + jl;
        const real_t* b = f5.p[fi] + (long long)ibl * f5.stride[fi] + jl;
        const real_t* t = tl.p[fi] + (long long)ibl * tl.stride[fi] + jl;
        for (int jk = slice; jk < nl; jk += nslice) {
          long long d = (long long)jk * nproma;
          s0 += a[d] - b[d];
          s1 += t[d] * lambda;
        }
      }
    }
    s0 = wave_sum(s0);
    s1 = wave_sum(s1);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[0][w] = s0; red[1][w] = s1; }
    __syncthreads();
    if (threadIdx.x == 0) {
      double r0 = 0.0, r1 = 0.0;
      for (int i = 0; i < (int)(blockDim.x >> 6); ++i) { r0 += red[0][i]; r1 += red[1][i]; }
      sums[((long long)ibl * 10 + fi) * 2 + 0] = r0;
      sums[((long long)ibl * 10 + fi) * 2 + 1] = r1;
    }
    __syncthreads();
  }
}

// Second stage of the Taylor sweep: the per-column level sums of taylor_kernel summed over the active columns of each block of
// the STATISTIC (ERROR_NORM sums over one block of the caller's NPROMA), in column order (deterministic), into the layout of
// taylor_sums_kernel: sums[((il*nblocks + ibl)*10 + f)*2 + {0,1}] = { sum(F - F5(lambda_il)), sum(TL)*lambda_il }.
struct TenLambdas { double v[kTaylorLambdas]; };
__global__ void __launch_bounds__(128) taylor_reduce_kernel(int nproma, int ngptot, long long ncols_pad, long long nblocks, TenLambdas lam,
                                                            const double* colsum, double* sums) {
  const long long ibl = blockIdx.x;
  const int t = threadIdx.x;
  if (t >= 10 * kTaylorLambdas) return;
  const int il = t / 10, f = t - 10 * il;
  const long long c0 = ibl * nproma;
  const int icend = (int)min((long long)nproma, (long long)ngptot - c0);
  const double* s1 = colsum + (long long)t * ncols_pad + c0;
  const double* s2 = colsum + (long long)(10 * kTaylorLambdas + f) * ncols_pad + c0;
  double r0 = 0.0, r1 = 0.0;
  for (int j = 0; j < icend; ++j) { r0 += s1[j]; r1 += s2[j]; }
  double* o = sums + (((long long)il * nblocks + ibl) * 10 + f) * 2;
  o[0] = r0;
  o[1] = r1 * lam.v[il];
}

// The same for LARGE blocks of the statistic (one thread per value would walk thousands of columns one after the other): one
// workgroup per (block, value), its threads stride the block's columns, fixed-order reduction (wave shuffles, one LDS stage) --
// deterministic as well.  blockIdx.y < 100: sum(F - F5) of (lambda, field) = blockIdx.y; 100..109: sum(TL) of field blockIdx.y - 100,
// written once per lambda with its factor.
__global__ void __launch_bounds__(256) taylor_reduce_wide_kernel(int nproma, int ngptot, long long ncols_pad, long long nblocks, TenLambdas lam,
                                                                 const double* colsum, double* sums) {
  const long long ibl = blockIdx.x;
  const int t = blockIdx.y;
  const long long c0 = ibl * nproma;
  const int icend = (int)min((long long)nproma, (long long)ngptot - c0);
  const double* src = colsum + (long long)t * ncols_pad + c0;
  double r = 0.0;
  for (int j = threadIdx.x; j < icend; j += blockDim.x) r += src[j];
  r = wave_sum(r);
  __shared__ double red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = r;
  __syncthreads();
  if (threadIdx.x != 0) return;
  r = (red[0] + red[1]) + (red[2] + red[3]);
  if (t < 10 * kTaylorLambdas) {
    const int il = t / 10, f = t - 10 * il;
    sums[(((long long)il * nblocks + ibl) * 10 + f) * 2 + 0] = r;
  } else {
    const int f = t - 10 * kTaylorLambdas;
    for (int il = 0; il < kTaylorLambdas; ++il) sums[(((long long)il * nblocks + ibl) * 10 + f) * 2 + 1] = r * lam.v[il];
  }
}

// Adjoint-test norms (cloudsc_driver_ad_mod.F90:184-195,240-264): lane = column, level sums in registers
// (cloudsc2_column.hpp), wave max by shuffles, one atomic max per wave.
__global__ void __launch_bounds__(kBlock) adjoint_norm1_kernel(Geom g, Strides sa, OutPtrs y, double* norms) {
  long long gcol = global_column();
  LaneOff oa; bool active;
  if (!lane_setup_v(g, sa, gcol, oa, active) || !active) return;
  norms[gcol] = adjoint_norm1_column(g.nlev, g.nproma, oa, y);
}

__global__ void __launch_bounds__(kBlock)
adjoint_norm2_kernel(Geom g, Strides s, Strides sa, InPtrs in, const real_t* qsat, long long qsat_stride, InPtrs xa,
                     double* norms, long long ncols_pad, double* gmax) {
  long long gcol = global_column();
  LaneOff o, oa; bool active;
  double n3 = 0.0;
  if (lane_setup_v(g, s, gcol, o, active) && active) {
    lane_setup_v(g, sa, gcol, oa, active);
    const long long oq = (gcol / g.nproma) * qsat_stride + (gcol % g.nproma);
    double n2 = adjoint_norm2_column(g.nlev, g.nproma, o, oa, oq, in, qsat, xa);
    double n1 = norms[gcol];
    n3 = adjoint_norm3(n1, n2);
    norms[ncols_pad + gcol] = n2;
    norms[2 * ncols_pad + gcol] = n3;
    n3 = fabs(n3);
    if (!(n3 == n3)) n3 = __longlong_as_double(0x7ff0000000000000LL);  // NaN counts as failure (+inf)
  }
  double m = wave_max(n3);
  if ((threadIdx.x & 63) == 0) atomic_max_pos(gmax, m);
}
}  // namespace

namespace cloudsc2 {

// ---------------------------------------------------------------------------------------------------------
// error handling
// ---------------------------------------------------------------------------------------------------------
thread_local std::string g_err;

int fail(int code, const char* msg) {
  g_err = msg;
  return code;
}

bool device_ok() {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) { (void)hipGetLastError(); return false; }
  return n > 0;
}

int no_device() { return fail(CLOUDSC2_ENODEVICE, "no HIP device available (this library has no CPU path)"); }

// The calling thread's launch log (cloudsc2_debug_launch_log): the first kLaunchLogMax sweep kernels enqueued since the reset, and how
// many there were in all.  Plain thread-local integers: no allocation, no lock, no device call.
namespace {
constexpr int kLaunchLogMax = 64;
struct LaunchLog {
  long long count;
  int family[kLaunchLogMax];
  unsigned word[kLaunchLogMax];
};
thread_local LaunchLog g_launch_log = {};
}  // namespace

void log_launch(int family, unsigned word) {
  LaunchLog& l = g_launch_log;
  if (l.count < kLaunchLogMax) { l.family[l.count] = family; l.word[l.count] = word; }
  if (l.count < 0x7fffffff) ++l.count;
}

// 0 = fast math (shared reciprocals, branch-free exp), 1 = precise (IEEE division, libm exp/tanh, reference order)
namespace {
int initial_math_mode() {
  const char* e = getenv("CLOUDSC2_MATH");
  return (e && (!strcmp(e, "precise") || !strcmp(e, "1"))) ? 1 : 0;
}
std::atomic<int> g_precise{initial_math_mode()};
}  // namespace

// arithmetic of one call: the call's own request, else the process default (read, never written, by the launchers)
bool precise_of(const cloudsc2_params* prm) {
  if (prm->math_mode == 2) return true;
  if (prm->math_mode == 1) return false;
  return g_precise.load() != 0;
}

// ---------------------------------------------------------------------------------------------------------
// launch-invariant constants and per-level tables
// ---------------------------------------------------------------------------------------------------------
// Device copies of the level tables are immutable once created and keyed by content, so launches on
// different streams never race on them.
namespace {
struct TabEntry {
  int device;
  int nlev;
  std::vector<double> ceta;
  LevelTab* dev;
  int kb0, kb1;  // tropopause band: levels jk (0-based) in [kb0,kb1) can have 0.1 < ceta < 0.4 and jk < nlev-1
};
std::mutex g_tab_mutex;
std::vector<TabEntry> g_tabs;
}  // namespace

int get_tables(const cloudsc2_params& p, const LevelTab** dev, int* kb0, int* kb1) {
  int device = 0;
  HIP_TRY(hipGetDevice(&device));
  std::lock_guard<std::mutex> lock(g_tab_mutex);
  for (auto& e : g_tabs) {
    if (e.device == device && e.nlev == p.nlev && memcmp(e.ceta.data(), p.ceta, sizeof(double) * p.nlev) == 0) {
      *dev = e.dev; *kb0 = e.kb0; *kb1 = e.kb1;
      return 0;
    }
  }
  // CETA is a property of the vertical grid: a process sees one or two of them.  A caller that varies it per call would
  // grow the cache without bound, so it is capped; an evicted table must not be freed while a launch may still read it,
  // hence the device-wide synchronisation (rare by construction).
  constexpr size_t kMaxTables = 16;
  if (g_tabs.size() >= kMaxTables) {
    HIP_TRY(hipDeviceSynchronize());
    (void)hipFree(g_tabs.front().dev);
    g_tabs.erase(g_tabs.begin());
  }
  TabEntry e;
  e.device = device;
  e.nlev = p.nlev;
  e.ceta.assign(p.ceta, p.ceta + p.nlev);
  LevelTab host;
  memset(&host, 0, sizeof(host));
  e.kb0 = p.nlev; e.kb1 = 0;
  for (int jk = 0; jk < p.nlev; ++jk) {
    host.lev[jk].ceta = p.ceta[jk];
    // cloudsc2.F90:266  ZSCALM(JK)=ZSCAL*MAX((CETA(JK)-0.2),ZEPS1)**0.2, ZSCAL=0.9 (:172)
    host.lev[jk].zscalm = 0.9 * pow(fmax(p.ceta[jk] - 0.2, 1.e-12), 0.2);
    if (jk < p.nlev - 1 && p.ceta[jk] > 0.1 && p.ceta[jk] < 0.4) {  // cloudsc2.F90:318-321
      if (jk < e.kb0) e.kb0 = jk;
      if (jk + 1 > e.kb1) e.kb1 = jk + 1;
    }
  }
  if (e.kb1 <= e.kb0) { e.kb0 = 0; e.kb1 = 0; }
  // (a launcher may be the first to ask for this table, possibly while ANOTHER stream of the process is being captured into a graph:
  //  the thread's capture mode is relaxed for the allocation, and the upload goes through a private non-blocking stream instead of
  //  the legacy stream, which would synchronise with -- and invalidate -- such a capture.  A launch on a stream that is itself
  //  capturing needs its table to exist already: any earlier launch, cloudsc2_state_* call or driver call with the same CETA made it.)
  {
    hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
    const bool exchanged = hipThreadExchangeStreamCaptureMode(&mode) == hipSuccess;
    hipStream_t up = nullptr;
    hipError_t err = hipStreamCreateWithFlags(&up, hipStreamNonBlocking);
    if (err == hipSuccess) err = hipMalloc((void**)&e.dev, sizeof(LevelTab));
    if (err == hipSuccess) err = hipMemcpyAsync(e.dev, &host, sizeof(LevelTab), hipMemcpyHostToDevice, up);
    if (err == hipSuccess) err = hipStreamSynchronize(up);
    if (up) (void)hipStreamDestroy(up);
    if (exchanged) (void)hipThreadExchangeStreamCaptureMode(&mode);
    if (err != hipSuccess) {
      if (e.dev) (void)hipFree(e.dev);
      (void)hipGetLastError();
      g_err = std::string("level tables: ") + hipGetErrorString(err);
      return (int)err;
    }
  }
  g_tabs.push_back(e);
  *dev = e.dev; *kb0 = e.kb0; *kb1 = e.kb1;
  return 0;
}
int check_geom_args(const cloudsc2_params* prm, int nproma, int nlev, int ngptot) {
  if (!prm) return fail(CLOUDSC2_EINVAL, "params is NULL");
  if (nproma < 1 || nlev < 2 || ngptot < 1) return fail(CLOUDSC2_EINVAL, "nproma >= 1, nlev >= 2, ngptot >= 1 required");
  if (nlev > CLOUDSC2_MAX_NLEV) return fail(CLOUDSC2_EINVAL, "nlev exceeds CLOUDSC2_MAX_NLEV");
  if (prm->nlev != nlev) return fail(CLOUDSC2_EINVAL, "params.nlev does not match nlev");
  if (prm->math_mode < 0 || prm->math_mode > 2) return fail(CLOUDSC2_EINVAL, "params.math_mode must be 0 (default), 1 (fast) or 2 (precise)");
  return 0;
}
void fill_geom(Geom& g, int nproma, int nlev, int ngptot) {
  g.nproma = nproma; g.nlev = nlev; g.ngptot = ngptot; g.ncols_pad = ncols_pad(nproma, ngptot);
  g.kb0 = 0; g.kb1 = 0; g.fair = 0;
}
int check_geom(const cloudsc2_params* prm, int nproma, int nlev, int ngptot, Geom& g) {
  if (int rc = check_geom_args(prm, nproma, nlev, ngptot)) return rc;
  if (!device_ok()) return no_device();
  fill_geom(g, nproma, nlev, ngptot);
  return 0;
}
namespace {

// What an ensemble launcher hands its parent's implementation: the parent checks the call and builds the argument block exactly as for
// its own launch (from the caller's parameter block: the template), then ens_launch runs it for `members` members instead.
struct EnsSpec {
  int members;
  const double* params;   // device, (members, PAR_COUNT)
  const double* dparams;  // device, (members, PAR_COUNT): the parameter tangents (TL), else NULL
  EnsStrides ms;
  void* workspace;        // device, cloudsc2_ens_workspace_bytes()
  double* par_adj;        // device, (members, PAR_COUNT): the parameter adjoints (reverse sweep), else NULL
};
const Geom& geom_of(const NlArgs& a) { return a.g; }
const Geom& geom_of(const TlParArgs& a) { return a.a.g; }
const Geom& geom_of(const AdParArgs& a) { return a.a.nl.g; }
const Geom& geom_of(const NlColsumArgs& a) { return a.a.g; }
const Geom& geom_of(const TlEnsColsumArgs& a) { return a.a.a.a.g; }
const Geom& geom_of(const AdEnsColsumArgs& a) { return a.a.a.a.nl.g; }
constexpr size_t kEnsBlockBytes = std::max({sizeof(NlArgs), sizeof(TlParArgs), sizeof(AdParArgs), sizeof(NlColsumArgs), sizeof(TlEnsColsumArgs),
                                            sizeof(AdEnsColsumArgs)});
size_t ens_blocks_bytes(int members) { return ((size_t)members * kEnsBlockBytes + 255) / 256 * 256; }

// Two launches, neither paced nor logged: the members' argument blocks, then the sweep over members x ceil(ncols_pad / kBlock) workgroups.
template <class Args>
int ens_launch(KernelFn<EnsArgs<Args>> fn, const Args& tmpl, double ptsphy, const EnsSpec& e, hipStream_t st) {
  EnsArgs<Args> a;
  a.blocks = (Args*)e.workspace; a.wgs_per_member = grid_for(geom_of(tmpl).ncols_pad, kBlock);
  if (!fn) return launch_kernel(fn, a, 0, st);  // (its refusal comes first, and before the members' blocks are written)
  if ((long long)a.wgs_per_member * e.members > 0x7fffffffLL) return fail(CLOUDSC2_EINVAL, "ensemble: members x workgroups per member exceeds the grid limit");
  hipLaunchKernelGGL(ens_args_kernel<Args>, dim3(grid_for(e.members, kEnsArgsBlock)), dim3(kEnsArgsBlock), 0, st, tmpl, e.ms, ptsphy, e.members,
                     e.params, e.dparams, (Args*)e.workspace);
  HIP_TRY(hipGetLastError());
  return launch_kernel(fn, a, a.wgs_per_member * (unsigned)e.members, st);
}

// What a TL launch runs.  pert_in NULL: the increments are 0.01*x of the trajectory inputs (C2F_SELFINC), supsat_inc * PSUPSAT for PSUPSAT,
// and yy, if given, receives <y,y> of every column's outputs.  The other forms are given pert_in and no trajectory outputs.
struct TlMode {
  const cloudsc2_inputs* pert_in = nullptr;
  double supsat_inc = 0.0;
  double* yy = nullptr;
  bool satlin = false;           // SATUR is differentiated in the sweep (C2F_SATLIN): no qsat on either input side
  const double* dpar = nullptr;  // the parameter tangents (C2F_PARLIN)
  const EnsSpec* ens = nullptr;  // the launch runs for the members of an ensemble (needs dpar, which the members' rows replace)
};

int tl_launch_impl(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, const cloudsc2_inputs* traj_in,
                   const cloudsc2_outputs* traj_out, const cloudsc2_outputs* pert_out, void* stream, const TlMode& m) {
  const cloudsc2_inputs* pert_in = m.pert_in;
  Sweep w;
  int rc = w.begin(prm, nproma, nlev, ngptot, (!traj_in || !traj_out || !pert_out) ? "NULL argument block" : nullptr);
  if (rc) return rc;
  const int nset = outputs_given(*traj_out);
  if (nset != 0 && nset != kNumOut) return fail(CLOUDSC2_EINVAL, "traj_out: give all ten trajectory outputs or none");
  if (m.satlin && (traj_in->qsat.ptr || (pert_in && pert_in->qsat.ptr)))
    return fail(CLOUDSC2_EINVAL, "SATUR differentiated in the sweep: traj_in->qsat and pert_in->qsat must be NULL");
  if ((rc = w.trajectory(*traj_in, *traj_out, false))) return rc;
  TlArgs args;
  args.sp = Strides{0, 0, 0, 0, 0};
  if (pert_in) {
    if ((rc = resolve_in(*pert_in, !m.satlin, args.sp, args.din))) return rc;
  } else {
    memset(&args.din, 0, sizeof(args.din));  // (sp: taken from the outputs by resolve_out)
  }
  if ((rc = resolve_out(*pert_out, true, args.sp, args.dout))) return rc;
  const Strides& sp = args.sp;
  if ((rc = w.finish(*prm, ptsphy, traj_in->qsat.ptr, {sp.full, sp.half, sp.cml, sp.clv, sp.loc}))) return rc;
  if (!pert_in) w.f |= C2F_SELFINC;
  if (nset == kNumOut) w.f |= C2F_TRAJ;
  if (m.satlin) w.f |= C2F_SATLIN;
  args.c = w.c; args.g = w.g; args.s = w.s; args.in = w.in; args.out = w.out; args.tab = w.tab;
  args.supsat_inc = (real_t)m.supsat_inc;
  args.yy = m.yy;
  const hipStream_t st = (hipStream_t)stream;
  if (!m.dpar) {
    if (m.ens) return fail(CLOUDSC2_EINVAL, "ensemble: the parameter form of the TL sweep (dpar) is required");
    schedule_tl(args.g, w.f, (const void*)tl_variant(w.f));
    return launch_variant(kFamTl, w.f, tl_variant(w.f), args, w.g.ncols_pad, st);
  }
  w.f |= C2F_PARLIN;
  TlParArgs pargs;
  pargs.a = args;
  pargs.par = make_parlin(w.c, m.dpar);  // (an ensemble's template: overwritten whole by every member's row)
  if (m.ens) return ens_launch(tl_ens_variant(w.f), pargs, ptsphy, *m.ens, st);
  schedule_tl(pargs.a.g, w.f, (const void*)tl_par_variant(w.f));
  return launch_variant(kFamTlPar, w.f, tl_par_variant(w.f), pargs, w.g.ncols_pad, st);
}

// What an AD launch runs.  which 0: both sweeps (the fused kernel, or the two kernels in stream order); 1: the trajectory pass
// alone; 2: the reverse sweep alone.  assign: the input adjoints are assigned, not accumulated.  vjp: the vector-Jacobian product.
// norms / gmax: the adjoint test's norms formed in the reverse sweep.
// satlin: the vector-Jacobian product with SATUR differentiated in the sweep (C2F_SATLIN).
struct AdMode {
  int which;
  bool assign, vjp;
  double* norms;
  double* gmax;
  bool satlin = false;
  double* par_work = nullptr;  // the vector-Jacobian product with the parameter adjoints (C2F_PARLIN): the workspace and the result
  double* par_adj = nullptr;
  const EnsSpec* ens = nullptr;  // the launch runs for the members of an ensemble (which 1, or the parameter form of which 2)
};

int ad_launch_impl(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, const cloudsc2_inputs* traj_in,
                   const cloudsc2_outputs* traj_out, const cloudsc2_inputs* adj_in, const cloudsc2_outputs* adj_out, cloudsc2_real* scratch,
                   void* stream, AdMode m) {
  Sweep w;
  int rc = w.begin(prm, nproma, nlev, ngptot,
                   (!traj_in || !traj_out || (m.which != 1 && (!adj_in || !adj_out))) ? "NULL argument block" : nullptr);
  if (rc) return rc;
  // the reverse sweep alone reads PFPLSL5 / PFPLSN5 and nothing else of the trajectory outputs
  if ((rc = w.trajectory(*traj_in, *traj_out, m.which != 2))) return rc;
  if (m.which == 2 && (!w.out.fplsl || !w.out.fplsn)) return fail(CLOUDSC2_EINVAL, "reverse sweep: traj_out->fplsl and ->fplsn (PFPLSL5, PFPLSN5) are required");
  AdArgs args;
  memset(&args, 0, sizeof(args));
  if (m.satlin && (traj_in->qsat.ptr || adj_in->qsat.ptr))
    return fail(CLOUDSC2_EINVAL, "SATUR differentiated in the sweep: traj_in->qsat and adj_in->qsat must be NULL");
  if (m.which != 1) {
    InPtrs aip_c;
    if ((rc = resolve_in(*adj_in, !m.satlin, args.sa, aip_c))) return rc;
    if ((rc = resolve_out(*adj_out, true, args.sa, args.aout))) return rc;
    args.ain = writable(*adj_in);
  }
  const Strides& sa = args.sa;
  if ((rc = w.finish(*prm, ptsphy, traj_in->qsat.ptr, {sa.full, sa.half, sa.cml, sa.clv, sa.loc, (long long)nproma * nlev /* scratch */})))
    return rc;
  if (w.c.evap && !scratch) return fail(CLOUDSC2_EINVAL, "LEVAPLS2/LDRAIN1D: the cover-checkpoint plane `scratch` is required");
  args.nl = w.nl();
  args.nl.ckpt = scratch;
  unsigned f = w.f;
  if (m.assign) f |= C2F_ASSIGN;
  if (m.vjp) {  // the vector-Jacobian product: reverse sweep alone, assign form, adj_out read only, true PSUPSAT adjoint
    if (m.which != 2 || !m.assign || m.norms) return fail(CLOUDSC2_EINVAL, "vector-Jacobian product: reverse sweep alone, assign form, no norms");
    f |= C2F_VJP;
    if (m.satlin) f |= C2F_SATLIN;
  }
  if (m.norms) {  // the adjoint test's norm2 / norm3 formed in the reverse sweep
    if (m.which != 2 || !m.assign || w.c.evap || !m.gmax) return fail(CLOUDSC2_EINVAL, "fused adjoint norms: reverse sweep alone, assign form, no evaporation branch");
    f |= C2F_ADNORM;
    args.norms = m.norms; args.gmax = m.gmax;
  }
  const hipStream_t st = (hipStream_t)stream;
  const long long n = w.g.ncols_pad;
  // the trajectory pass as a kernel of its own: the NL sweep, with the cover checkpoint when the evaporation branch is on; it runs the
  // NL kernel's three waves per SIMD, kept abreast like cloudsc2_nl_launch does (inside the fused kernel, one wave per SIMD, the
  // priority code is compiled out)
  const unsigned f_fwd = (f & ~C2F_ASSIGN) | (w.c.evap ? C2F_CKPT : 0u);
  const void* fwd = (const void*)nl_variant(f_fwd);
  const void* rev = (const void*)ad_reverse_variant(f);
  if (m.ens && m.which == 1) return ens_launch(nl_ens_variant(f_fwd), args.nl, ptsphy, *m.ens, st);
  if (m.ens && !m.par_work) return fail(CLOUDSC2_EINVAL, "ensemble: the trajectory pass or the parameter form of the reverse sweep");
  if (m.which == 1) {
    schedule(args.nl.g, fwd, false, nullptr);
    return launch_variant(kFamNl, f_fwd, nl_variant(f_fwd), args.nl, n, st);
  }
  if (m.par_work) {  // the reverse sweep with the parameter sums, then their fold
    if (!m.vjp || !m.par_adj) return fail(CLOUDSC2_EINVAL, "parameter adjoints: the vector-Jacobian product, with workspace and result");
    f |= C2F_PARLIN;
    AdParArgs pargs;
    pargs.a = args;
    pargs.par = make_parlin(w.c, nullptr);
    pargs.work = m.par_work;  // (of an ensemble: the first member's slab)
    if (m.ens) {
      if ((rc = ens_launch(vjp_ens_variant(f), pargs, ptsphy, *m.ens, st))) return rc;
      hipLaunchKernelGGL(par_fold_ens_kernel, dim3(PAR_COUNT, (unsigned)m.ens->members), dim3(kParFoldBlock), 0, st, (const double*)m.par_work, n,
                         (long long)w.g.ngptot, m.par_adj);
    } else {
      schedule(pargs.a.nl.g, nullptr, false, (const void*)vjp_par_variant(f));
      if ((rc = launch_variant(kFamVjpPar, f, vjp_par_variant(f), pargs, n, st))) return rc;
      hipLaunchKernelGGL(par_fold_kernel, dim3(PAR_COUNT), dim3(kParFoldBlock), 0, st, (const double*)m.par_work, n, (long long)w.g.ngptot, m.par_adj);
    }
    HIP_TRY(hipGetLastError());
    return 0;
  }
  if (m.which == 2) {
    schedule(args.nl.g, nullptr, false, rev);
    return launch_variant(kFamAdReverse, f, ad_reverse_variant(f), args, n, st);
  }
  if (!kAdSplitSmall || n > kAdSplitBelow) {
    schedule(args.nl.g, nullptr, false, (const void*)ad_variant(f));
    return launch_variant(kFamAd, f, ad_variant(f), args, n, st);
  }
  // trajectory pass, then the reverse pass, in stream order: one Geom carries the NL kernel's `fair` and the reverse kernel's pacing
  // (the NL kernel does not look at the pacing fields unless fair & 4)
  schedule(args.nl.g, fwd, false, rev);
  if ((rc = launch_variant(kFamNl, f_fwd, nl_variant(f_fwd), args.nl, n, st))) return rc;
  return launch_variant(kFamAdReverse, f, ad_reverse_variant(f), args, n, st);
}

}  // namespace
// refusals several launchers share (each entry point keeps its own order of them)
int check_satur(int satur) {
  return satur == 0 || satur == 1 ? 0 : fail(CLOUDSC2_EINVAL, "satur must be 0 (qsat given) or 1 (SATUR differentiated in the sweep)");
}
int require_qsat(int satur, const cloudsc2_inputs* traj_in) {
  return !satur && traj_in && !traj_in->qsat.ptr ? fail(CLOUDSC2_EINVAL, "satur = 0: traj_in->qsat is required") : 0;
}
namespace {
int check_rpecons(const cloudsc2_params* prm) {  // (its partial is formed as ZBETA / RPECONS)
  return prm && (prm->levapls2 || prm->ldrain1d) && prm->rpecons == 0.0
             ? fail(CLOUDSC2_EINVAL, "parameter derivative with the evaporation branch: rpecons must not be 0") : 0;
}
// what the two parameter launchers check before their parents' checks
int check_par(const cloudsc2_params* prm, int satur) {
  if (int rc = check_satur(satur)) return rc;
  if (int rc = require_device()) return rc;
  return check_rpecons(prm);
}
// direction b of a parameter sweep runs with the unit tangent of parameter b (the sets from `np` on are not read: valid contents all the same)
void unit_parlins(ParLin* par, const Consts& c, int np) {
  for (int b = 0; b < kBatchMax; ++b) {
    double e[PAR_COUNT] = {};
    e[b < np ? b : 0] = 1.0;
    par[b] = make_parlin(c, e);
  }
}
// the directions a parameter sweep runs: without the evaporation branch nothing depends on rpecons (parjac_directions of the kernel's flags)
int par_directions(const cloudsc2_params* prm) { return (prm->levapls2 || prm->ldrain1d) ? (int)PAR_COUNT : (int)PAR_COUNT - 1; }
// What the launchers of the three parameter sweeps share once their own blocks are resolved (tl_parjac, parnormal, parcolsum: argument
// blocks with c g s in par tab): geometry, tables, constants and flags, then the block's common members and the unit ParLin of
// every run direction.  `more`: Sweep::finish's.
template <class Args>
int par_sweep_args(Sweep& w, const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, const cloudsc2_inputs* traj_in,
                   std::initializer_list<long long> more, Args& a) {
  int rc = w.begin(prm, nproma, nlev, ngptot, nullptr);
  if (!rc) rc = w.finish(*prm, ptsphy, traj_in->qsat.ptr, more);
  if (rc) return rc;
  a.c = w.c; a.g = w.g; a.s = w.s; a.in = w.in; a.tab = w.tab;
  unit_parlins(a.par, w.c, par_directions(prm));
  return 0;
}

int work_doubles(int rows, int nproma, int ngptot, long long* n) {  // rows x the padded column count
  if (nproma < 1 || ngptot < 1 || !n) return fail(CLOUDSC2_EINVAL, "nproma >= 1, ngptot >= 1 and a result pointer required");
  *n = (long long)rows * ncols_pad(nproma, ngptot);
  return 0;
}

// what the ensemble launchers check before their parents' checks
int check_ens(const cloudsc2_params* prm, int satur, int members, const double* params_dev, const void* workspace) {
  if (int rc = check_satur(satur)) return rc;
  if (members < 1 || members > 65535) return fail(CLOUDSC2_EINVAL, "ensemble: 1 <= members <= 65535 required");
  if (!params_dev || !workspace) return fail(CLOUDSC2_EINVAL, "ensemble: the parameter array and the workspace are required");
  if (prm && !prm->lphylin) return fail(CLOUDSC2_EINVAL, "ensemble: CLOUDSC2TL / CLOUDSC2AD linearise the LPHYLIN form only (prm->lphylin = 0)");
  return 0;
}
// a block the members WRITE: with more than one member no field may be shared (member stride 0), the
// members would write over each other; then the device check, as in check_par
template <class Block>
int check_ens_unshared(const Block* b, const long long* mstride, int members) {
  for (int i = 0; b && members > 1 && i < (int)(sizeof(Block) / sizeof(cloudsc2_field)); ++i)
    if (fields_of(*b)[i].ptr && (!mstride || mstride[i] == 0))
      return fail(CLOUDSC2_EINVAL, "ensemble: a field the members write has member stride 0 (every member needs its own)");
  return 0;
}
template <class Block>
int check_ens_written(const Block* b, const long long* mstride, int members) {
  if (int rc = check_ens_unshared(b, mstride, members)) return rc;
  return require_device();
}
// the member strides of a launch's four blocks and its checkpoint plane (NULL: all members share the block's fields)
EnsStrides ens_strides(const long long* in, const long long* out, const long long* in2, const long long* out2, long long ckpt) {
  EnsStrides ms;
  for (int i = 0; i < kNumIn; ++i) { ms.in[i] = in ? in[i] : 0; ms.in2[i] = in2 ? in2[i] : 0; }
  for (int i = 0; i < kNumOut; ++i) { ms.out[i] = out ? out[i] : 0; ms.out2[i] = out2 ? out2[i] : 0; }
  ms.ckpt = ckpt;
  return ms;
}

// ---------------------------------------------------------------------------------------------------------
// batched TL / reverse sweeps: nbatch directions over one trajectory, in chunks of at most kBatchMax per launch
// ---------------------------------------------------------------------------------------------------------
bool same_strides(const Strides& a, const Strides& b) {
  return a.full == b.full && a.half == b.half && a.cml == b.cml && a.clv == b.clv && a.loc == b.loc;
}

// Balanced chunks in stream order (5 -> 3 + 2, 9 -> 3 + 3 + 3): `launch(first, count)` once per chunk, until one fails.  A larger
// chunk next to a small rest would leave the rest's launch with the worse ratio of trajectory to direction traffic.
template <class Launch>
int for_each_chunk(int nbatch, Launch launch) {
  const int nchunks = (nbatch + kBatchMax - 1) / kBatchMax, base = nbatch / nchunks, extra = nbatch % nchunks;
  for (int ch = 0, first = 0; ch < nchunks; ++ch) {
    const int count = base + (ch < extra ? 1 : 0);
    if (int rc = launch(first, count)) return rc;
    first += count;
  }
  return 0;
}

// Whether the batched kernels' launches of a few partial rounds are paced like their single-direction twins': measured once at
// 160 000 columns (profiles/EXPERIMENTS.md, "Batched tangents and cotangents")
constexpr bool kPaceBatch = true;

// ---------------------------------------------------------------------------------------------------------
// state expansion / validation launchers
// ---------------------------------------------------------------------------------------------------------
int check_expand_args(const cloudsc2_real* table, int klon, int period, long long start, int nlevx, int ndim, int nproma,
                      long long ngptot, cloudsc2_field field, long long* nblocks) {
  if (!device_ok()) return no_device();
  if (!table || !field.ptr) return fail(CLOUDSC2_EINVAL, "NULL argument");
  if (klon < 1 || period < 1 || period > klon || start < 0 || nlevx < 1 || ndim < 1 || nproma < 1 || ngptot < 1)
    return fail(CLOUDSC2_EINVAL, "expand/validate: need 1 <= period <= KLON, start >= 0, positive dimensions");
  *nblocks = (ngptot + nproma - 1) / nproma;
  if (field.block_stride < (long long)nproma * nlevx * ndim)
    return fail(CLOUDSC2_EINVAL, "expand/validate: block stride smaller than NPROMA*NLEV*NDIM");
  return 0;
}

int ten_ptrs(const cloudsc2_outputs* o, int nlev, TenPtrs& t) {
  const cloudsc2_field* f = fields_of(*o);  // (the order of the ERROR_NORM calls, cloudsc_driver_tl_mod.F90:233-242)
  for (int i = 0; i < kNumOut; ++i) {
    if (!f[i].ptr) return fail(CLOUDSC2_EINVAL, "taylor sums: NULL field");
    t.p[i] = f[i].ptr; t.stride[i] = f[i].block_stride; t.nlevx[i] = nlev + (kOutGroup[i] == kHalf ? 1 : 0);
  }
  return 0;
}

}  // namespace

// ncols_minmax < 0: the field's own whole blocks
int validate_launch_impl(const cloudsc2_real* table, int klon, int period, long long start, int nlevx, int ndim, int nproma,
                         long long ngptot, cloudsc2_field field, double* workspace, double* stats, void* stream,
                         long long ncols_minmax) {
  long long nblocks;
  int rc = check_expand_args(table, klon, period, start, nlevx, ndim, nproma, ngptot, field, &nblocks);
  if (rc) return rc;
  if (!workspace || !stats) return fail(CLOUDSC2_EINVAL, "NULL argument");
  const long long total = nblocks * nproma * nlevx * ndim;
  const int nparts = (int)std::min<long long>((total + 255) / 256, 2048);
  hipLaunchKernelGGL(validate_partial_kernel, dim3(nparts), dim3(256), 0, (hipStream_t)stream, table, klon, period, start,
                     nlevx, ndim, nproma, ngptot, nblocks, (const real_t*)field.ptr, field.block_stride, workspace,
                     ncols_minmax < 0 ? nblocks * nproma : ncols_minmax);
  hipLaunchKernelGGL(validate_final_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)workspace, nparts, stats,
                     (int)(ncols_minmax > nblocks * nproma));
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace cloudsc2

// =========================================================================================================
// C ABI
// =========================================================================================================
extern "C" {

const char* cloudsc2_last_error(void) { return g_err.c_str(); }

int cloudsc2_device_available(void) { return device_ok() ? 1 : 0; }
int cloudsc2_current_device(void) {
  int dev = 0;
  if (!device_ok() || hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return 0; }
  return dev;
}
int cloudsc2_real_bytes(void) { return (int)sizeof(cloudsc2_real); }

#ifdef C2_WAVE_TIMES
// diagnostic build only: host_buf == NULL: (re)allocate the log for `nwaves` waves and arm it; else: copy it back (4 x u64 per wave)
int cloudsc2_debug_wave_log(unsigned long long* host_buf, long long nwaves) {
  static unsigned long long* dev = nullptr;
  static long long cap = 0;
  if (!host_buf) {
    if (dev) (void)hipFree(dev);
    HIP_TRY(hipMalloc((void**)&dev, (size_t)nwaves * 32));
    HIP_TRY(hipMemset(dev, 0, (size_t)nwaves * 32));
    cap = nwaves;
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_wave_log), &dev, sizeof(dev)));
    return 0;
  }
  if (!dev || nwaves > cap) return fail(CLOUDSC2_EINVAL, "wave log not armed");
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(host_buf, dev, (size_t)nwaves * 32, hipMemcpyDeviceToHost));
  return 0;
}
#endif

void cloudsc2_debug_launch_log_reset(void) { g_launch_log.count = 0; }
int cloudsc2_debug_launch_log(int* families, unsigned* flags, int max) {
  if (max < 0 || (max > 0 && (!families || !flags))) return fail(CLOUDSC2_EINVAL, "cloudsc2_debug_launch_log: max >= 0 and, with max > 0, both arrays required");
  const LaunchLog& l = g_launch_log;
  for (int i = 0; i < max && i < kLaunchLogMax && i < l.count; ++i) { families[i] = l.family[i]; flags[i] = l.word[i]; }
  return (int)l.count;
}

void cloudsc2_set_math_mode(int precise) { g_precise.store(precise ? 1 : 0); }
int cloudsc2_get_math_mode(void) { return g_precise.load(); }

int cloudsc2_satur_launch(const cloudsc2_params* prm, int nproma, int nlev, int ngptot, cloudsc2_field pap,
                          cloudsc2_field t, cloudsc2_field qsat, void* stream) {
  Geom g;
  int rc = check_geom(prm, nproma, nlev, ngptot, g);
  if (rc) return rc;
  if (!pap.ptr || !t.ptr || !qsat.ptr) return fail(CLOUDSC2_EINVAL, "NULL field");
  if (pap.block_stride != t.block_stride || pap.block_stride != qsat.block_stride)
    return fail(CLOUDSC2_EINVAL, "pap, t, qsat must share one block stride");
  SaturArgs args;
  args.c = make_consts(*prm, 1.0);
  args.g = g;
  args.s = Strides{pap.block_stride, 0, 0, 0, 0};
  args.pap = pap.ptr; args.t = t.ptr; args.qsat = qsat.ptr;
  hipLaunchKernelGGL(precise_of(prm) ? satur_kernel<true> : satur_kernel<false>, dim3(grid_for(g.ncols_pad, kBlock)), dim3(kBlock), 0,
                     (hipStream_t)stream, args);
  HIP_TRY(hipGetLastError());
  return 0;
}

int cloudsc2_satur_lin_launch(const cloudsc2_params* prm, int nproma, int nlev, int ngptot, cloudsc2_field pap, cloudsc2_field t,
                              cloudsc2_field qsat, cloudsc2_field dqs_dpap, cloudsc2_field dqs_dt, void* stream) {
  Geom g;
  int rc = check_geom(prm, nproma, nlev, ngptot, g);
  if (rc) return rc;
  if (!pap.ptr || !t.ptr || !dqs_dpap.ptr || !dqs_dt.ptr) return fail(CLOUDSC2_EINVAL, "NULL field");
  if (pap.block_stride != t.block_stride || pap.block_stride != dqs_dpap.block_stride || pap.block_stride != dqs_dt.block_stride ||
      (qsat.ptr && pap.block_stride != qsat.block_stride))
    return fail(CLOUDSC2_EINVAL, "pap, t, qsat, dqs_dpap, dqs_dt must share one block stride");
  SaturLinArgs args;
  args.c = make_consts(*prm, 1.0);
  args.g = g;
  args.s = Strides{pap.block_stride, 0, 0, 0, 0};
  args.pap = pap.ptr; args.t = t.ptr; args.qsat = qsat.ptr; args.dqs_dpap = dqs_dpap.ptr; args.dqs_dt = dqs_dt.ptr;
  hipLaunchKernelGGL(precise_of(prm) ? satur_lin_kernel<true> : satur_lin_kernel<false>, dim3(grid_for(g.ncols_pad, kBlock)), dim3(kBlock), 0,
                     (hipStream_t)stream, args);
  HIP_TRY(hipGetLastError());
  return 0;
}

int cloudsc2_nl_launch(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot,
                       const cloudsc2_inputs* in, const cloudsc2_outputs* out, cloudsc2_field zero_plane,
                       double pert_lambda, void* stream) {
  Sweep w;
  int rc;
  if ((rc = w.begin(prm, nproma, nlev, ngptot, (!in || !out) ? "NULL argument block" : nullptr)) || (rc = w.trajectory(*in, *out, true)) ||
      (rc = w.finish(*prm, ptsphy, in->qsat.ptr, {(long long)zero_plane.block_stride})))
    return rc;
  if (pert_lambda != 0.0) w.f |= C2F_PERT;
  if (!prm->lphylin && !prm->ldrain1d) w.f |= C2F_NOLIN;  // cloudsc2.F90:349 (CLOUDSC2TL / CLOUDSC2AD have the LPHYLIN form only)
  if ((w.f & C2F_NOLIN) && (w.f & C2F_PERT))
    return fail(CLOUDSC2_EINVAL, "pert_lambda != 0 with LPHYLIN = 0: the perturbed runs of the Taylor test exist in the LPHYLIN form only");
  NlArgs args = w.nl();
  args.zero_plane = zero_plane.ptr; args.zero_stride = zero_plane.block_stride; args.lam = pert_lambda;
  schedule(args.g, (const void*)nl_variant(w.f), true, nullptr);
  return launch_variant(kFamNl, w.f, nl_variant(w.f), args, w.g.ncols_pad, (hipStream_t)stream);
}

int cloudsc2_tl_launch(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot,
                       const cloudsc2_inputs* traj_in, const cloudsc2_outputs* traj_out,
                       const cloudsc2_inputs* pert_in, const cloudsc2_outputs* pert_out, void* stream) {
  if (!pert_in) return fail(CLOUDSC2_EINVAL, "NULL argument block");
  TlMode m; m.pert_in = pert_in;
  return tl_launch_impl(prm, ptsphy, nproma, nlev, ngptot, traj_in, traj_out, pert_out, stream, m);
}

int cloudsc2_tl_launch_self(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot,
                            const cloudsc2_inputs* traj_in, const cloudsc2_outputs* traj_out, double supsat_increment,
                            const cloudsc2_outputs* pert_out, double* yy, void* stream) {
  TlMode m; m.supsat_inc = supsat_increment; m.yy = yy;
  return tl_launch_impl(prm, ptsphy, nproma, nlev, ngptot, traj_in, traj_out, pert_out, stream, m);
}

int cloudsc2_ad_launch(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot,
                       const cloudsc2_inputs* traj_in, const cloudsc2_outputs* traj_out,
                       const cloudsc2_inputs* adj_in, const cloudsc2_outputs* adj_out, cloudsc2_real* scratch,
                       void* stream) {
  return ad_launch_impl(prm, ptsphy, nproma, nlev, ngptot, traj_in, traj_out, adj_in, adj_out, scratch, stream, AdMode{0, false, false});
}

int cloudsc2_ad_launch_assign(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot,
                              const cloudsc2_inputs* traj_in, const cloudsc2_outputs* traj_out,
                              const cloudsc2_inputs* adj_in, const cloudsc2_outputs* adj_out, cloudsc2_real* scratch,
                              void* stream) {
  return ad_launch_impl(prm, ptsphy, nproma, nlev, ngptot, traj_in, traj_out, adj_in, adj_out, scratch, stream, AdMode{0, true, false});
}

int cloudsc2_ad_launch_forward(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot,
                               const cloudsc2_inputs* traj_in, const cloudsc2_outputs* traj_out, cloudsc2_real* scratch,
                               void* stream) {
  return ad_launch_impl(prm, ptsphy, nproma, nlev, ngptot, traj_in, traj_out, nullptr, nullptr, scratch, stream, AdMode{1, false, false});
}

int cloudsc2_ad_launch_reverse(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot,
                               const cloudsc2_inputs* traj_in, const cloudsc2_outputs* traj_out,
                               const cloudsc2_inputs* adj_in, const cloudsc2_outputs* adj_out, const cloudsc2_real* scratch,
                               int assign, void* stream) {
  return ad_launch_impl(prm, ptsphy, nproma, nlev, ngptot, traj_in, traj_out, adj_in, adj_out, const_cast<cloudsc2_real*>(scratch),
                        stream, AdMode{2, assign != 0, false});
}

int cloudsc2_vjp_launch(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot,
                        const cloudsc2_inputs* traj_in, const cloudsc2_outputs* traj_out,
                        const cloudsc2_inputs* adj_in, const cloudsc2_outputs* adj_out,
                        const cloudsc2_real* scratch, void* stream) {
  return ad_launch_impl(prm, ptsphy, nproma, nlev, ngptot, traj_in, traj_out, adj_in, adj_out, const_cast<cloudsc2_real*>(scratch),
                        stream, AdMode{2, true, true});
}

int cloudsc2_tl_launch_satur(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot,
                             const cloudsc2_inputs* traj_in, const cloudsc2_inputs* pert_in, const cloudsc2_outputs* pert_out,
                             void* stream) {
  if (!pert_in) return fail(CLOUDSC2_EINVAL, "NULL argument block");
  const cloudsc2_outputs none = {};
  TlMode m; m.pert_in = pert_in; m.satlin = true;
  return tl_launch_impl(prm, ptsphy, nproma, nlev, ngptot, traj_in, &none, pert_out, stream, m);
}

int cloudsc2_vjp_launch_satur(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot,
                              const cloudsc2_inputs* traj_in, const cloudsc2_outputs* traj_out,
                              const cloudsc2_inputs* adj_in, const cloudsc2_outputs* adj_out,
                              const cloudsc2_real* scratch, void* stream) {
  return ad_launch_impl(prm, ptsphy, nproma, nlev, ngptot, traj_in, traj_out, adj_in, adj_out, const_cast<cloudsc2_real*>(scratch),
                        stream, AdMode{2, true, true, nullptr, nullptr, true});
}

// ---- sparse TL and reverse sweeps: only the planes given are moved (C2F_SPARSE) -------------------------------------------------------
// Two kernel nodes of their own, launched directly like parnormal_kernel: no family number, no launch-log entry.  Scheduling is the
// twins' (cloudsc2_tl_launch / _satur without trajectory stores, cloudsc2_vjp_launch / _satur).
// (what is wrong with the call itself is reported before the device is looked for: CLOUDSC2_EINVAL with or without one)
static int check_sparse(const cloudsc2_params* prm, int satur, const cloudsc2_inputs* traj_in, const cloudsc2_inputs* other_in) {
  if (int rc = check_satur(satur)) return rc;
  if (!prm->lphylin) return fail(CLOUDSC2_EINVAL, "sparse sweep: CLOUDSC2TL / CLOUDSC2AD linearise the LPHYLIN form only (prm->lphylin = 0)");
  if (satur && (traj_in->qsat.ptr || other_in->qsat.ptr))
    return fail(CLOUDSC2_EINVAL, "satur = 1: SATUR is differentiated in the sweep, every qsat field must be NULL");
  return require_qsat(satur, traj_in);
}

int cloudsc2_tl_launch_sparse(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, int satur,
                              const cloudsc2_inputs* traj_in, const cloudsc2_inputs* pert_in, const cloudsc2_outputs* pert_out,
                              void* stream) {
  if (!prm || !traj_in || !pert_in || !pert_out) return fail(CLOUDSC2_EINVAL, "NULL argument block");
  int rc = check_sparse(prm, satur, traj_in, pert_in);
  if (rc) return rc;
  Sweep w;
  if ((rc = resolve_in(*traj_in, false, w.s, w.in))) return rc;
  memset(&w.out, 0, sizeof(w.out));
  if (!outputs_given(*pert_out)) return fail(CLOUDSC2_EINVAL, "sparse TL sweep: no output tangent is wanted (every pert_out field is NULL)");
  TlSparseArgs sargs;
  TlArgs& args = sargs.a;
  if ((rc = resolve_sparse(*pert_in, *pert_out, 'o', args.sp, args.din, args.dout, sargs.m.rd, sargs.m.wr))) return rc;
  if ((rc = w.begin(prm, nproma, nlev, ngptot, nullptr))) return rc;
  const Strides& sp = args.sp;
  if ((rc = w.finish(*prm, ptsphy, !satur, {sp.full, sp.half, sp.cml, sp.clv, sp.loc}))) return rc;
  if (satur) w.f |= C2F_SATLIN;
  args.c = w.c; args.g = w.g; args.s = w.s; args.in = w.in; args.out = w.out; args.tab = w.tab;
  args.supsat_inc = 0; args.yy = nullptr;
  const KernelFn<TlSparseArgs> fn = tl_sparse_variant(w.f);
  schedule_tl(args.g, w.f, (const void*)fn);
  return launch_kernel(fn, sargs, grid_for(w.g.ncols_pad, kBlock), (hipStream_t)stream);
}

int cloudsc2_vjp_launch_sparse(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, int satur,
                               const cloudsc2_inputs* traj_in, const cloudsc2_outputs* traj_out, const cloudsc2_inputs* adj_in,
                               const cloudsc2_outputs* adj_out, const cloudsc2_real* scratch, void* stream) {
  if (!prm || !traj_in || !traj_out || !adj_in || !adj_out) return fail(CLOUDSC2_EINVAL, "NULL argument block");
  int rc = check_sparse(prm, satur, traj_in, adj_in);
  if (rc) return rc;
  Sweep w;
  if ((rc = w.trajectory(*traj_in, *traj_out, false))) return rc;
  if (!w.out.fplsl || !w.out.fplsn) return fail(CLOUDSC2_EINVAL, "reverse sweep: traj_out->fplsl and ->fplsn (PFPLSL5, PFPLSN5) are required");
  if ((prm->levapls2 || prm->ldrain1d) && !scratch) return fail(CLOUDSC2_EINVAL, "LEVAPLS2/LDRAIN1D: the cover-checkpoint plane `scratch` is required");
  AdSparseArgs sargs;
  memset(&sargs, 0, sizeof(sargs));
  AdArgs& args = sargs.a;
  InPtrs ain_c;
  if ((rc = resolve_sparse(*adj_in, *adj_out, 'i', args.sa, ain_c, args.aout, sargs.m.wr, sargs.m.rd))) return rc;
  if (!sargs.m.rd) return fail(CLOUDSC2_EINVAL, "sparse reverse sweep: no cotangent is given (every adj_out field is NULL)");
  if (!sargs.m.wr) return fail(CLOUDSC2_EINVAL, "sparse reverse sweep: no gradient is wanted (every adj_in field is NULL)");
  args.ain = writable(*adj_in);
  if ((rc = w.begin(prm, nproma, nlev, ngptot, nullptr))) return rc;
  const Strides& sa = args.sa;
  if ((rc = w.finish(*prm, ptsphy, !satur, {sa.full, sa.half, sa.cml, sa.clv, sa.loc, (long long)nproma * nlev /* scratch */}))) return rc;
  if (satur) w.f |= C2F_SATLIN;
  args.nl = w.nl();
  args.nl.ckpt = const_cast<cloudsc2_real*>(scratch);
  const KernelFn<AdSparseArgs> fn = vjp_sparse_variant(w.f);
  schedule(args.nl.g, nullptr, false, (const void*)fn);
  return launch_kernel(fn, sargs, grid_for(w.g.ncols_pad, kBlock), (hipStream_t)stream);
}

// ---- column sums formed in the sweeps (C2F_COLSUM) -------------------------------------------------------------------------------------
// Three kernel nodes of their own, launched directly like the sparse ones: no family number, no launch-log entry.  Scheduling is the
// twins': cloudsc2_nl_launch's (the keep form with the evaporation branch: the trajectory pass's), the sparse launchers'.
// (what is wrong with the call itself is reported before the device is looked for: CLOUDSC2_EINVAL with or without one)
// (every refusal of the three names its launcher: the entry points run their implementation through `named`)
static int named(const char* who, int rc) {
  if (rc != CLOUDSC2_EINVAL) return rc;
  const std::string msg = std::string(who) + ": " + g_err;
  return fail(rc, msg.c_str());
}
static int check_colsum_geom(const cloudsc2_params* prm, int nproma, int nlev, int ngptot) {
  if (nproma < 1 || nlev < 2 || ngptot < 1 || nlev > CLOUDSC2_MAX_NLEV || prm->nlev != nlev || prm->math_mode < 0 || prm->math_mode > 2)
    return fail(CLOUDSC2_EINVAL, "nproma >= 1, 2 <= nlev = params.nlev <= CLOUDSC2_MAX_NLEV, ngptot >= 1, params.math_mode in 0..2 required");
  return 0;
}
// the table and the block of sums: cs.w, cs.y, cs.stride; mask: the sums present
static int resolve_colsum(const cloudsc2_real* weights, const cloudsc2_outputs* sums, int nproma, const char* none, ColsumTab& cs,
                          unsigned& mask) {
  auto refuse = [&](const char* what) { return fail(CLOUDSC2_EINVAL, what); };
  if (!weights) return refuse("the weight table is NULL");
  const cloudsc2_field* f = fields_of(*sums);
  mask = 0u;
  long long stride = 0;
  for (int k = 0; k < kNumOut; ++k) {
    reinterpret_cast<real_t**>(&cs.y)[k] = f[k].ptr;
    if (!f[k].ptr) continue;
    if (mask && f[k].block_stride != stride) return refuse("the sums given must share one block stride");
    stride = f[k].block_stride;
    mask |= 1u << k;
  }
  if (!mask) return refuse(none);
  if (stride < nproma) return refuse("the block stride of the sums is below nproma");
  cs.w = weights; cs.stride = stride; cs.mask = mask;
  return 0;
}

static int nl_colsum_impl(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, const cloudsc2_inputs* in,
                          const cloudsc2_real* weights, const cloudsc2_outputs* sums, const cloudsc2_outputs* keep,
                          cloudsc2_real* scratch, void* stream, const EnsSpec* ens = nullptr) {
  if (!prm || !in || !sums) return fail(CLOUDSC2_EINVAL, "NULL argument block");
  int rc = check_colsum_geom(prm, nproma, nlev, ngptot);
  if (rc) return rc;
  if (!prm->lphylin) return fail(CLOUDSC2_EINVAL, "the LPHYLIN form only (prm->lphylin = 0)");
  NlColsumArgs cargs;
  memset(&cargs, 0, sizeof(cargs));
  unsigned mask;
  if ((rc = resolve_colsum(weights, sums, nproma, "no sum is given (every sums field is NULL)", cargs.cs, mask))) return rc;
  Sweep w;
  if ((rc = resolve_in(*in, false, w.s, w.in))) return rc;
  memset(&w.out, 0, sizeof(w.out));
  if (keep) {
    if (!keep->fplsl.ptr != !keep->fplsn.ptr) return fail(CLOUDSC2_EINVAL, "keep needs both planes, fplsl and fplsn");
    if (!keep->fplsl.ptr) return fail(CLOUDSC2_EINVAL, "keep needs both planes, fplsl and fplsn (neither is given)");
    if (keep->fplsl.block_stride != w.s.half || keep->fplsn.block_stride != w.s.half)
      return fail(CLOUDSC2_EINVAL, "the kept flux planes must have the block stride of in->paph");
    if (keep->fplsl.ptr == keep->fplsn.ptr) return fail(CLOUDSC2_EINVAL, "keep->fplsl and keep->fplsn are one plane");
    if ((prm->levapls2 || prm->ldrain1d) && !scratch)
      return fail(CLOUDSC2_EINVAL, "keep with LEVAPLS2/LDRAIN1D: the cover-checkpoint plane `scratch` is required");
    w.out.fplsl = keep->fplsl.ptr; w.out.fplsn = keep->fplsn.ptr;
  }
  if ((rc = w.begin(prm, nproma, nlev, ngptot, nullptr))) return rc;
  if ((rc = w.finish(*prm, ptsphy, in->qsat.ptr, {cargs.cs.stride, keep ? (long long)nproma * nlev : 0LL}))) return rc;
  if (keep) w.f |= C2F_CKPT;
  cargs.a = w.nl();
  cargs.a.ckpt = (keep && w.c.evap) ? scratch : nullptr;
  if (ens) return ens_launch(nl_ens_colsum_variant(w.f), cargs, ptsphy, *ens, (hipStream_t)stream);  // (neither paced nor kept abreast)
  const KernelFn<NlColsumArgs> fn = nl_colsum_variant(w.f);
  schedule(cargs.a.g, (const void*)fn, !keep, nullptr);
  return launch_kernel(fn, cargs, grid_for(w.g.ncols_pad, kBlock), (hipStream_t)stream);
}

static int tl_colsum_impl(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, int satur,
                          const cloudsc2_inputs* traj_in, const cloudsc2_inputs* pert_in, const cloudsc2_real* weights,
                          const cloudsc2_outputs* pert_sums, void* stream, const EnsSpec* ens = nullptr) {
  if (!prm || !traj_in || !pert_in || !pert_sums) return fail(CLOUDSC2_EINVAL, "NULL argument block");
  int rc = check_colsum_geom(prm, nproma, nlev, ngptot);
  if (rc) return rc;
  if ((rc = check_sparse(prm, satur, traj_in, pert_in))) return rc;
  TlColsumArgs cargs;
  memset(&cargs, 0, sizeof(cargs));
  TlSparseArgs& sargs = cargs.a;
  TlArgs& args = sargs.a;
  if ((rc = resolve_colsum(weights, pert_sums, nproma, "no sum is wanted (every pert_sums field is NULL)", cargs.cs, sargs.m.wr))) return rc;
  Sweep w;
  if ((rc = resolve_in(*traj_in, false, w.s, w.in))) return rc;
  memset(&w.out, 0, sizeof(w.out));
  const cloudsc2_outputs none = {};
  unsigned none_mask;
  if ((rc = resolve_sparse(*pert_in, none, 'o', args.sp, args.din, args.dout, sargs.m.rd, none_mask))) return rc;
  if ((rc = w.begin(prm, nproma, nlev, ngptot, nullptr))) return rc;
  const Strides& sp = args.sp;
  if ((rc = w.finish(*prm, ptsphy, !satur, {sp.full, sp.half, sp.cml, sp.clv, sp.loc, cargs.cs.stride}))) return rc;
  if (satur) w.f |= C2F_SATLIN;
  args.c = w.c; args.g = w.g; args.s = w.s; args.in = w.in; args.out = w.out; args.tab = w.tab;
  args.supsat_inc = 0; args.yy = nullptr;
  if (ens) {  // the members' blocks: the parameter derivative behind the column-sum block (the template's tangents: every member's row replaces them)
    TlEnsColsumArgs eargs;
    eargs.a = cargs;
    eargs.par = make_parlin(w.c, nullptr);
    return ens_launch(tl_ens_colsum_variant(w.f), eargs, ptsphy, *ens, (hipStream_t)stream);
  }
  const KernelFn<TlColsumArgs> fn = tl_colsum_variant(w.f);
  schedule_tl(args.g, w.f, (const void*)fn);
  return launch_kernel(fn, cargs, grid_for(w.g.ncols_pad, kBlock), (hipStream_t)stream);
}

static int vjp_colsum_impl(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, int satur,
                           const cloudsc2_inputs* traj_in, const cloudsc2_outputs* traj_out, const cloudsc2_inputs* adj_in,
                           const cloudsc2_real* weights, const cloudsc2_outputs* adj_sums, const cloudsc2_real* scratch,
                           void* stream, const EnsSpec* ens = nullptr) {
  if (!prm || !traj_in || !traj_out || !adj_in || !adj_sums) return fail(CLOUDSC2_EINVAL, "NULL argument block");
  int rc = check_colsum_geom(prm, nproma, nlev, ngptot);
  if (rc) return rc;
  if ((rc = check_sparse(prm, satur, traj_in, adj_in))) return rc;
  AdColsumArgs cargs;
  memset(&cargs, 0, sizeof(cargs));
  AdSparseArgs& sargs = cargs.a;
  AdArgs& args = sargs.a;
  if ((rc = resolve_colsum(weights, adj_sums, nproma, "no cotangent is given (every adj_sums field is NULL)", cargs.cs, sargs.m.rd))) return rc;
  Sweep w;
  if ((rc = w.trajectory(*traj_in, *traj_out, false))) return rc;
  if (!w.out.fplsl || !w.out.fplsn)
    return fail(CLOUDSC2_EINVAL, "traj_out->fplsl and ->fplsn (PFPLSL5, PFPLSN5) are required");
  if ((prm->levapls2 || prm->ldrain1d) && !scratch)
    return fail(CLOUDSC2_EINVAL, "LEVAPLS2/LDRAIN1D: the cover-checkpoint plane `scratch` is required");
  const cloudsc2_outputs none = {};
  InPtrs ain_c;
  unsigned none_mask;
  if ((rc = resolve_sparse(*adj_in, none, 'i', args.sa, ain_c, args.aout, sargs.m.wr, none_mask))) return rc;
  // (an ensemble's launch always has the parameter adjoints to form: its write mask may be empty)
  if (!sargs.m.wr && !ens) return fail(CLOUDSC2_EINVAL, "no gradient is wanted (every adj_in field is NULL)");
  args.ain = writable(*adj_in);
  if ((rc = w.begin(prm, nproma, nlev, ngptot, nullptr))) return rc;
  const Strides& sa = args.sa;
  if ((rc = w.finish(*prm, ptsphy, !satur, {sa.full, sa.half, sa.cml, sa.clv, sa.loc, (long long)nproma * nlev /* scratch */, cargs.cs.stride})))
    return rc;
  if (satur) w.f |= C2F_SATLIN;
  args.nl = w.nl();
  args.nl.ckpt = const_cast<cloudsc2_real*>(scratch);
  if (ens) {  // the members' blocks, one (PAR_COUNT, ncols_pad) slab of sums each behind them in the workspace, then the fold per member
    AdEnsColsumArgs eargs;
    eargs.a = cargs;
    eargs.par = make_parlin(w.c, nullptr);
    eargs.work = (double*)((char*)ens->workspace + ens_blocks_bytes(ens->members));
    if ((rc = ens_launch(vjp_ens_colsum_variant(w.f), eargs, ptsphy, *ens, (hipStream_t)stream))) return rc;
    if (kEnsColsumFieldsPass && sargs.m.wr) {  // fp32: the field gradients once more, in the column-sum twin's bits, over the same blocks
      VjpEnsColsumKArgs ka;
      ka.blocks = (const AdEnsColsumArgs*)ens->workspace; ka.wgs_per_member = grid_for(w.g.ncols_pad, kBlock);
      if ((rc = launch_kernel(vjp_ens_colsum_fields_variant(w.f), ka, ka.wgs_per_member * (unsigned)ens->members, (hipStream_t)stream))) return rc;
    }
    hipLaunchKernelGGL(par_fold_ens_kernel, dim3(PAR_COUNT, (unsigned)ens->members), dim3(kParFoldBlock), 0, (hipStream_t)stream,
                       (const double*)eargs.work, w.g.ncols_pad, (long long)w.g.ngptot, ens->par_adj);
    HIP_TRY(hipGetLastError());
    return 0;
  }
  const KernelFn<AdColsumArgs> fn = vjp_colsum_variant(w.f);
  schedule(args.nl.g, nullptr, false, (const void*)fn);
  return launch_kernel(fn, cargs, grid_for(w.g.ncols_pad, kBlock), (hipStream_t)stream);
}

int cloudsc2_nl_launch_colsum(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, const cloudsc2_inputs* in,
                              const cloudsc2_real* weights, const cloudsc2_outputs* sums, const cloudsc2_outputs* keep,
                              cloudsc2_real* scratch, void* stream) {
  return named("cloudsc2_nl_launch_colsum", nl_colsum_impl(prm, ptsphy, nproma, nlev, ngptot, in, weights, sums, keep, scratch, stream));
}
int cloudsc2_tl_launch_colsum(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, int satur,
                              const cloudsc2_inputs* traj_in, const cloudsc2_inputs* pert_in, const cloudsc2_real* weights,
                              const cloudsc2_outputs* pert_sums, void* stream) {
  return named("cloudsc2_tl_launch_colsum", tl_colsum_impl(prm, ptsphy, nproma, nlev, ngptot, satur, traj_in, pert_in, weights, pert_sums, stream));
}
int cloudsc2_vjp_launch_colsum(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, int satur,
                               const cloudsc2_inputs* traj_in, const cloudsc2_outputs* traj_out, const cloudsc2_inputs* adj_in,
                               const cloudsc2_real* weights, const cloudsc2_outputs* adj_sums, const cloudsc2_real* scratch,
                               void* stream) {
  return named("cloudsc2_vjp_launch_colsum", vjp_colsum_impl(prm, ptsphy, nproma, nlev, ngptot, satur, traj_in, traj_out, adj_in, weights, adj_sums, scratch, stream));
}

static_assert(CLOUDSC2_NPAR == PAR_COUNT, "the header's parameter count is the level functions'");

int cloudsc2_par_work_doubles(int nproma, int ngptot, long long* n) { return work_doubles(PAR_COUNT, nproma, ngptot, n); }
int cloudsc2_parnormal_work_doubles(int nproma, int ngptot, long long* n) { return work_doubles(CLOUDSC2_NNORMAL, nproma, ngptot, n); }

int cloudsc2_tl_launch_par(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, int satur,
                           const cloudsc2_inputs* traj_in, const cloudsc2_inputs* pert_in, const double* dpar,
                           const cloudsc2_outputs* pert_out, void* stream) {
  if (int rc = check_par(prm, satur)) return rc;
  if (!pert_in || !dpar) return fail(CLOUDSC2_EINVAL, "NULL argument block");
  if (int rc = require_qsat(satur, traj_in)) return rc;
  const cloudsc2_outputs none = {};
  TlMode m; m.pert_in = pert_in; m.satlin = satur != 0; m.dpar = dpar;
  return tl_launch_impl(prm, ptsphy, nproma, nlev, ngptot, traj_in, &none, pert_out, stream, m);
}

int cloudsc2_vjp_launch_par(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, int satur,
                            const cloudsc2_inputs* traj_in, const cloudsc2_outputs* traj_out,
                            const cloudsc2_inputs* adj_in, const cloudsc2_outputs* adj_out,
                            const cloudsc2_real* scratch, double* work, double* par_adj, void* stream) {
  if (int rc = check_par(prm, satur)) return rc;
  if (!work || !par_adj) return fail(CLOUDSC2_EINVAL, "the parameter workspace and result are required");
  if (int rc = require_qsat(satur, traj_in)) return rc;
  return ad_launch_impl(prm, ptsphy, nproma, nlev, ngptot, traj_in, traj_out, adj_in, adj_out, const_cast<cloudsc2_real*>(scratch),
                        stream, AdMode{2, true, true, nullptr, nullptr, satur != 0, work, par_adj});
}

// ---- perturbed-parameter ensembles: the three launchers above for `members` members, the parameters read on the device ----------------

long long cloudsc2_ens_workspace_bytes(int members, int nproma, int nlev, int ngptot) {
  if (members < 1 || members > 65535 || nproma < 1 || nlev < 2 || nlev > CLOUDSC2_MAX_NLEV || ngptot < 1)
    return fail(CLOUDSC2_EINVAL, "1 <= members <= 65535, nproma >= 1, 2 <= nlev <= CLOUDSC2_MAX_NLEV, ngptot >= 1 required");
  return (long long)ens_blocks_bytes(members) + (long long)members * PAR_COUNT * ncols_pad(nproma, ngptot) * (long long)sizeof(double);
}

int cloudsc2_nl_launch_ens(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, int members, const double* params_dev,
                           const cloudsc2_inputs* traj_in, const long long* traj_in_mstride, const cloudsc2_outputs* traj_out,
                           const long long* traj_out_mstride, cloudsc2_real* scratch, long long scratch_mstride, void* workspace,
                           void* stream) {
  if (int rc = check_ens(prm, 0, members, params_dev, workspace)) return rc;
  if (scratch && members > 1 && scratch_mstride == 0) return fail(CLOUDSC2_EINVAL, "ensemble: the cover-checkpoint plane has member stride 0");
  if (int rc = check_ens_written(traj_out, traj_out_mstride, members)) return rc;
  EnsSpec e = {members, params_dev, nullptr, ens_strides(traj_in_mstride, traj_out_mstride, nullptr, nullptr, scratch_mstride), workspace, nullptr};
  AdMode m{1, false, false};
  m.ens = &e;
  return ad_launch_impl(prm, ptsphy, nproma, nlev, ngptot, traj_in, traj_out, nullptr, nullptr, scratch, stream, m);
}

int cloudsc2_tl_launch_ens(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, int satur, int members,
                           const double* params_dev, const double* dparams_dev, const cloudsc2_inputs* traj_in,
                           const long long* traj_in_mstride, const cloudsc2_inputs* pert_in, const long long* pert_in_mstride,
                           const cloudsc2_outputs* pert_out, const long long* pert_out_mstride, void* workspace, void* stream) {
  if (int rc = check_ens(prm, satur, members, params_dev, workspace)) return rc;
  if (int rc = check_ens_written(pert_out, pert_out_mstride, members)) return rc;
  if (!pert_in || !dparams_dev) return fail(CLOUDSC2_EINVAL, "NULL argument block");
  if (int rc = require_qsat(satur, traj_in)) return rc;
  EnsSpec e = {members, params_dev, dparams_dev, ens_strides(traj_in_mstride, nullptr, pert_in_mstride, pert_out_mstride, 0), workspace, nullptr};
  const cloudsc2_outputs none = {};
  const double no_tangent[PAR_COUNT] = {};  // (the template's; every member's come from dparams_dev)
  TlMode m; m.pert_in = pert_in; m.satlin = satur != 0; m.dpar = no_tangent; m.ens = &e;
  return tl_launch_impl(prm, ptsphy, nproma, nlev, ngptot, traj_in, &none, pert_out, stream, m);
}

int cloudsc2_vjp_launch_ens(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, int satur, int members,
                            const double* params_dev, const cloudsc2_inputs* traj_in, const long long* traj_in_mstride,
                            const cloudsc2_outputs* traj_out, const long long* traj_out_mstride, const cloudsc2_inputs* adj_in,
                            const long long* adj_in_mstride, const cloudsc2_outputs* adj_out, const long long* adj_out_mstride,
                            const cloudsc2_real* scratch, long long scratch_mstride, void* workspace, double* par_adj, void* stream) {
  if (int rc = check_ens(prm, satur, members, params_dev, workspace)) return rc;
  if (int rc = check_ens_written(adj_in, adj_in_mstride, members)) return rc;
  if (!par_adj) return fail(CLOUDSC2_EINVAL, "the parameter adjoints' array is required");
  if (int rc = require_qsat(satur, traj_in)) return rc;
  EnsSpec e = {members, params_dev, nullptr, ens_strides(traj_in_mstride, traj_out_mstride, adj_in_mstride, adj_out_mstride, scratch_mstride), workspace,
               par_adj};
  AdMode m{2, true, true, nullptr, nullptr, satur != 0, (double*)((char*)workspace + ens_blocks_bytes(members)), par_adj};
  m.ens = &e;
  return ad_launch_impl(prm, ptsphy, nproma, nlev, ngptot, traj_in, traj_out, adj_in, adj_out, const_cast<cloudsc2_real*>(scratch), stream, m);
}

// ---- column sums of an ensemble's members: the column-sum launchers for `members` members (C2F_MEMBER) ------------------------------------
// check_ens and the written-field rule first, then the column-sum parent checks the call and builds the template block; ens_launch runs it.
// The sums advance by EnsStrides::out2, the NL sweep's kept planes by ::out.
static int check_ens_colsum(const cloudsc2_params* prm, int satur, int members, const double* params_dev, const void* workspace) {
  if (!prm) return fail(CLOUDSC2_EINVAL, "NULL argument block");
  return check_ens(prm, satur, members, params_dev, workspace);
}

int cloudsc2_nl_launch_ens_colsum(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, int members,
                                  const double* params_dev, const cloudsc2_inputs* in, const long long* in_mstride,
                                  const cloudsc2_real* weights, const cloudsc2_outputs* sums, const long long* sums_mstride,
                                  const cloudsc2_outputs* keep, const long long* keep_mstride, cloudsc2_real* scratch,
                                  long long scratch_mstride, void* workspace, void* stream) {
  const char* who = "cloudsc2_nl_launch_ens_colsum";
  if (int rc = named(who, check_ens_colsum(prm, 0, members, params_dev, workspace))) return rc;
  if (keep && scratch && members > 1 && scratch_mstride == 0)
    return named(who, fail(CLOUDSC2_EINVAL, "ensemble: the cover-checkpoint plane has member stride 0"));
  if (int rc = named(who, check_ens_unshared(sums, sums_mstride, members))) return rc;
  if (int rc = named(who, check_ens_unshared(keep, keep_mstride, members))) return rc;
  EnsSpec e = {members, params_dev, nullptr, ens_strides(in_mstride, keep ? keep_mstride : nullptr, nullptr, sums_mstride, scratch_mstride),
               workspace, nullptr};
  return named(who, nl_colsum_impl(prm, ptsphy, nproma, nlev, ngptot, in, weights, sums, keep, scratch, stream, &e));
}

int cloudsc2_tl_launch_ens_colsum(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, int satur, int members,
                                  const double* params_dev, const double* dparams_dev, const cloudsc2_inputs* traj_in,
                                  const long long* traj_in_mstride, const cloudsc2_inputs* pert_in, const long long* pert_in_mstride,
                                  const cloudsc2_real* weights, const cloudsc2_outputs* pert_sums, const long long* sums_mstride,
                                  void* workspace, void* stream) {
  const char* who = "cloudsc2_tl_launch_ens_colsum";
  if (int rc = named(who, check_ens_colsum(prm, satur, members, params_dev, workspace))) return rc;
  if (int rc = named(who, check_ens_unshared(pert_sums, sums_mstride, members))) return rc;
  if (!dparams_dev) return named(who, fail(CLOUDSC2_EINVAL, "NULL argument block"));
  EnsSpec e = {members, params_dev, dparams_dev, ens_strides(traj_in_mstride, nullptr, pert_in_mstride, sums_mstride, 0), workspace, nullptr};
  return named(who, tl_colsum_impl(prm, ptsphy, nproma, nlev, ngptot, satur, traj_in, pert_in, weights, pert_sums, stream, &e));
}

int cloudsc2_vjp_launch_ens_colsum(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, int satur, int members,
                                   const double* params_dev, const cloudsc2_inputs* traj_in, const long long* traj_in_mstride,
                                   const cloudsc2_outputs* traj_out, const long long* traj_out_mstride, const cloudsc2_inputs* adj_in,
                                   const long long* adj_in_mstride, const cloudsc2_real* weights, const cloudsc2_outputs* adj_sums,
                                   const long long* sums_mstride, const cloudsc2_real* scratch, long long scratch_mstride,
                                   void* workspace, double* par_adj, void* stream) {
  const char* who = "cloudsc2_vjp_launch_ens_colsum";
  if (int rc = named(who, check_ens_colsum(prm, satur, members, params_dev, workspace))) return rc;
  if (int rc = named(who, check_ens_unshared(adj_in, adj_in_mstride, members))) return rc;
  if (!par_adj) return named(who, fail(CLOUDSC2_EINVAL, "the parameter adjoints' array is required"));
  EnsSpec e = {members, params_dev, nullptr, ens_strides(traj_in_mstride, traj_out_mstride, adj_in_mstride, sums_mstride, scratch_mstride),
               workspace, par_adj};
  return named(who, vjp_colsum_impl(prm, ptsphy, nproma, nlev, ngptot, satur, traj_in, traj_out, adj_in, weights, adj_sums, scratch, stream, &e));
}

int cloudsc2_batch_max(void) { return kBatchMax; }

int cloudsc2_tl_launch_batch(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, const cloudsc2_inputs* traj_in,
                             int nbatch, const cloudsc2_inputs* pert_in, const cloudsc2_outputs* pert_out, void* stream) {
  Sweep w;
  int rc = w.begin(prm, nproma, nlev, ngptot,
                   (!traj_in || !pert_in || !pert_out) ? "NULL argument block" : nbatch < 1 ? "nbatch >= 1 required" : nullptr);
  if (rc) return rc;
  if (nbatch == 1) {  // one direction: the single-direction sweep itself (it requires qsat of pert_in only, so ask here)
    if (!traj_in->qsat.ptr) return fail(CLOUDSC2_EINVAL, "qsat field required");
    const cloudsc2_outputs none = {};
    TlMode m; m.pert_in = pert_in;
    return tl_launch_impl(prm, ptsphy, nproma, nlev, ngptot, traj_in, &none, pert_out, stream, m);
  }
  if ((rc = resolve_in(*traj_in, true, w.s, w.in))) return rc;
  memset(&w.out, 0, sizeof(w.out));
  std::vector<InPtrs> din((size_t)nbatch);
  std::vector<OutPtrs> dout((size_t)nbatch);
  Strides sp = {0, 0, 0, 0, 0};
  for (int b = 0; b < nbatch; ++b) {
    Strides sb = {0, 0, 0, 0, 0};
    if ((rc = resolve_in(pert_in[b], true, sb, din[b])) || (rc = resolve_out(pert_out[b], true, sb, dout[b]))) return rc;
    if (b == 0) sp = sb;
    else if (!same_strides(sp, sb)) return fail(CLOUDSC2_EINVAL, "batched launch: every direction must have the same block stride per layout group");
  }
  if ((rc = w.finish(*prm, ptsphy, true, {sp.full, sp.half, sp.cml, sp.clv, sp.loc}))) return rc;
  TlBatchArgs args;
  args.c = w.c; args.g = w.g; args.s = w.s; args.sp = sp; args.in = w.in; args.tab = w.tab;
  return for_each_chunk(nbatch, [&](int first, int count) {
    const unsigned word = w.f + 64u * (unsigned)count;  // (the direction count is the kernel's compile-time one)
    const KernelFn<TlBatchArgs> fn = tl_batch_variant(word);
    for (int b = 0; b < kBatchMax; ++b) {  // (the sets from `count` on are not read: valid pointers all the same)
      args.din[b] = din[first + (b < count ? b : 0)];
      args.dout[b] = dout[first + (b < count ? b : 0)];
    }
    schedule(args.g, nullptr, false, kPaceBatch ? (const void*)fn : nullptr);
    return launch_variant(kFamTlBatch, word, fn, args, w.g.ncols_pad, (hipStream_t)stream);
  });
}

int cloudsc2_vjp_launch_batch(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, const cloudsc2_inputs* traj_in,
                              const cloudsc2_outputs* traj_out, int nbatch, const cloudsc2_inputs* adj_in, const cloudsc2_outputs* adj_out,
                              const cloudsc2_real* scratch, void* stream) {
  Sweep w;
  int rc = w.begin(prm, nproma, nlev, ngptot,
                   (!traj_in || !traj_out || !adj_in || !adj_out) ? "NULL argument block" : nbatch < 1 ? "nbatch >= 1 required" : nullptr);
  if (rc) return rc;
  if (!traj_in->qsat.ptr) return fail(CLOUDSC2_EINVAL, "qsat field required");
  if (nbatch == 1)  // one direction: the single-direction sweep itself
    return ad_launch_impl(prm, ptsphy, nproma, nlev, ngptot, traj_in, traj_out, adj_in, adj_out, const_cast<cloudsc2_real*>(scratch), stream,
                          AdMode{2, true, true});
  if ((rc = w.trajectory(*traj_in, *traj_out, false))) return rc;
  if (!w.out.fplsl || !w.out.fplsn) return fail(CLOUDSC2_EINVAL, "reverse sweep: traj_out->fplsl and ->fplsn (PFPLSL5, PFPLSN5) are required");
  std::vector<InPtrsRW> ain((size_t)nbatch);
  std::vector<OutPtrs> aout((size_t)nbatch);
  Strides sa = {0, 0, 0, 0, 0};
  for (int b = 0; b < nbatch; ++b) {
    Strides sb = {0, 0, 0, 0, 0};
    InPtrs checked;
    if ((rc = resolve_in(adj_in[b], true, sb, checked)) || (rc = resolve_out(adj_out[b], true, sb, aout[b]))) return rc;
    ain[b] = writable(adj_in[b]);
    if (b == 0) sa = sb;
    else if (!same_strides(sa, sb)) return fail(CLOUDSC2_EINVAL, "batched launch: every direction must have the same block stride per layout group");
  }
  if ((rc = w.finish(*prm, ptsphy, true, {sa.full, sa.half, sa.cml, sa.clv, sa.loc, (long long)nproma * nlev /* scratch */}))) return rc;
  if (w.c.evap && !scratch) return fail(CLOUDSC2_EINVAL, "LEVAPLS2/LDRAIN1D: the cover-checkpoint plane `scratch` is required");
  VjpBatchArgs args;
  args.nl = w.nl();
  args.nl.ckpt = const_cast<cloudsc2_real*>(scratch);
  args.sa = sa;
  return for_each_chunk(nbatch, [&](int first, int count) {
    const unsigned word = w.f + 64u * (unsigned)count;
    const KernelFn<VjpBatchArgs> fn = vjp_batch_variant(word);
    for (int b = 0; b < kBatchMax; ++b) {
      args.ain[b] = ain[first + (b < count ? b : 0)];
      args.aout[b] = aout[first + (b < count ? b : 0)];
    }
    schedule(args.nl.g, nullptr, false, kPaceBatch ? (const void*)fn : nullptr);
    return launch_variant(kFamVjpBatch, word, fn, args, w.g.ncols_pad, (hipStream_t)stream);
  });
}

// The parameter Jacobian: the sensitivities of the ten outputs to the tunable parameters in ONE sweep over the trajectory
// (tl_parjac_column: no tangent planes; direction k runs with make_parlin of the unit tangent of parameter k).  Without the evaporation
// branch the kernel runs CLOUDSC2_NPAR - 1 directions and pert_out[PAR_RPECONS] is not looked at.
int cloudsc2_tl_launch_parjac(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, const cloudsc2_inputs* traj_in,
                              const cloudsc2_outputs* pert_out, void* stream) {
  // (what is wrong with the call itself is reported before the device is looked for: CLOUDSC2_EINVAL with or without one)
  if (!prm || !traj_in || !pert_out) return fail(CLOUDSC2_EINVAL, "NULL argument block");
  if (!prm->lphylin) return fail(CLOUDSC2_EINVAL, "parameter Jacobian: CLOUDSC2TL linearises the LPHYLIN form only (prm->lphylin = 0)");
  int rc = check_rpecons(prm);
  if (rc) return rc;
  const int np = par_directions(prm);
  Sweep w;
  if ((rc = resolve_in(*traj_in, false, w.s, w.in))) return rc;
  memset(&w.out, 0, sizeof(w.out));
  TlParJacArgs args;
  Strides sp = {0, 0, 0, 0, 0};
  for (int b = 0; b < np; ++b) {
    Strides sb = {0, 0, 0, 0, 0};
    if ((rc = resolve_out(pert_out[b], true, sb, args.dout[b]))) return rc;
    if (b == 0) sp = sb;
    else if (!same_strides(sp, sb)) return fail(CLOUDSC2_EINVAL, "parameter Jacobian: every block must have the same block stride per layout group");
  }
  if ((rc = par_sweep_args(w, prm, ptsphy, nproma, nlev, ngptot, traj_in, {sp.full, sp.half, sp.loc}, args))) return rc;
  args.sp = sp;
  for (int b = np; b < kBatchMax; ++b) args.dout[b] = args.dout[0];  // (not read: valid pointers all the same)
  const KernelFn<TlParJacArgs> fn = tl_parjac_variant(w.f);
  schedule(args.g, nullptr, false, kPaceBatch ? (const void*)fn : nullptr);
  return launch_variant(kFamTlParjac, w.f, fn, args, w.g.ncols_pad, (hipStream_t)stream);
}

// The Gauss-Newton normal equations of the parameters: J^T W J and J^T W r over every active column, level and observed output, without
// J ever existing in memory (parnormal_column sums each column in registers; the fold of cloudsc2_vjp_launch_par adds the columns).
// Two kernel nodes, both launched directly: this is not a sweep family (no family number, no pacing, no launch-log entry).
static_assert(CLOUDSC2_NNORMAL == normal_sums(PAR_COUNT) && CLOUDSC2_NNORMAL <= 32, "rows of the workspace: one bit each in the fold's mask");
// the CLOUDSC2_NNORMAL rows of `work` folded over the columns into `normal` (both normal-equation launchers)
static int fold_normal(const Geom& g, bool evap, const double* work, double* normal, hipStream_t st) {
  const long long n = g.ncols_pad;
  if (evap) {
    hipLaunchKernelGGL(par_fold_kernel, dim3(CLOUDSC2_NNORMAL), dim3(kParFoldBlock), 0, st, work, n, (long long)g.ngptot, normal);
  } else {  // the rows with rpecons were not written: not read, stored as zeros
    unsigned unwritten = 1u << normal_row_g(PAR_RPECONS);
    for (int a = 0; a < PAR_COUNT; ++a) unwritten |= 1u << normal_row_h(a, PAR_RPECONS);
    hipLaunchKernelGGL(par_fold_rows_kernel, dim3(CLOUDSC2_NNORMAL), dim3(kParFoldBlock), 0, st, work, n, (long long)g.ngptot, unwritten, normal);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}
int cloudsc2_parnormal_launch(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, const cloudsc2_inputs* traj_in,
                              const cloudsc2_outputs* resid, const cloudsc2_outputs* weight, double* work, double* normal, void* stream) {
  // (what is wrong with the call itself is reported before the device is looked for: CLOUDSC2_EINVAL with or without one)
  if (!prm || !traj_in || !resid || !work || !normal) return fail(CLOUDSC2_EINVAL, "NULL argument block, workspace or result");
  if (!prm->lphylin) return fail(CLOUDSC2_EINVAL, "normal equations: CLOUDSC2TL linearises the LPHYLIN form only (prm->lphylin = 0)");
  int rc = check_rpecons(prm);
  if (rc) return rc;
  Sweep w;
  if ((rc = resolve_in(*traj_in, false, w.s, w.in))) return rc;
  memset(&w.out, 0, sizeof(w.out));
  const cloudsc2_outputs none = {};
  const cloudsc2_outputs& wt = weight ? *weight : none;
  const cloudsc2_field *rf = fields_of(*resid), *wf = fields_of(wt);
  bool weighted[kGroups] = {};
  int nobs = 0;
  for (int i = 0; i < kNumOut; ++i) {
    if (rf[i].ptr) ++nobs;
    else if (wf[i].ptr) return fail(CLOUDSC2_EINVAL, "normal equations: a weight is given for an output that is not observed (its residual is NULL)");
    if (wf[i].ptr) weighted[kOutGroup[i]] = true;
  }
  if (!nobs) return fail(CLOUDSC2_EINVAL, "normal equations: no output is observed (every residual field is NULL)");
  ParNormalArgs args;
  Strides sr = {0, 0, 0, 0, 0}, sw = {0, 0, 0, 0, 0};
  if ((rc = resolve_out(*resid, false, sr, args.resid)) || (rc = resolve_out(wt, false, sw, args.weight))) return rc;
  if ((weighted[kLoc] && sw.loc != sr.loc) || (weighted[kFull] && sw.full != sr.full) || (weighted[kHalf] && sw.half != sr.half))
    return fail(CLOUDSC2_EINVAL, "normal equations: residuals and weights must have the same block stride per layout group");
  if ((rc = par_sweep_args(w, prm, ptsphy, nproma, nlev, ngptot, traj_in, {sr.full, sr.half, sr.loc}, args))) return rc;
  const unsigned f = w.f & ~C2F_OFF32;  // (64-bit offsets always: a 32-bit form is not built)
  args.sr = sr; args.work = work;
  schedule(args.g, nullptr, false, nullptr);
  if ((rc = launch_kernel(parnormal_variant(f), args, grid_for(w.g.ncols_pad, kBlock), (hipStream_t)stream))) return rc;
  return fold_normal(w.g, w.c.evap, work, normal, (hipStream_t)stream);
}

// ---- the parameter Jacobian and the normal equations of the column sums (parcolsum_column) ------------------------------------------------
// The sensitivities of the column sums to the tunable parameters, stored (cloudsc2_parjac_launch_colsum) or contracted per column into the
// normal equations (cloudsc2_parnormal_launch_colsum: then the fold of cloudsc2_parnormal_launch).  Launched directly like parnormal_kernel:
// no family number, no pacing, no launch-log entry.  What is wrong with the call itself is reported before the device is looked for.
// the common part: `blocks` holds `nblk` blocks of (nblocks, nproma) fields, block 0 the one whose present fields are the mask; `form`:
// 0 or C2F_NORMAL
static int parcolsum_impl(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, const cloudsc2_inputs* traj_in,
                   const cloudsc2_real* wtable, ParColsumArgs& args, unsigned form, void* stream) {
  Sweep w;
  int rc;
  if ((rc = resolve_in(*traj_in, false, w.s, w.in))) return rc;
  memset(&w.out, 0, sizeof(w.out));
  if ((rc = par_sweep_args(w, prm, ptsphy, nproma, nlev, ngptot, traj_in, {args.cs.stride}, args))) return rc;
  args.cs.w = wtable;
  schedule(args.g, nullptr, false, nullptr);
  return launch_kernel(parcolsum_variant(w.f | form), args, grid_for(w.g.ncols_pad, kBlock), (hipStream_t)stream);
}
// what both launchers refuse first
static int check_parcolsum(const cloudsc2_params* prm, int nproma, int nlev, int ngptot, const cloudsc2_real* wtable) {
  int rc = check_colsum_geom(prm, nproma, nlev, ngptot);
  if (rc) return rc;
  if (!prm->lphylin) return fail(CLOUDSC2_EINVAL, "CLOUDSC2TL linearises the LPHYLIN form only (prm->lphylin = 0)");
  if ((rc = check_rpecons(prm))) return rc;
  if (!wtable) return fail(CLOUDSC2_EINVAL, "the weight table is NULL");
  return 0;
}

static int parjac_colsum_impl(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, const cloudsc2_inputs* traj_in,
                       const cloudsc2_real* wtable, const cloudsc2_outputs* sens_sums, void* stream) {
  if (!prm || !traj_in || !sens_sums) return fail(CLOUDSC2_EINVAL, "NULL argument block");
  int rc = check_parcolsum(prm, nproma, nlev, ngptot, wtable);
  if (rc) return rc;
  const int np = par_directions(prm);
  ParColsumArgs args;
  memset(&args, 0, sizeof(args));
  unsigned mask = 0u;
  if ((rc = resolve_colsum(wtable, &sens_sums[0], nproma, "no sum is wanted (every field of sens_sums[0] is NULL)", args.cs, mask))) return rc;
  args.y[0] = args.cs.y;
  for (int b = 1; b < np; ++b) {
    ColsumTab cb;
    unsigned mb = 0u;
    if ((rc = resolve_colsum(wtable, &sens_sums[b], nproma, "every parameter's block of sens_sums must hold the same sums (one holds none)", cb, mb)))
      return rc;
    if (mb != mask) return fail(CLOUDSC2_EINVAL, "every parameter's block of sens_sums must hold the same sums");
    if (cb.stride != args.cs.stride) return fail(CLOUDSC2_EINVAL, "the sums given must share one block stride");
    args.y[b] = cb.y;
  }
  for (int b = np; b < kBatchMax; ++b) args.y[b] = args.y[0];  // (not read: valid pointers all the same)
  memset(&args.cs.y, 0, sizeof(args.cs.y));
  return parcolsum_impl(prm, ptsphy, nproma, nlev, ngptot, traj_in, wtable, args, 0u, stream);
}

static int parnormal_colsum_impl(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, const cloudsc2_inputs* traj_in,
                          const cloudsc2_real* wtable, const cloudsc2_outputs* resid, const cloudsc2_outputs* weight, double* work,
                          double* normal, void* stream) {
  if (!prm || !traj_in || !resid || !work || !normal) return fail(CLOUDSC2_EINVAL, "NULL argument block, workspace or result");
  int rc = check_parcolsum(prm, nproma, nlev, ngptot, wtable);
  if (rc) return rc;
  const cloudsc2_outputs none = {};
  const cloudsc2_outputs& wt = weight ? *weight : none;
  const cloudsc2_field *rf = fields_of(*resid), *wf = fields_of(wt);
  for (int i = 0; i < kNumOut; ++i)
    if (!rf[i].ptr && wf[i].ptr) return fail(CLOUDSC2_EINVAL, "a weight is given for a sum that is not observed (its residual is NULL)");
  ParColsumArgs args;
  memset(&args, 0, sizeof(args));
  unsigned mask = 0u, wmask = 0u;
  if ((rc = resolve_colsum(wtable, resid, nproma, "no sum is observed (every residual field is NULL)", args.cs, mask))) return rc;
  args.y[0] = args.cs.y;
  if (outputs_given(wt)) {
    ColsumTab cw;
    if ((rc = resolve_colsum(wtable, &wt, nproma, "", cw, wmask))) return rc;
    if (cw.stride != args.cs.stride) return fail(CLOUDSC2_EINVAL, "residuals and weights must share one block stride");
    args.y[1] = cw.y;
  }
  memset(&args.cs.y, 0, sizeof(args.cs.y));
  args.work = work;
  if ((rc = parcolsum_impl(prm, ptsphy, nproma, nlev, ngptot, traj_in, wtable, args, C2F_NORMAL, stream))) return rc;
  return fold_normal(args.g, args.c.evap, work, normal, (hipStream_t)stream);
}

int cloudsc2_parjac_launch_colsum(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, const cloudsc2_inputs* traj_in,
                                  const cloudsc2_real* wtable, const cloudsc2_outputs* sens_sums, void* stream) {
  return named("cloudsc2_parjac_launch_colsum", parjac_colsum_impl(prm, ptsphy, nproma, nlev, ngptot, traj_in, wtable, sens_sums, stream));
}
int cloudsc2_parnormal_launch_colsum(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, const cloudsc2_inputs* traj_in,
                                     const cloudsc2_real* wtable, const cloudsc2_outputs* resid, const cloudsc2_outputs* weight, double* work,
                                     double* normal, void* stream) {
  return named("cloudsc2_parnormal_launch_colsum",
               parnormal_colsum_impl(prm, ptsphy, nproma, nlev, ngptot, traj_in, wtable, resid, weight, work, normal, stream));
}

int cloudsc2_ad_launch_reverse_norms(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot,
                                     const cloudsc2_inputs* traj_in, const cloudsc2_outputs* traj_out,
                                     const cloudsc2_inputs* adj_in, const cloudsc2_outputs* adj_out,
                                     double* norms, double* blockmax, void* stream) {
  if (!norms || !blockmax) return fail(CLOUDSC2_EINVAL, "NULL argument");
  return ad_launch_impl(prm, ptsphy, nproma, nlev, ngptot, traj_in, traj_out, adj_in, adj_out, nullptr, stream,
                        AdMode{2, true, false, norms, blockmax});
}

int cloudsc2_expand_launch(const cloudsc2_real* table, int klon, int period, long long start, int nlevx, int ndim, int nproma,
                           long long ngptot, cloudsc2_field field, void* stream) {
  long long nblocks;
  int rc = check_expand_args(table, klon, period, start, nlevx, ndim, nproma, ngptot, field, &nblocks);
  if (rc) return rc;
  const long long total = nblocks * nproma * nlevx * ndim;
  const unsigned grid = (unsigned)std::min<long long>((total + 255) / 256, 256 * 32);
  hipLaunchKernelGGL(expand_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, table, klon, period, start, nlevx, ndim,
                     nproma, ngptot, nblocks, field.ptr, field.block_stride);
  HIP_TRY(hipGetLastError());
  return 0;
}

int cloudsc2_validate_workspace_doubles(void) { return 5 * 2048; }

int cloudsc2_validate_launch(const cloudsc2_real* table, int klon, int period, long long start, int nlevx, int ndim, int nproma,
                             long long ngptot, cloudsc2_field field, double* workspace, double* stats, void* stream) {
  return validate_launch_impl(table, klon, period, start, nlevx, ndim, nproma, ngptot, field, workspace, stats, stream, -1);
}

int cloudsc2_taylor_sums_launch(int nproma, int nlev, int ngptot, const cloudsc2_outputs* f,
                                const cloudsc2_outputs* f_pert, const cloudsc2_outputs* tl, double lambda,
                                double* sums, void* stream) {
  if (!f || !f_pert || !tl || !sums) return fail(CLOUDSC2_EINVAL, "NULL argument");
  if (!device_ok()) return no_device();
  TenPtrs a, b, c;
  int rc;
  if ((rc = ten_ptrs(f, nlev, a))) return rc;
  if ((rc = ten_ptrs(f_pert, nlev, b))) return rc;
  if ((rc = ten_ptrs(tl, nlev, c))) return rc;
  int nblocks = (ngptot + nproma - 1) / nproma;
  hipLaunchKernelGGL(taylor_sums_kernel, dim3(nblocks), dim3(256), 0, (hipStream_t)stream, nproma, nlev, ngptot, a, b, c, lambda, sums);
  HIP_TRY(hipGetLastError());
  return 0;
}

int cloudsc2_taylor_sweep_work_doubles(int nproma, int ngptot, long long* n) {
  if (!n || nproma < 1 || ngptot < 1) return fail(CLOUDSC2_EINVAL, "taylor sweep: bad argument");
  *n = (long long)(10 * kTaylorLambdas + 10) * ncols_pad(nproma, ngptot);
  return 0;
}

int cloudsc2_taylor_sweep_launch(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, int nproma_stat,
                                 const cloudsc2_inputs* in, const cloudsc2_outputs* out, const cloudsc2_outputs* tl,
                                 double* work, double* sums, void* stream) {
  Sweep w;
  int rc = w.begin(prm, nproma, nlev, ngptot, (!in || !out || !tl || !work || !sums) ? "NULL argument" : nullptr);
  if (rc) return rc;
  if (nproma_stat < 1) return fail(CLOUDSC2_EINVAL, "taylor sweep: the block of the statistic must be >= 1");
  if (!prm->lphylin && !prm->ldrain1d) return fail(CLOUDSC2_EINVAL, "taylor sweep: CLOUDSC_DRIVER_TL runs with LPHYLIN (cloudsc2tl.F90 has that form only)");
  TaylorArgs args;
  if ((rc = w.trajectory(*in, *out, true))) return rc;
  if ((rc = ten_ptrs(tl, nlev, args.tl))) return rc;
  if ((rc = w.finish(*prm, ptsphy, in->qsat.ptr, {}))) return rc;
  args.nl = w.nl();
  TenLambdas lam;
  for (int il = 0; il < kTaylorLambdas; ++il) {
    lam.v[il] = pow(10.0, -(double)(il + 1));  // ZLAMBDA=10._JPRB**(-REAL(ILAM,JPRB)), cloudsc_driver_tl_mod.F90:199
    args.lam[il] = (real_t)lam.v[il];
  }
  args.colsum = work;
  const Geom& g = w.g;
  const long long nwaves = (g.ncols_pad + kTaylorCols - 1) / kTaylorCols;
  const long long per8 = 8LL * kBlock;  // the kernel's XCD mapping wants a multiple of 8 blocks
  if ((rc = launch_variant(kFamTaylor, w.f, taylor_variant(w.f), args, (nwaves * 64 + per8 - 1) / per8 * per8, (hipStream_t)stream))) return rc;
  const long long nblocks_stat = ((long long)ngptot + nproma_stat - 1) / nproma_stat;
  if (nproma_stat <= 512) {
    hipLaunchKernelGGL(taylor_reduce_kernel, dim3((unsigned)nblocks_stat), dim3(128), 0, (hipStream_t)stream, nproma_stat, ngptot,
                       g.ncols_pad, nblocks_stat, lam, (const double*)work, sums);
  } else {
    hipLaunchKernelGGL(taylor_reduce_wide_kernel, dim3((unsigned)nblocks_stat, 10 * kTaylorLambdas + 10), dim3(256), 0, (hipStream_t)stream,
                       nproma_stat, ngptot, g.ncols_pad, nblocks_stat, lam, (const double*)work, sums);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

int cloudsc2_adjoint_norms_launch(int nproma, int nlev, int ngptot, const cloudsc2_inputs* traj_in,
                                  const cloudsc2_field* qsat, const cloudsc2_outputs* y,
                                  const cloudsc2_inputs* x_adj, double* norms, double* blockmax, void* stream) {
  // y == NULL: second half only (norm2/norm3 from norm1 already in norms); x_adj == NULL: first half only.
  if (!norms) return fail(CLOUDSC2_EINVAL, "NULL argument");
  if (!device_ok()) return no_device();
  Geom g;
  g.nproma = nproma; g.nlev = nlev; g.ngptot = ngptot; g.ncols_pad = ncols_pad(nproma, ngptot); g.kb0 = g.kb1 = 0; g.fair = 0;
  dim3 grid(grid_for(g.ncols_pad, kBlock)), block(kBlock);
  int rc;
  if (y) {
    Strides sa = {0, 0, 0, 0, 0};
    OutPtrs yp;
    if ((rc = resolve_out(*y, true, sa, yp))) return rc;
    hipLaunchKernelGGL(adjoint_norm1_kernel, grid, block, 0, (hipStream_t)stream, g, sa, yp, norms);
    HIP_TRY(hipGetLastError());
  }
  if (x_adj) {
    if (!traj_in || !qsat || !qsat->ptr || !blockmax) return fail(CLOUDSC2_EINVAL, "NULL argument");
    Strides s = {0, 0, 0, 0, 0}, sa = {0, 0, 0, 0, 0};
    InPtrs ip, xp;
    if ((rc = resolve_in(*traj_in, false, s, ip))) return rc;
    if ((rc = resolve_in(*x_adj, true, sa, xp))) return rc;
    hipLaunchKernelGGL(adjoint_norm2_kernel, grid, block, 0, (hipStream_t)stream, g, s, sa, ip, (const real_t*)qsat->ptr,
                       qsat->block_stride, xp, norms, g.ncols_pad, blockmax);
    HIP_TRY(hipGetLastError());
  }
  return 0;
}

}  // extern "C"
