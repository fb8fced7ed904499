// cloudsc2_driver.hip -- driver-level entry points (host pointers in the GLOBAL_STATE layout) and the resident state.
// These replace the bodies of the reference's three driver procedures: the OpenMP block loop becomes one launch over all blocks,
// thread-private scratch arrays (cloudsc_driver_tl_mod.F90:77-95, cloudsc_driver_ad_mod.F90:66-79) become device arrays over all blocks.

#include <thread>
#include "cloudsc2_host.hpp"

using namespace cloudsc2;

namespace {


__global__ void __launch_bounds__(256)
scale_planes_kernel(real_t* dst, long long dst_stride, const real_t* src, long long src_stride, long long plane, long long nblocks,
                    real_t factor) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= plane * nblocks) return;
  long long ibl = i / plane, r = i - ibl * plane;
  dst[ibl * dst_stride + r] = src[ibl * src_stride + r] * factor;
}

// One (NPROMA, nrows, NBLOCKS) array from one blocking to another (resident states the library blocks differently from the caller:
// cloudsc2_state_upload / _download).  Columns g < ncopy are copied; ncopy <= g < nzero are written as zero (whole blocks of the
// two arrays the driver zeroes, cloudsc_driver_mod.F90:87-88); everything else keeps its value.
__global__ void __launch_bounds__(256)
reblock_kernel(const real_t* __restrict__ src, int np_src, long long stride_src, real_t* __restrict__ dst, int np_dst,
               long long stride_dst, long long nrows, long long ncopy, long long nzero) {
  const long long total = nrows * nzero;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const long long row = e / nzero, g = e - row * nzero;
    const long long bd = g / np_dst, jd = g - bd * np_dst;
    real_t v = 0;
    if (g < ncopy) {
      const long long bs = g / np_src, js = g - bs * np_src;
      v = src[bs * stride_src + row * np_src + js];
    }
    dst[bd * stride_dst + row * np_dst + jd] = v;
  }
}

constexpr size_t kAlignReals = 256 / sizeof(real_t);
size_t r32(size_t n) { return (n + kAlignReals - 1) & ~(kAlignReals - 1); }
constexpr size_t kF64 = sizeof(double) / sizeof(real_t);  // real_t slots per fp64 statistic

struct Arena {
  real_t* base = nullptr;
  size_t cap = 0, used = 0;
  int device = -1;

  // sizes in elements of real_t; take_f64 carves fp64 arrays (statistics) out of the same allocation
  // `probe`: the sweep the placement search times on every candidate (state_probe below); none = the allocator's generic streams
  int reserve(size_t nreals, const ProbeFn* probe = nullptr, PlacePolicy policy = kPlaceSearch) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (base && (cap < nreals || dev != device)) { (void)device_free_impl(base); base = nullptr; cap = 0; }
    if (!base) {
      // placed: the fastest of several candidate allocations / compositions (cloudsc2_alloc.hip)
      int rc = device_malloc_impl((void**)&base, nreals * sizeof(real_t), probe, policy);
      if (rc) { base = nullptr; return rc; }
      cap = nreals;
      device = dev;
    }
    used = 0;
    return 0;
  }
  real_t* take(size_t n) {
    n = r32(n);  // keep every array 256-byte aligned
    real_t* p = base + used;
    used += n;
    return p;
  }
  double* take_f64(size_t n) { return (double*)take(n * (sizeof(double) / sizeof(real_t))); }
  void release() {
    if (base) (void)device_free_impl(base);
    base = nullptr; cap = 0; used = 0;
  }
};
Arena g_arena;
std::mutex g_arena_mutex;

struct DevState {
  // GLOBAL_STATE arrays (cloudsc2_array_state_mod.F90:26-79) on the device
  real_t *pt, *pq, *b_cml, *b_loc, *pap, *paph, *plu, *plude, *pmfu, *pmfd, *pa, *pclv, *psupsat, *pcovptot;
  real_t *pfplsl, *pfplsn, *pfhpsl, *pfhpsn, *qsat;
  long long S, H;  // block strides of full-level / half-level arrays
  long long nblocks;
};

// The whole state is ONE placed allocation.  Measured on one box, fresh processes, NL at 160 000 columns
// (profiles/r02_placement/z_one_arena_vs_split.txt): one arena 0.812 ms on 8 of 8; written arrays in a placed allocation and the
// read-only ones in a plain or in a second placed one 0.88-0.93 ms; no placement 0.90-0.96 ms -- where the INPUTS lie relative to
// the outputs matters in the mixed read/write sweep although a pure read stream does not care (r02_hbm_placement.md).
size_t state_out_reals(long long ncols_pad, int nlev) {
  size_t s = (size_t)ncols_pad * nlev, h = (size_t)ncols_pad * (nlev + 1);
  return 3 * r32(s) + 4 * r32(h) + r32(8 * s);
}
size_t state_in_reals(long long ncols_pad, int nlev) {
  size_t s = (size_t)ncols_pad * nlev, h = (size_t)ncols_pad * (nlev + 1);
  return 8 * r32(s) + r32(h) + r32(8 * s) + r32(5 * s);
}
size_t state_reals(long long ncols_pad, int nlev) { return state_in_reals(ncols_pad, nlev) + state_out_reals(ncols_pad, nlev); }

void state_take(Arena& a, DevState& d, long long ncols_pad, int nproma, int nlev) {
  Arena& ain = a;
  Arena& aout = a;  // read-only arrays first, then what the sweeps write
  size_t s = (size_t)ncols_pad * nlev, h = (size_t)ncols_pad * (nlev + 1);
  d.S = (long long)nproma * nlev;
  d.H = (long long)nproma * (nlev + 1);
  d.nblocks = ncols_pad / nproma;
  d.pt = ain.take(s); d.pq = ain.take(s); d.pap = ain.take(s); d.plu = ain.take(s); d.plude = ain.take(s);
  d.pmfu = ain.take(s); d.pmfd = ain.take(s); d.psupsat = ain.take(s);
  d.paph = ain.take(h); d.b_cml = ain.take(8 * s); d.pclv = ain.take(5 * s);
  d.pa = aout.take(s); d.pcovptot = aout.take(s); d.qsat = aout.take(s);
  d.pfplsl = aout.take(h); d.pfplsn = aout.take(h); d.pfhpsl = aout.take(h); d.pfhpsn = aout.take(h);
  d.b_loc = aout.take(8 * s);
}

struct HostState {
  const real_t *pt, *pq, *b_cml; real_t* b_loc;
  const real_t *pap, *paph, *plu, *plude, *pmfu, *pmfd; real_t* pa; const real_t *pclv, *psupsat;
  real_t *pcovptot, *pfplsl, *pfplsn, *pfhpsl, *pfhpsn;
};

// Host <-> device traffic of the driver-level entry points is PCIe-bound (the kernels take ~1 ms per 160 000 columns,
// the state is 39.5 KB per column), so only what the kernels read goes up and only what they write comes down:
//   up   9 full-level arrays + PAPH, planes T,Q,QL,QI of B_CML, planes QL,QI of PCLV      (17.5 KB / column)
//   down planes T,Q,QL,QI,QV of B_LOC, PA, PCOVPTOT, the four flux arrays                  (12.1 KB / column)
// Everything else keeps its host value: planes A,QR,QS of B_LOC and the padded tail columns of the last block are never
// written by the reference either (cloudsc_driver_mod.F90:84-107), so they are not transferred in either direction --
// except PCOVPTOT and CLD(:,:,NCLV), which the driver zeroes for whole blocks (:87-88).
int copy_planes(real_t* dst, const real_t* src, long long plane_off, long long plane, long long block_stride, long long nblocks,
                hipMemcpyKind kind, hipStream_t st) {
  // one (NPROMA, NLEV) plane of every block of an AoSoA buffer
  if (nblocks <= 0) return 0;
  HIP_TRY(hipMemcpy2DAsync(dst + plane_off, block_stride * sizeof(real_t), src + plane_off, block_stride * sizeof(real_t),
                           plane * sizeof(real_t), (size_t)nblocks, kind, st));
  return 0;
}

int upload(const HostState& h, const DevState& d, long long ncols_pad, int nlev, hipStream_t st) {
  size_t s = (size_t)ncols_pad * nlev * sizeof(real_t), hh = (size_t)ncols_pad * (nlev + 1) * sizeof(real_t);
  const long long P = d.S;
  HIP_TRY(hipMemcpyAsync(d.pt, h.pt, s, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d.pq, h.pq, s, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d.pap, h.pap, s, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d.paph, h.paph, hh, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d.plu, h.plu, s, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d.plude, h.plude, s, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d.pmfu, h.pmfu, s, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d.pmfd, h.pmfd, s, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d.psupsat, h.psupsat, s, hipMemcpyHostToDevice, st));
  int rc;
  for (int p : {0, 2, 3, 4})  // PGTENT, PGTENQ, PGTENL, PGTENI
    if ((rc = copy_planes(d.b_cml, h.b_cml, p * P, P, 8 * P, d.nblocks, hipMemcpyHostToDevice, st))) return rc;
  for (int p : {0, 1})        // PL, PI
    if ((rc = copy_planes(d.pclv, h.pclv, p * P, P, 5 * P, d.nblocks, hipMemcpyHostToDevice, st))) return rc;
  return 0;
}

// active part of one (NPROMA, NLEVx) array: whole blocks contiguously, then the rows of the partial last block; host and device
// copy may have different block strides (a plane of an AoSoA buffer on one side, a plain array on the other)
int download_active2(real_t* hdst, long long hstride, const real_t* dsrc, long long dstride, long long nlevx, int nproma,
                     long long ngptot, hipStream_t st) {
  const long long nfull = ngptot / nproma, icend = ngptot - nfull * nproma;
  const long long plane = (long long)nproma * nlevx;
  if (nfull > 0) {
    if (hstride == plane && dstride == plane) {
      HIP_TRY(hipMemcpyAsync(hdst, dsrc, (size_t)nfull * plane * sizeof(real_t), hipMemcpyDeviceToHost, st));
    } else {
      HIP_TRY(hipMemcpy2DAsync(hdst, hstride * sizeof(real_t), dsrc, dstride * sizeof(real_t), plane * sizeof(real_t), (size_t)nfull,
                               hipMemcpyDeviceToHost, st));
    }
  }
  if (icend > 0) {
    HIP_TRY(hipMemcpy2DAsync(hdst + nfull * hstride, (size_t)nproma * sizeof(real_t), dsrc + nfull * dstride, (size_t)nproma * sizeof(real_t),
                             (size_t)icend * sizeof(real_t), (size_t)nlevx, hipMemcpyDeviceToHost, st));
  }
  return 0;
}
int download_active(real_t* hdst, const real_t* dsrc, long long plane_off, long long nlevx, long long block_stride, int nproma,
                    long long ngptot, hipStream_t st) {
  return download_active2(hdst + plane_off, block_stride, dsrc + plane_off, block_stride, nlevx, nproma, ngptot, st);
}

int download(const HostState& h, const DevState& d, long long ncols_pad, int nlev, hipStream_t st, int nproma, long long ngptot) {
  const long long P = d.S, PH = d.H;
  int rc;
  for (int p : {0, 2, 3, 4})  // PTENT, PTENQ, PTENL, PTENI
    if ((rc = download_active(h.b_loc, d.b_loc, p * P, nlev, 8 * P, nproma, ngptot, st))) return rc;
  if ((rc = copy_planes(h.b_loc, d.b_loc, 7 * P, P, 8 * P, d.nblocks, hipMemcpyDeviceToHost, st))) return rc;  // CLD(:,:,NCLV) = 0
  if ((rc = download_active(h.pa, d.pa, 0, nlev, P, nproma, ngptot, st))) return rc;
  HIP_TRY(hipMemcpyAsync(h.pcovptot, d.pcovptot, (size_t)ncols_pad * nlev * sizeof(real_t), hipMemcpyDeviceToHost, st));
  if ((rc = download_active(h.pfplsl, d.pfplsl, 0, nlev + 1, PH, nproma, ngptot, st))) return rc;
  if ((rc = download_active(h.pfplsn, d.pfplsn, 0, nlev + 1, PH, nproma, ngptot, st))) return rc;
  if ((rc = download_active(h.pfhpsl, d.pfhpsl, 0, nlev + 1, PH, nproma, ngptot, st))) return rc;
  if ((rc = download_active(h.pfhpsn, d.pfhpsn, 0, nlev + 1, PH, nproma, ngptot, st))) return rc;
  return 0;
}

cloudsc2_field fld(real_t* p, long long stride) { cloudsc2_field f; f.ptr = p; f.block_stride = stride; return f; }

// Trajectory argument blocks in the driver-array -> kernel-dummy mapping of cloudsc_driver_mod.F90:94-107.
void traj_blocks(const DevState& d, int nproma, int nlev, bool with_qsat, cloudsc2_inputs& in, cloudsc2_outputs& out) {
  const long long S = d.S, H = d.H, P = (long long)nproma * nlev;
  in.paph = fld(d.paph, H); in.pap = fld(d.pap, S); in.q = fld(d.pq, S);
  in.qsat = fld(with_qsat ? d.qsat : nullptr, S); in.t = fld(d.pt, S);
  in.l = fld(d.pclv + 0 * P, 5 * S); in.i = fld(d.pclv + 1 * P, 5 * S);
  in.lude = fld(d.plude, S); in.lu = fld(d.plu, S); in.mfu = fld(d.pmfu, S); in.mfd = fld(d.pmfd, S);
  in.gtent = fld(d.b_cml + 0 * P, 8 * S); in.gtenq = fld(d.b_cml + 2 * P, 8 * S);
  in.gtenl = fld(d.b_cml + 3 * P, 8 * S); in.gteni = fld(d.b_cml + 4 * P, 8 * S);
  in.supsat = fld(d.psupsat, S);
  out.tent = fld(d.b_loc + 0 * P, 8 * S); out.tenq = fld(d.b_loc + 2 * P, 8 * S);
  out.tenl = fld(d.b_loc + 3 * P, 8 * S); out.teni = fld(d.b_loc + 4 * P, 8 * S);
  out.clc = fld(d.pa, S); out.covptot = fld(d.pcovptot, S);
  out.fplsl = fld(d.pfplsl, H); out.fplsn = fld(d.pfplsn, H); out.fhpsl = fld(d.pfhpsl, H); out.fhpsn = fld(d.pfhpsn, H);
}

// The sweep the placement search times on every candidate allocation of a state: the real NL kernel (SATUR fused, default
// constants) over a state laid out at the start of the candidate exactly as state_take lays it out, on all-zero fields (every
// candidate is cleared first, so all run the same path; the kernel's loads and stores do not depend on the data).
ProbeFn state_probe(int nproma, int nlev, int ngptot) {
  return [=](void* base, size_t bytes) {
    cloudsc2_params prm;
    cloudsc2_params_default(&prm);
    prm.nlev = nlev;
    prm.math_mode = 1;
    for (int k = 0; k < nlev && k < CLOUDSC2_MAX_NLEV; ++k) prm.ceta[k] = (k + 0.5) / nlev;
    Geom g;
    if (check_geom(&prm, nproma, nlev, ngptot, g)) return;
    if (state_reals(g.ncols_pad, nlev) * sizeof(real_t) > bytes) return;
    Arena view;
    view.base = (real_t*)base;
    view.cap = bytes / sizeof(real_t);
    DevState d;
    state_take(view, d, g.ncols_pad, nproma, nlev);
    cloudsc2_inputs in; cloudsc2_outputs out;
    traj_blocks(d, nproma, nlev, false, in, out);
    const cloudsc2_field zero = fld(d.b_loc + 7LL * nproma * nlev, 8 * d.S);
    (void)cloudsc2_nl_launch(&prm, 3600.0, nproma, nlev, ngptot, &in, &out, zero, 0.0, nullptr);
  };
}

// Which judge for an allocation of `total` reals that starts with a state of `state` reals: the NL sweep when the state is all there
// is; the allocator's two generic streams over the WHOLE buffer when more than 256 MiB follow the state (the perturbation sets and
// scratch of TL / AD).  Measured at 160 000 columns, fresh processes: judged by the NL sweep on the state part alone AD came out at
// 3.36-3.46 ms three times of four and TL at 1.91 once; by the NL sweep plus the generic streams on the tail, added up, TL 1.82-1.83
// two times of six (the candidates chosen were slow as a whole: a buffer's class is a property of the whole, not the sum of its
// parts); by the generic streams over the whole buffer TL 1.640-1.661 on 10 of 10 and AD 3.03-3.07 on 15 of 15.
const ProbeFn* judge_for(const ProbeFn& nl_probe, size_t total, size_t state) {
  return (total > state && (total - state) * sizeof(real_t) >= (256u << 20)) ? nullptr : &nl_probe;
}

struct FlatIn { cloudsc2_inputs in; };
void flat_in_take(Arena& a, long long ncols_pad, int nproma, int nlev, cloudsc2_inputs& in) {
  size_t s = (size_t)ncols_pad * nlev, h = (size_t)ncols_pad * (nlev + 1);
  const long long S = (long long)nproma * nlev, H = (long long)nproma * (nlev + 1);
  in.paph = fld(a.take(h), H);
  cloudsc2_field* f[15] = {&in.pap, &in.q, &in.qsat, &in.t, &in.l, &in.i, &in.lude, &in.lu, &in.mfu, &in.mfd,
                           &in.gtent, &in.gtenq, &in.gtenl, &in.gteni, &in.supsat};
  for (auto p : f) *p = fld(a.take(s), S);
}
void flat_out_take(Arena& a, long long ncols_pad, int nproma, int nlev, cloudsc2_outputs& out) {
  size_t s = (size_t)ncols_pad * nlev, h = (size_t)ncols_pad * (nlev + 1);
  const long long S = (long long)nproma * nlev, H = (long long)nproma * (nlev + 1);
  cloudsc2_field* f[6] = {&out.tent, &out.tenq, &out.tenl, &out.teni, &out.clc, &out.covptot};
  for (auto p : f) *p = fld(a.take(s), S);
  cloudsc2_field* g[4] = {&out.fplsl, &out.fplsn, &out.fhpsl, &out.fhpsn};
  for (auto p : g) *p = fld(a.take(h), H);
}
// One perturbation / adjoint set (16 inputs + 10 outputs) for all blocks.  NPROMA >= 64: separate (NPROMA,NLEVx,NBLOCKS) arrays.
// NPROMA < 64: ONE buffer (NPROMA, NLEV+1, 26, NBLOCKS), the AoSoA arrangement of the reference's tendency buffers -- a wave then
// spans two or more blocks, i.e. twice the streams, and with 26 separate arrays the TL / AD sweeps thrash the CU's address-
// translation cache (TL 2.86 -> 1.66 ms, AD 4.07 -> 3.23 ms at NPROMA 32, 160 000 columns; profiles/r02_utcl1_counters.txt);
// at NPROMA >= 64 the separate arrays are as fast (TL) or 4 % faster (AD).
constexpr int kPairPlanes = 26;
bool pair_blocked(int nproma) { return nproma < 64; }
size_t pair_reals(long long ncols_pad, int nlev) { return r32((size_t)kPairPlanes * (size_t)ncols_pad * (nlev + 1)); }
void pair_take(Arena& a, long long ncols_pad, int nproma, int nlev, cloudsc2_inputs& in, cloudsc2_outputs& out) {
  if (!pair_blocked(nproma)) {
    flat_in_take(a, ncols_pad, nproma, nlev, in);
    flat_out_take(a, ncols_pad, nproma, nlev, out);
    return;
  }
  const long long plane = (long long)nproma * (nlev + 1), stride = kPairPlanes * plane;
  real_t* base = a.take((size_t)kPairPlanes * (size_t)ncols_pad * (nlev + 1));
  cloudsc2_field* fi[16] = {&in.paph, &in.pap, &in.q, &in.qsat, &in.t, &in.l, &in.i, &in.lude, &in.lu, &in.mfu, &in.mfd,
                            &in.gtent, &in.gtenq, &in.gtenl, &in.gteni, &in.supsat};
  cloudsc2_field* fo[10] = {&out.tent, &out.tenq, &out.tenl, &out.teni, &out.clc, &out.fplsl, &out.fplsn, &out.fhpsl, &out.fhpsn,
                            &out.covptot};
  for (int k = 0; k < 16; ++k) *fi[k] = fld(base + k * plane, stride);
  for (int k = 0; k < 10; ++k) *fo[k] = fld(base + (16 + k) * plane, stride);
}

size_t flat_in_reals(long long ncols_pad, int nlev) { return 15 * r32((size_t)ncols_pad * nlev) + r32((size_t)ncols_pad * (nlev + 1)); }
size_t flat_out_reals(long long ncols_pad, int nlev) { return 6 * r32((size_t)ncols_pad * nlev) + 4 * r32((size_t)ncols_pad * (nlev + 1)); }

// Event pair around the kernels of one driver call.  The events belong to the object: every early error return of the
// callers destroys them.
struct Timer {
  hipEvent_t a = nullptr, b = nullptr;
  Timer() = default;
  Timer(const Timer&) = delete;
  Timer& operator=(const Timer&) = delete;
  ~Timer() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
  int start(hipStream_t st) {
    HIP_TRY(hipEventCreate(&a));
    HIP_TRY(hipEventCreate(&b));
    HIP_TRY(hipEventRecord(a, st));
    return 0;
  }
  int stop(hipStream_t st, double* ms) {
    HIP_TRY(hipEventRecord(b, st));
    HIP_TRY(hipEventSynchronize(b));
    float f = 0;
    HIP_TRY(hipEventElapsedTime(&f, a, b));
    if (ms) *ms = f;
    return 0;
  }
};

// Streams and events of the slab pipeline, released on every path out of nl_run_slabs.
struct SlabResources {
  hipStream_t s_up = nullptr, s_k = nullptr;
  std::vector<hipEvent_t> ev;
  SlabResources() = default;
  SlabResources(const SlabResources&) = delete;
  SlabResources& operator=(const SlabResources&) = delete;
  ~SlabResources() {
    for (auto e : ev) if (e) (void)hipEventDestroy(e);
    if (s_up) (void)hipStreamDestroy(s_up);
    if (s_k) (void)hipStreamDestroy(s_k);
  }
  int create(size_t nevents) {
    HIP_TRY(hipStreamCreateWithFlags(&s_up, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&s_k, hipStreamNonBlocking));
    ev.assign(nevents, nullptr);
    for (auto& e : ev) HIP_TRY(hipEventCreate(&e));
    return 0;
  }
};

// ---- CLOUDSC_DRIVER on host arrays: upload / kernel / download pipelined over slabs of NPROMA blocks -----------------
// The call is PCIe-bound (17.5 KB up + 12.1 KB down per column against ~6 bytes per nanosecond of kernel), so the blocks
// are processed in slabs: a helper thread uploads slab i+1 while this thread launches the kernel for slab i and
// downloads it -- the two directions of the link work at the same time.  (The caller's arrays are ordinary pageable
// memory; page-locking 6 GB per call would cost more than it saves.)
HostState host_view(const HostState& h, long long b0, const DevState& d) {
  const long long S = d.S, H = d.H;
  HostState v = h;
  v.pt += b0 * S; v.pq += b0 * S; v.b_cml += b0 * 8 * S; v.b_loc += b0 * 8 * S; v.pap += b0 * S; v.paph += b0 * H;
  v.plu += b0 * S; v.plude += b0 * S; v.pmfu += b0 * S; v.pmfd += b0 * S; v.pa += b0 * S; v.pclv += b0 * 5 * S;
  v.psupsat += b0 * S; v.pcovptot += b0 * S; v.pfplsl += b0 * H; v.pfplsn += b0 * H; v.pfhpsl += b0 * H; v.pfhpsn += b0 * H;
  return v;
}
DevState dev_view(const DevState& d, long long b0, long long nb) {
  const long long S = d.S, H = d.H;
  DevState v = d;
  v.pt += b0 * S; v.pq += b0 * S; v.b_cml += b0 * 8 * S; v.b_loc += b0 * 8 * S; v.pap += b0 * S; v.paph += b0 * H;
  v.plu += b0 * S; v.plude += b0 * S; v.pmfu += b0 * S; v.pmfd += b0 * S; v.pa += b0 * S; v.pclv += b0 * 5 * S;
  v.psupsat += b0 * S; v.pcovptot += b0 * S; v.pfplsl += b0 * H; v.pfplsn += b0 * H; v.pfhpsl += b0 * H; v.pfhpsn += b0 * H;
  v.qsat += b0 * S;
  v.nblocks = nb;
  return v;
}

int upload_slab_sync(const HostState& h, const DevState& d, long long ncols, int nlev, hipStream_t st) {
  int rc = upload(h, d, ncols, nlev, st);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(st));
  return 0;
}

int nl_run_slabs(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, const Geom& g, const HostState& h,
                 const DevState& d, double* kernel_ms) {
  const long long nb = d.nblocks;
  const long long slab_blocks = std::max<long long>(1, 16384 / nproma);  // ~290 MB up, ~200 MB down, ~0.3 ms of kernel per slab
  const long long nslabs = (nb + slab_blocks - 1) / slab_blocks;
  int device = 0;
  HIP_TRY(hipGetDevice(&device));
  SlabResources res;
  {
    const int rc_res = res.create((size_t)(2 * nslabs));
    if (rc_res) return rc_res;
  }
  const hipStream_t s_up = res.s_up, s_k = res.s_k;
  const std::vector<hipEvent_t>& ev = res.ev;

  std::atomic<long long> uploaded{0};
  std::atomic<int> up_rc{0};
  std::string up_err;
  auto slab_cols = [&](long long i, long long& b0, long long& nbs, long long& active) {
    b0 = i * slab_blocks;
    nbs = std::min(slab_blocks, nb - b0);
    active = std::min<long long>(nbs * nproma, (long long)ngptot - b0 * nproma);
  };
  std::thread uploader([&] {
    if (hipSetDevice(device) != hipSuccess) { up_rc = CLOUDSC2_EINVAL; up_err = "hipSetDevice failed in the upload thread"; return; }
    for (long long i = 0; i < nslabs && up_rc == 0; ++i) {
      long long b0, nbs, active;
      slab_cols(i, b0, nbs, active);
      int rc = upload_slab_sync(host_view(h, b0, d), dev_view(d, b0, nbs), nbs * nproma, nlev, s_up);
      if (rc) { up_err = g_err; up_rc = rc; return; }
      uploaded.store(i + 1, std::memory_order_release);
    }
  });

  int rc = 0;
  for (long long i = 0; i < nslabs && rc == 0; ++i) {
    while (uploaded.load(std::memory_order_acquire) <= i && up_rc == 0) std::this_thread::yield();
    if (up_rc != 0) break;
    long long b0, nbs, active;
    slab_cols(i, b0, nbs, active);
    const DevState dv = dev_view(d, b0, nbs);
    cloudsc2_inputs in; cloudsc2_outputs out;
    traj_blocks(dv, nproma, nlev, false, in, out);
    if (hipEventRecord(ev[2 * i], s_k) != hipSuccess) { rc = fail(CLOUDSC2_EINVAL, "hipEventRecord failed"); break; }
    // TENDENCY_LOC(IBL)%cld(:,:,NCLV)=0 (cloudsc_driver_mod.F90:88) is plane 7 of B_LOC
    rc = cloudsc2_nl_launch(prm, ptsphy, nproma, nlev, (int)active, &in, &out, fld(dv.b_loc + 7LL * nproma * nlev, 8 * dv.S), 0.0, s_k);
    if (rc) break;
    if (hipEventRecord(ev[2 * i + 1], s_k) != hipSuccess) { rc = fail(CLOUDSC2_EINVAL, "hipEventRecord failed"); break; }
    rc = download(host_view(h, b0, d), dv, nbs * nproma, nlev, s_k, nproma, active);
  }
  uploader.join();
  if (rc == 0 && up_rc != 0) rc = fail(up_rc, up_err.c_str());
  const hipError_t e_sync = hipStreamSynchronize(s_k);
  if (rc == 0 && e_sync != hipSuccess) rc = fail(CLOUDSC2_EINVAL, hipGetErrorString(e_sync));
  if (rc == 0 && kernel_ms) {
    double total = 0.0;
    for (long long i = 0; i < nslabs; ++i) {
      float f = 0.f;
      if (hipEventElapsedTime(&f, ev[2 * i], ev[2 * i + 1]) == hipSuccess) total += f;
    }
    *kernel_ms = total;  // sum over the slabs' launches
  }
  (void)g;
  return rc;
}

}  // namespace

extern "C" {

void cloudsc2_release_workspace(void) {
  std::lock_guard<std::mutex> lock(g_arena_mutex);
  g_arena.release();
}

int cloudsc2_nl_run(const cloudsc2_params* prm, int nproma, int nlev, int ngptot, double ptsphy, const cloudsc2_real* pt,
                    const cloudsc2_real* pq, const cloudsc2_real* b_cml, cloudsc2_real* b_loc, const cloudsc2_real* pap, const cloudsc2_real* paph,
                    const cloudsc2_real* plu, const cloudsc2_real* plude, const cloudsc2_real* pmfu, const cloudsc2_real* pmfd, cloudsc2_real* pa,
                    const cloudsc2_real* pclv, const cloudsc2_real* psupsat, cloudsc2_real* pcovptot, cloudsc2_real* pfplsl, cloudsc2_real* pfplsn,
                    cloudsc2_real* pfhpsl, cloudsc2_real* pfhpsn, double* kernel_ms) {
  Geom g;
  int rc = check_geom(prm, nproma, nlev, ngptot, g);
  if (rc) return rc;
  std::lock_guard<std::mutex> lock(g_arena_mutex);
  const ProbeFn probe = state_probe(nproma, nlev, ngptot);
  // (the call is PCIe-bound: its workspace is one plain hipMalloc unless CLOUDSC2_PLACE=1 asks for the search; cloudsc2_alloc.hip)
  if ((rc = g_arena.reserve(state_reals(g.ncols_pad, nlev), &probe, kPlaceOnRequest))) return rc;
  DevState d;
  state_take(g_arena, d, g.ncols_pad, nproma, nlev);
  HostState h = {pt, pq, b_cml, b_loc, pap, paph, plu, plude, pmfu, pmfd, pa, pclv, psupsat, pcovptot, pfplsl, pfplsn, pfhpsl, pfhpsn};
  return nl_run_slabs(prm, ptsphy, nproma, nlev, ngptot, g, h, d, kernel_ms);
}

// ---- the two self-tests on a state that is already on the device ------------------------------------------------------------
// `ws` supplies the thread-private scratch arrays of the reference drivers (cloudsc_driver_tl_mod.F90:77-95,
// cloudsc_driver_ad_mod.F90:66-79) as device arrays over all blocks; the caller has reserved taylor_ws_reals / adjoint_ws_reals.
}  // extern "C"
namespace {

// nproma_stat: the NPROMA of the statistic (ERROR_NORM sums over one block of the CALLER's blocking); the arrays may be blocked otherwise
size_t taylor_nsums(int ngptot, int nproma_stat) { return (size_t)(((long long)ngptot + nproma_stat - 1) / nproma_stat) * 10 * 2 * 10; }
size_t taylor_ws_reals(long long ncols_pad, int nproma, int nlev, int ngptot, int nproma_stat) {
  (void)nproma;
  const size_t nsums = taylor_nsums(ngptot, nproma_stat);
  // one perturbation set (increments + TL outputs), the per-column sums of the lambda sweep, the block sums
  return std::max(flat_in_reals(ncols_pad, nlev) + flat_out_reals(ncols_pad, nlev), pair_reals(ncols_pad, nlev)) +
         r32((size_t)(10 * kTaylorLambdas + 10) * (size_t)ncols_pad * kF64) + r32(nsums * kF64);
}
size_t adjoint_ws_reals(long long ncols_pad, int nlev) {
  const size_t ncol = (size_t)ncols_pad;
  return std::max(flat_in_reals(ncols_pad, nlev) + flat_out_reals(ncols_pad, nlev), pair_reals(ncols_pad, nlev)) + r32(ncol * nlev) +
         r32(3 * ncol * kF64) + r32(32 * kF64);
}

int taylor_compute(const cloudsc2_params* prm_in, const Geom& g, int nproma, int nlev, int ngptot, double ptsphy, const DevState& d,
                   Arena& ws, double znormg[10], double* kernel_ms, hipStream_t st, int nproma_stat) {
  const long long nblocks_stat = ((long long)ngptot + nproma_stat - 1) / nproma_stat;  // blocks of the statistic
  const size_t nsums = taylor_nsums(ngptot, nproma_stat);
  cloudsc2_inputs inc;
  cloudsc2_outputs tlo;
  pair_take(ws, g.ncols_pad, nproma, nlev, inc, tlo);   // the TL outputs in the layout of a perturbation set; no increments exist
  (void)inc;
  double* colsum = ws.take_f64((size_t)(10 * kTaylorLambdas + 10) * (size_t)g.ncols_pad);  // per-column sums of the lambda sweep
  double* sums = ws.take_f64(nsums);
  int rc;
  cloudsc2_inputs in; cloudsc2_outputs out;
  traj_blocks(d, nproma, nlev, true, in, out);
  // The verdict (cloudsc_driver_tl_mod.F90:272-311) looks for a V shape in |1 - ratio| whose right arm is pure round-off
  // of the finite differences; unless the caller asks for fast math explicitly it is evaluated with the precise-math
  // kernels (IEEE division, libm exp, the reference's operation order) so that this noise floor is the reference's own.
  // The mode travels in this call's own copy of the parameter block: nothing process-wide is touched.
  cloudsc2_params prm_call = *prm_in;
  if (prm_call.math_mode == 0) prm_call.math_mode = 2;
  const cloudsc2_params* prm = &prm_call;
  Timer tm;
  if ((rc = tm.start(st))) return rc;
  // PCOVPTOT and CLD(:,:,NCLV) are zeroed first (cloudsc_driver_tl_mod.F90:131-132), then SATUR (:135)
  HIP_TRY(hipMemsetAsync(d.pcovptot, 0, (size_t)g.ncols_pad * nlev * sizeof(real_t), st));
  {
    const long long plane = (long long)nproma * nlev, nblocks = g.ncols_pad / nproma, n = plane * nblocks;
    hipLaunchKernelGGL(scale_planes_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d.b_loc + 7 * plane, 8 * d.S,
                       (const real_t*)(d.b_loc + 7 * plane), 8 * d.S, plane, nblocks, RC(0.0));
  }
  if ((rc = cloudsc2_satur_launch(prm, nproma, nlev, ngptot, in.pap, in.t, in.qsat, st))) return rc;
  // The reference trajectory (:138-151) and the TL (:173-194) in ONE sweep: CLOUDSC2TL recomputes, level by level, the trajectory
  // CLOUDSC2 has just computed from the same inputs -- here with the same level function --, so the TL sweep stores it (C2F_TRAJ)
  // and no NL sweep runs at all; the increments (:156-171), dx = 0.01*x, are formed inside the sweep from the inputs it reads anyway.
  if ((rc = cloudsc2_tl_launch_self(prm, ptsphy, nproma, nlev, ngptot, &in, &out, 0.01, &tlo, nullptr, st))) return rc;
  // the ten perturbed NL runs (:197-230) and the ERROR_NORM sums (:233-244): one sweep with the lambdas on the lanes -- the state
  // is read once for all ten runs and no perturbed outputs exist in memory (taylor_column)
  if ((rc = cloudsc2_taylor_sweep_launch(prm, ptsphy, nproma, nlev, ngptot, nproma_stat, &in, &out, &tlo, colsum, sums, st))) return rc;
  if ((rc = tm.stop(st, kernel_ms))) return rc;
  std::vector<double> hs(nsums);
  HIP_TRY(hipMemcpyAsync(hs.data(), sums, nsums * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));

  const double eps = sizeof(real_t) == 4 ? 1.1920928955078125e-07 : 2.220446049250313e-16;  // EPSILON(1._JPRB)
  for (int il = 0; il < 10; ++il) {
    double zg = 0.0;
    for (long long b = 0; b < nblocks_stat; ++b) {
      double znorm = 0.0, zcount = 0.0;
      for (int f = 0; f < 10; ++f) {
        const double* p = &hs[((size_t)il * nblocks_stat + b) * 20 + f * 2];
        if (fabs(p[1]) > eps) {  // ERROR_NORM, cloudsc_driver_tl_mod.F90:27-30
          zcount += 1.0;
          znorm += fabs(p[0] / p[1]);
        }
      }
      if (znorm == 0.0 || zcount == 0.0) return fail(CLOUDSC2_ETLWRONG, "TL is totally wrong !!! (a block has no active statistics)");
      zg = fmax(zg, znorm / zcount);
    }
    znormg[il] = zg;
  }
  return 0;
}

int adjoint_compute(const cloudsc2_params* prm, const Geom& g, int nproma, int nlev, int ngptot, double ptsphy, const DevState& d,
                    Arena& ws, double* znormg, double* kernel_ms, hipStream_t st) {
  const long long nblocks = g.ncols_pad / nproma;
  const size_t ncol = (size_t)g.ncols_pad;
  cloudsc2_inputs x;
  cloudsc2_outputs y;
  pair_take(ws, g.ncols_pad, nproma, nlev, x, y);
  real_t* scratch = ws.take(ncol * nlev);
  double* norms = ws.take_f64(3 * ncol);
  double* gmax = ws.take_f64(32);
  int rc;
  cloudsc2_inputs in; cloudsc2_outputs out;
  traj_blocks(d, nproma, nlev, true, in, out);
  HIP_TRY(hipMemsetAsync(gmax, 0, sizeof(double), st));
  HIP_TRY(hipMemsetAsync(norms, 0, 3 * ncol * sizeof(double), st));
  Timer tm;
  if ((rc = tm.start(st))) return rc;
  // the driver zeroes PCOVPTOT and CLD(:,:,NCLV) first (cloudsc_driver_ad_mod.F90:113-114)
  HIP_TRY(hipMemsetAsync(d.pcovptot, 0, ncol * nlev * sizeof(real_t), st));
  {
    long long plane = (long long)nproma * nlev;
    long long n = plane * nblocks;
    hipLaunchKernelGGL(scale_planes_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d.b_loc + 7 * plane, 8 * d.S,
                       (const real_t*)(d.b_loc + 7 * plane), 8 * d.S, plane, nblocks, RC(0.0));
  }
  if ((rc = cloudsc2_satur_launch(prm, nproma, nlev, ngptot, in.pap, in.t, in.qsat, st))) return rc;   // :117
  // With the evaporation branch the reverse sweep needs the cover checkpoints, which only CLOUDSC2AD's forward sweep writes: both
  // sweeps then, and the norms by their own kernels.  Otherwise (every shipped configuration):
  //  * :124-139 + :160-181: dx = 0.01*x (ZSUPSAT = 0) is formed inside the TL sweep, which also leaves norm1 = <y,y> (:184-195)
  //    of every column while y is in registers;
  //  * :198-213 zeroes the 16 input adjoints and :216-237 accumulates into them: zero + accumulate == assign, which neither writes
  //    nor re-reads those planes;
  //  * CLOUDSC2AD's forward sweep (cloudsc2ad.F90:366-866) would recompute and rewrite the trajectory outputs the TL launch has just
  //    written from the same inputs with the same level function: the reverse sweep alone takes PFPLSL5 / PFPLSN5 from them;
  //  * norm2 = <x0, x_adj> and norm3 (:240-264) are formed in that sweep while x_adj is in registers.
  const bool evap = prm->levapls2 || prm->ldrain1d;
  const char* full = getenv("CLOUDSC2_AD_SYMMETRY_FULL");  // measurements only: the unfused sequence although nothing requires it
  if (evap || (full && atoi(full) != 0)) {
    if ((rc = cloudsc2_tl_launch_self(prm, ptsphy, nproma, nlev, ngptot, &in, &out, 0.0, &y, nullptr, st))) return rc;
    if ((rc = cloudsc2_adjoint_norms_launch(nproma, nlev, ngptot, nullptr, nullptr, &y, nullptr, norms, gmax, st))) return rc;
    if ((rc = cloudsc2_ad_launch_assign(prm, ptsphy, nproma, nlev, ngptot, &in, &out, &x, &y, scratch, st))) return rc;
    cloudsc2_field qf = in.qsat;
    if ((rc = cloudsc2_adjoint_norms_launch(nproma, nlev, ngptot, &in, &qf, nullptr, &x, norms, gmax, st))) return rc;
  } else {
    if ((rc = cloudsc2_tl_launch_self(prm, ptsphy, nproma, nlev, ngptot, &in, &out, 0.0, &y, norms, st))) return rc;
    if ((rc = cloudsc2_ad_launch_reverse_norms(prm, ptsphy, nproma, nlev, ngptot, &in, &out, &x, &y, norms, gmax, st))) return rc;
  }
  if ((rc = tm.stop(st, kernel_ms))) return rc;
  double hmax = 0.0;
  HIP_TRY(hipMemcpyAsync(&hmax, gmax, sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  *znormg = hmax;
  return 0;
}

}  // namespace

// ---- resident state: the library-owned GLOBAL_STATE on the device (include/cloudsc2_hip.h) ---------------------------------
// The device arrays of a resident state are blocked by `nproma`, which is the LIBRARY's choice: results do not depend on the blocking
// (every column is independent; tests/test_gpu_parity.py::test_results_do_not_depend_on_the_blocking) and nobody but the library
// addresses these arrays, so a caller's NPROMA that the sweeps dislike (32: a wave spans two blocks, TL / AD +8 %; 100: 800-byte
// rows) is replaced by 128.  `nproma_user` is the caller's: the blocking of the host arrays of upload / download, and the block of
// the Taylor test's ERROR_NORM statistic and of the validator's MINVAL / MAXVAL.
struct cloudsc2_state {
  int nproma = 0, nproma_user = 0, nlev = 0, ngptot = 0, device = 0;
  long long ncols_pad_user = 0;
  Geom g;
  Arena arena, ws, tmp;  // state arrays (one placed allocation); scratch of the self-tests; table staging + validation workspace
  DevState d;
};

namespace {
struct FieldSpec { int nlevx_extra; int ndim; };  // resolved by state_field()
int state_field(const cloudsc2_state* s, int field, cloudsc2_field* f, int* nlevx) {
  const DevState& d = s->d;
  const long long S = d.S, H = d.H, P = (long long)s->nproma * s->nlev;
  real_t* full[] = {d.pt, d.pq, d.pap, nullptr, d.plu, d.plude, d.pmfu, d.pmfd, d.pa, d.psupsat, d.pcovptot};
  *nlevx = s->nlev;
  if (field >= CLOUDSC2_F_PT && field <= CLOUDSC2_F_PCOVPTOT && field != CLOUDSC2_F_PAPH) { *f = fld(full[field], S); return 0; }
  switch (field) {
    case CLOUDSC2_F_PAPH: *f = fld(d.paph, H); *nlevx = s->nlev + 1; return 0;
    case CLOUDSC2_F_PFPLSL: *f = fld(d.pfplsl, H); *nlevx = s->nlev + 1; return 0;
    case CLOUDSC2_F_PFPLSN: *f = fld(d.pfplsn, H); *nlevx = s->nlev + 1; return 0;
    case CLOUDSC2_F_PFHPSL: *f = fld(d.pfhpsl, H); *nlevx = s->nlev + 1; return 0;
    case CLOUDSC2_F_PFHPSN: *f = fld(d.pfhpsn, H); *nlevx = s->nlev + 1; return 0;
    case CLOUDSC2_F_QSAT: *f = fld(d.qsat, S); return 0;
    default: break;
  }
  if (field >= CLOUDSC2_F_CML_T && field < CLOUDSC2_F_CML_T + 8) { *f = fld(d.b_cml + (field - CLOUDSC2_F_CML_T) * P, 8 * S); return 0; }
  if (field >= CLOUDSC2_F_LOC_T && field < CLOUDSC2_F_LOC_T + 8) { *f = fld(d.b_loc + (field - CLOUDSC2_F_LOC_T) * P, 8 * S); return 0; }
  if (field >= CLOUDSC2_F_PCLV_QL && field < CLOUDSC2_F_PCLV_QL + 5) { *f = fld(d.pclv + (field - CLOUDSC2_F_PCLV_QL) * P, 5 * S); return 0; }
  return fail(CLOUDSC2_EINVAL, "unknown field id");
}
// the blocking of a resident state's device arrays for a caller's NPROMA (CLOUDSC2_STATE_NPROMA: 0 = always the caller's; N = the
// block to use instead of the default 128 when the caller's is not a multiple of the wave size)
int state_blocking(int nproma_user) {
  const char* e = getenv("CLOUDSC2_STATE_NPROMA");
  const int want = (e && *e) ? atoi(e) : 128;
  return (want > 0 && nproma_user % 64 != 0) ? want : nproma_user;
}

int reblock(const real_t* src, int np_src, long long stride_src, real_t* dst, int np_dst, long long stride_dst, long long nrows,
            long long ncopy, long long nzero, hipStream_t st) {
  const long long total = nrows * nzero;
  if (total <= 0) return 0;
  const unsigned grid = (unsigned)std::min<long long>((total + 255) / 256, 256 * 64);
  hipLaunchKernelGGL(reblock_kernel, dim3(grid), dim3(256), 0, st, src, np_src, stride_src, dst, np_dst, stride_dst, nrows, ncopy, nzero);
  HIP_TRY(hipGetLastError());
  return 0;
}

// upload / download of a state whose device blocking differs from the host arrays': every array (or plane of an AoSoA buffer)
// goes through one staging array in the HOST's blocking and a re-blocking kernel.  Same transfer sets as upload() / download().
int upload_reblocked(cloudsc2_state* s, const HostState& h, hipStream_t st) {
  const int npu = s->nproma_user, npd = s->nproma, nlev = s->nlev;
  const long long nbu = s->ncols_pad_user / npu, Pu = (long long)npu * nlev, Hu = (long long)npu * (nlev + 1);
  const DevState& d = s->d;
  int rc;
  if ((rc = s->tmp.reserve(r32((size_t)s->ncols_pad_user * (nlev + 1)), nullptr, kPlacePlain))) return rc;
  real_t* stage = s->tmp.take((size_t)s->ncols_pad_user * (nlev + 1));
  auto one = [&](const real_t* hsrc, long long hstride, long long nlevx, real_t* ddst, long long dstride) -> int {
    const long long plane = (long long)npu * nlevx;
    HIP_TRY(hipMemcpy2DAsync(stage, plane * sizeof(real_t), hsrc, hstride * sizeof(real_t), plane * sizeof(real_t), (size_t)nbu,
                             hipMemcpyHostToDevice, st));
    return reblock(stage, npu, plane, ddst, npd, dstride, nlevx, s->ngptot, s->ngptot, st);
  };
  const long long S = d.S, H = d.H, P = (long long)npd * nlev;
  if ((rc = one(h.pt, Pu, nlev, d.pt, S)) || (rc = one(h.pq, Pu, nlev, d.pq, S)) || (rc = one(h.pap, Pu, nlev, d.pap, S)) ||
      (rc = one(h.paph, Hu, nlev + 1, d.paph, H)) || (rc = one(h.plu, Pu, nlev, d.plu, S)) || (rc = one(h.plude, Pu, nlev, d.plude, S)) ||
      (rc = one(h.pmfu, Pu, nlev, d.pmfu, S)) || (rc = one(h.pmfd, Pu, nlev, d.pmfd, S)) || (rc = one(h.psupsat, Pu, nlev, d.psupsat, S)))
    return rc;
  for (int p : {0, 2, 3, 4})  // PGTENT, PGTENQ, PGTENL, PGTENI
    if ((rc = one(h.b_cml + p * Pu, 8 * Pu, nlev, d.b_cml + p * P, 8 * S))) return rc;
  for (int p : {0, 1})        // PL, PI
    if ((rc = one(h.pclv + p * Pu, 5 * Pu, nlev, d.pclv + p * P, 5 * S))) return rc;
  return 0;
}

int download_reblocked(cloudsc2_state* s, const HostState& h, hipStream_t st) {
  const int npu = s->nproma_user, npd = s->nproma, nlev = s->nlev;
  const long long nbu = s->ncols_pad_user / npu, Pu = (long long)npu * nlev, Hu = (long long)npu * (nlev + 1);
  const DevState& d = s->d;
  int rc;
  if ((rc = s->tmp.reserve(r32((size_t)s->ncols_pad_user * (nlev + 1)), nullptr, kPlacePlain))) return rc;
  real_t* stage = s->tmp.take((size_t)s->ncols_pad_user * (nlev + 1));
  // whole = false: the active columns only (padded tails keep their host values, as under the reference); true: whole blocks, the
  // padding zero (PCOVPTOT and CLD(:,:,NCLV), which the driver zeroes block-wise, cloudsc_driver_mod.F90:87-88)
  auto one = [&](real_t* hdst, long long hstride, long long nlevx, const real_t* dsrc, long long dstride, bool whole) -> int {
    const long long plane = (long long)npu * nlevx;
    int r = reblock(dsrc, npd, dstride, stage, npu, plane, nlevx, s->ngptot, whole ? s->ncols_pad_user : (long long)s->ngptot, st);
    if (r) return r;
    if (!whole) return download_active2(hdst, hstride, stage, plane, nlevx, npu, s->ngptot, st);
    HIP_TRY(hipMemcpy2DAsync(hdst, hstride * sizeof(real_t), stage, plane * sizeof(real_t), plane * sizeof(real_t), (size_t)nbu,
                             hipMemcpyDeviceToHost, st));
    return 0;
  };
  const long long S = d.S, H = d.H, P = (long long)npd * nlev;
  for (int p : {0, 2, 3, 4})  // PTENT, PTENQ, PTENL, PTENI
    if ((rc = one(h.b_loc + p * Pu, 8 * Pu, nlev, d.b_loc + p * P, 8 * S, false))) return rc;
  if ((rc = one(h.b_loc + 7 * Pu, 8 * Pu, nlev, d.b_loc + 7 * P, 8 * S, true))) return rc;  // CLD(:,:,NCLV) = 0
  if ((rc = one(h.pa, Pu, nlev, d.pa, S, false)) || (rc = one(h.pcovptot, Pu, nlev, d.pcovptot, S, true)) ||
      (rc = one(h.pfplsl, Hu, nlev + 1, d.pfplsl, H, false)) || (rc = one(h.pfplsn, Hu, nlev + 1, d.pfplsn, H, false)) ||
      (rc = one(h.pfhpsl, Hu, nlev + 1, d.pfhpsl, H, false)) || (rc = one(h.pfhpsn, Hu, nlev + 1, d.pfhpsn, H, false)))
    return rc;
  return 0;
}

int state_check(const cloudsc2_state* s) {
  if (!s) return fail(CLOUDSC2_EINVAL, "NULL state handle");
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev != s->device) return fail(CLOUDSC2_EINVAL, "the state lives on another HIP device than the calling thread's current one");
  return 0;
}
}  // namespace

extern "C" {

int cloudsc2_state_create(int nproma, int nlev, int ngptot, cloudsc2_state** out) {
  if (!out) return fail(CLOUDSC2_EINVAL, "NULL result pointer");
  *out = nullptr;
  if (nproma < 1 || nlev < 2 || ngptot < 1 || nlev > CLOUDSC2_MAX_NLEV) return fail(CLOUDSC2_EINVAL, "bad dimensions");
  if (int rc = require_device()) return rc;
  cloudsc2_state* s = new cloudsc2_state;
  s->nproma_user = nproma;
  s->ncols_pad_user = (((long long)ngptot + nproma - 1) / nproma) * nproma;
  nproma = state_blocking(nproma);  // from here on: the blocking of the device arrays
  s->nproma = nproma; s->nlev = nlev; s->ngptot = ngptot;
  const long long nblocks = ((long long)ngptot + nproma - 1) / nproma;
  s->g.nproma = nproma; s->g.nlev = nlev; s->g.ngptot = ngptot; s->g.ncols_pad = nblocks * nproma; s->g.kb0 = s->g.kb1 = 0; s->g.fair = 0;
  int rc = hipGetDevice(&s->device) == hipSuccess ? 0 : fail(CLOUDSC2_EINVAL, "hipGetDevice failed");
  const size_t n = state_reals(s->g.ncols_pad, nlev);
  const ProbeFn probe = state_probe(nproma, nlev, ngptot);
  if (!rc) rc = s->arena.reserve(n, &probe);  // ONE placed allocation for the whole state (cloudsc2_alloc.hip), judged by the NL sweep
  if (!rc && hipMemset(s->arena.base, 0, n * sizeof(real_t)) != hipSuccess) rc = fail(CLOUDSC2_EINVAL, "hipMemset failed");
  if (rc) { s->arena.release(); delete s; return rc; }
  state_take(s->arena, s->d, s->g.ncols_pad, nproma, nlev);  // FIELD_INIT: everything zero (cloudsc2_array_state_mod.F90:186-190)
  *out = s;
  return 0;
}

void cloudsc2_state_destroy(cloudsc2_state* s) {
  if (!s) return;
  s->arena.release(); s->ws.release(); s->tmp.release();
  delete s;
}

int cloudsc2_state_field(const cloudsc2_state* s, int field, cloudsc2_field* f) {
  int rc = state_check(s);
  if (rc) return rc;
  if (!f) return fail(CLOUDSC2_EINVAL, "NULL field");
  int nlevx;
  return state_field(s, field, f, &nlevx);
}

int cloudsc2_state_blocking(const cloudsc2_state* s, int* nproma_device, int* nproma_caller) {
  if (!s) return fail(CLOUDSC2_EINVAL, "NULL state handle");
  if (nproma_device) *nproma_device = s->nproma;
  if (nproma_caller) *nproma_caller = s->nproma_user;
  return 0;
}

int cloudsc2_state_expand(cloudsc2_state* s, int field, const cloudsc2_real* table, int klon, int period, long long start) {
  int rc = state_check(s);
  if (rc) return rc;
  if (!table) return fail(CLOUDSC2_EINVAL, "NULL table");
  cloudsc2_field f; int nlevx;
  if ((rc = state_field(s, field, &f, &nlevx))) return rc;
  const size_t n = (size_t)klon * nlevx;
  if ((rc = s->tmp.reserve(r32(n) + r32(cloudsc2_validate_workspace_doubles() * kF64) + r32(8 * kF64), nullptr, kPlacePlain))) return rc;
  real_t* dtab = s->tmp.take(n);
  HIP_TRY(hipMemcpy(dtab, table, n * sizeof(real_t), hipMemcpyHostToDevice));
  if ((rc = cloudsc2_expand_launch(dtab, klon, period, start, nlevx, 1, s->nproma, s->ngptot, f, nullptr))) return rc;
  HIP_TRY(hipStreamSynchronize(nullptr));
  return 0;
}

int cloudsc2_state_validate(cloudsc2_state* s, int field, int ndim, const cloudsc2_real* ref_table, int klon, int period, long long start,
                            double stats[5]) {
  int rc = state_check(s);
  if (rc) return rc;
  if (!ref_table || !stats || ndim < 1) return fail(CLOUDSC2_EINVAL, "bad argument");
  cloudsc2_field f; int nlevx;
  if ((rc = state_field(s, field, &f, &nlevx))) return rc;
  const size_t n = (size_t)klon * nlevx * ndim;
  const size_t nws = (size_t)cloudsc2_validate_workspace_doubles();
  if ((rc = s->tmp.reserve(r32(n) + r32(nws * kF64) + r32(8 * kF64), nullptr, kPlacePlain))) return rc;
  real_t* dtab = s->tmp.take(n);
  double* wsd = s->tmp.take_f64(nws);
  double* dst = s->tmp.take_f64(8);
  HIP_TRY(hipMemcpy(dtab, ref_table, n * sizeof(real_t), hipMemcpyHostToDevice));
  // MINVAL / MAXVAL over whole blocks of the caller's blocking (validate_mod.F90:186-187)
  if ((rc = validate_launch_impl(dtab, klon, period, start, nlevx, ndim, s->nproma, s->ngptot, f, wsd, dst, nullptr, s->ncols_pad_user)))
    return rc;
  HIP_TRY(hipMemcpy(stats, dst, 5 * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

#define C2_HOST18 pt, pq, b_cml, b_loc, pap, paph, plu, plude, pmfu, pmfd, pa, pclv, psupsat, pcovptot, pfplsl, pfplsn, pfhpsl, pfhpsn
int cloudsc2_state_upload(cloudsc2_state* s, const cloudsc2_real* pt, const cloudsc2_real* pq, const cloudsc2_real* b_cml, cloudsc2_real* b_loc,
                          const cloudsc2_real* pap, const cloudsc2_real* paph, const cloudsc2_real* plu, const cloudsc2_real* plude,
                          const cloudsc2_real* pmfu, const cloudsc2_real* pmfd, cloudsc2_real* pa, const cloudsc2_real* pclv,
                          const cloudsc2_real* psupsat, cloudsc2_real* pcovptot, cloudsc2_real* pfplsl, cloudsc2_real* pfplsn,
                          cloudsc2_real* pfhpsl, cloudsc2_real* pfhpsn) {
  int rc = state_check(s);
  if (rc) return rc;
  HostState h = {C2_HOST18};
  if (s->nproma == s->nproma_user) rc = upload(h, s->d, s->g.ncols_pad, s->nlev, nullptr);
  else rc = upload_reblocked(s, h, nullptr);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(nullptr));
  return 0;
}

int cloudsc2_state_download(cloudsc2_state* s, cloudsc2_real* b_loc, cloudsc2_real* pa, cloudsc2_real* pcovptot, cloudsc2_real* pfplsl,
                            cloudsc2_real* pfplsn, cloudsc2_real* pfhpsl, cloudsc2_real* pfhpsn) {
  int rc = state_check(s);
  if (rc) return rc;
  HostState h = {};
  h.b_loc = b_loc; h.pa = pa; h.pcovptot = pcovptot; h.pfplsl = pfplsl; h.pfplsn = pfplsn; h.pfhpsl = pfhpsl; h.pfhpsn = pfhpsn;
  if (!b_loc || !pa || !pcovptot || !pfplsl || !pfplsn || !pfhpsl || !pfhpsn) return fail(CLOUDSC2_EINVAL, "NULL output array");
  if (s->nproma == s->nproma_user) rc = download(h, s->d, s->g.ncols_pad, s->nlev, nullptr, s->nproma, s->ngptot);
  else rc = download_reblocked(s, h, nullptr);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(nullptr));
  return 0;
}

int cloudsc2_device_malloc_state(void** ptr, size_t bytes, int nproma, int nlev, int ngptot) {
  if (nproma < 1 || nlev < 2 || nlev > CLOUDSC2_MAX_NLEV || ngptot < 1) return fail(CLOUDSC2_EINVAL, "cloudsc2_device_malloc_state: bad geometry");
  const long long ncols_pad = (((long long)ngptot + nproma - 1) / nproma) * nproma;
  if (bytes < state_reals(ncols_pad, nlev) * sizeof(real_t))
    return fail(CLOUDSC2_EINVAL, "cloudsc2_device_malloc_state: fewer bytes than a state of this geometry needs");
  const ProbeFn probe = state_probe(nproma, nlev, ngptot);
  return device_malloc_impl(ptr, bytes, judge_for(probe, bytes / sizeof(real_t), state_reals(ncols_pad, nlev)));
}

int cloudsc2_state_nl(cloudsc2_state* s, const cloudsc2_params* prm, double ptsphy, int repeats, double* kernel_ms) {
  int rc = state_check(s);
  if (rc) return rc;
  if (repeats < 1) return fail(CLOUDSC2_EINVAL, "repeats >= 1 required");
  cloudsc2_inputs in; cloudsc2_outputs out;
  traj_blocks(s->d, s->nproma, s->nlev, false, in, out);
  const cloudsc2_field zero = fld(s->d.b_loc + 7LL * s->nproma * s->nlev, 8 * s->d.S);  // CLD(:,:,NCLV)=0, cloudsc_driver_mod.F90:88
  Timer tm;
  if ((rc = tm.start(nullptr))) return rc;
  for (int k = 0; k < repeats; ++k)
    if ((rc = cloudsc2_nl_launch(prm, ptsphy, s->nproma, s->nlev, s->ngptot, &in, &out, zero, 0.0, nullptr))) return rc;
  double ms = 0.0;
  if ((rc = tm.stop(nullptr, &ms))) return rc;
  if (kernel_ms) *kernel_ms = ms / repeats;
  return 0;
}

int cloudsc2_state_tl_taylor(cloudsc2_state* s, const cloudsc2_params* prm, double ptsphy, double znormg[10], double* kernel_ms) {
  int rc = state_check(s);
  if (rc) return rc;
  if (!prm || !znormg) return fail(CLOUDSC2_EINVAL, "NULL argument");
  Geom g;
  if ((rc = check_geom(prm, s->nproma, s->nlev, s->ngptot, g))) return rc;
  if ((rc = s->ws.reserve(taylor_ws_reals(g.ncols_pad, s->nproma, s->nlev, s->ngptot, s->nproma_user)))) return rc;
  return taylor_compute(prm, g, s->nproma, s->nlev, s->ngptot, ptsphy, s->d, s->ws, znormg, kernel_ms, nullptr, s->nproma_user);
}

int cloudsc2_state_ad_symmetry(cloudsc2_state* s, const cloudsc2_params* prm, double ptsphy, double* znormg, double* kernel_ms) {
  int rc = state_check(s);
  if (rc) return rc;
  if (!prm || !znormg) return fail(CLOUDSC2_EINVAL, "NULL argument");
  Geom g;
  if ((rc = check_geom(prm, s->nproma, s->nlev, s->ngptot, g))) return rc;
  if ((rc = s->ws.reserve(adjoint_ws_reals(g.ncols_pad, s->nlev)))) return rc;
  return adjoint_compute(prm, g, s->nproma, s->nlev, s->ngptot, ptsphy, s->d, s->ws, znormg, kernel_ms, nullptr);
}

// ---- the same two tests on HOST arrays: upload, compute, download (what CLOUDSC_DRIVER_TL / _AD bind) ------------------------
int cloudsc2_tl_taylor_run(const cloudsc2_params* prm, int nproma, int nlev, int ngptot, double ptsphy, const cloudsc2_real* pt,
                           const cloudsc2_real* pq, const cloudsc2_real* b_cml, cloudsc2_real* b_loc, const cloudsc2_real* pap, const cloudsc2_real* paph,
                           const cloudsc2_real* plu, const cloudsc2_real* plude, const cloudsc2_real* pmfu, const cloudsc2_real* pmfd, cloudsc2_real* pa,
                           const cloudsc2_real* pclv, const cloudsc2_real* psupsat, cloudsc2_real* pcovptot, cloudsc2_real* pfplsl, cloudsc2_real* pfplsn,
                           cloudsc2_real* pfhpsl, cloudsc2_real* pfhpsn, double znormg[10], double* kernel_ms) {
  Geom g;
  int rc = check_geom(prm, nproma, nlev, ngptot, g);
  if (rc) return rc;
  if (!znormg) return fail(CLOUDSC2_EINVAL, "znormg is NULL");
  std::lock_guard<std::mutex> lock(g_arena_mutex);
  const ProbeFn probe = state_probe(nproma, nlev, ngptot);
  const size_t n_state = state_reals(g.ncols_pad, nlev), n_all = n_state + taylor_ws_reals(g.ncols_pad, nproma, nlev, ngptot, nproma);
  if ((rc = g_arena.reserve(n_all, judge_for(probe, n_all, n_state), kPlaceOnRequest))) return rc;
  DevState d;
  state_take(g_arena, d, g.ncols_pad, nproma, nlev);
  HostState h = {C2_HOST18};
  hipStream_t st = nullptr;
  if ((rc = upload(h, d, g.ncols_pad, nlev, st))) return rc;
  if ((rc = taylor_compute(prm, g, nproma, nlev, ngptot, ptsphy, d, g_arena, znormg, kernel_ms, st, nproma))) return rc;
  if ((rc = download(h, d, g.ncols_pad, nlev, st, nproma, ngptot))) return rc;
  HIP_TRY(hipStreamSynchronize(st));
  return 0;
}

int cloudsc2_ad_symmetry_run(const cloudsc2_params* prm, int nproma, int nlev, int ngptot, double ptsphy, const cloudsc2_real* pt,
                             const cloudsc2_real* pq, const cloudsc2_real* b_cml, cloudsc2_real* b_loc, const cloudsc2_real* pap, const cloudsc2_real* paph,
                             const cloudsc2_real* plu, const cloudsc2_real* plude, const cloudsc2_real* pmfu, const cloudsc2_real* pmfd, cloudsc2_real* pa,
                             const cloudsc2_real* pclv, const cloudsc2_real* psupsat, cloudsc2_real* pcovptot, cloudsc2_real* pfplsl, cloudsc2_real* pfplsn,
                             cloudsc2_real* pfhpsl, cloudsc2_real* pfhpsn, double* znormg, double* kernel_ms) {
  Geom g;
  int rc = check_geom(prm, nproma, nlev, ngptot, g);
  if (rc) return rc;
  if (!znormg) return fail(CLOUDSC2_EINVAL, "znormg is NULL");
  std::lock_guard<std::mutex> lock(g_arena_mutex);
  const ProbeFn probe = state_probe(nproma, nlev, ngptot);
  const size_t n_state = state_reals(g.ncols_pad, nlev), n_all = n_state + adjoint_ws_reals(g.ncols_pad, nlev);
  if ((rc = g_arena.reserve(n_all, judge_for(probe, n_all, n_state), kPlaceOnRequest))) return rc;
  DevState d;
  state_take(g_arena, d, g.ncols_pad, nproma, nlev);
  HostState h = {C2_HOST18};
  hipStream_t st = nullptr;
  if ((rc = upload(h, d, g.ncols_pad, nlev, st))) return rc;
  if ((rc = adjoint_compute(prm, g, nproma, nlev, ngptot, ptsphy, d, g_arena, znormg, kernel_ms, st))) return rc;
  if ((rc = download(h, d, g.ncols_pad, nlev, st, nproma, ngptot))) return rc;
  HIP_TRY(hipStreamSynchronize(st));
  return 0;
}
#undef C2_HOST18

}  // extern "C"
