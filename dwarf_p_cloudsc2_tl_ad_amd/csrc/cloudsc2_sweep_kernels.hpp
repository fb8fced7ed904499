// cloudsc2_sweep_kernels.hpp -- the __global__ wrappers of the column sweeps (NL, TL, AD, the Taylor test's lambda sweep), their
// compile-time variant tables and what they share.  The sweeps are built as one translation unit per kernel family so that an edit to
// one sweep does not rebuild every variant table (~70 s as one unit): cloudsc2_kern.hip, compiled once with -DC2_FAMILY=<unit> for every
// name of the Makefile's FAMILIES, instantiates the unit's tables and exports each through one accessor (nl_variant(F) ...).  Which
// tables there are, and which unit builds which, is the table of C2_ROWS_<unit> below; the host units are listed in cloudsc2_host.hpp.
// -DC2_SINGLE_TU puts the sweeps and their launchers into ONE code object again (cloudsc2_launch.hip then defines every row's table):
// the experiment builds of `make variant`, `make asm`, `make resources` and the -DC2_WAVE_TIMES diagnostic, whose log pointer is a
// __device__ global that separate code objects cannot share.
#pragma once
#include <hip/hip_runtime.h>

#include <array>
#include <utility>

#include "cloudsc2_column.hpp"

namespace cloudsc2 {

// ---------------------------------------------------------------------------------------------------------
// kernels: thin wrappers around the per-column functions of cloudsc2_column.hpp.  Every kernel has ONE by-value
// argument block; the device code reads it in place from the kernel-argument segment (scalar cache).
// ---------------------------------------------------------------------------------------------------------
constexpr int kBlock = 128;

__device__ __forceinline__ long long global_column() { return (long long)blockIdx.x * blockDim.x + threadIdx.x; }

#if defined(__HIP_DEVICE_COMPILE__)
template <class T>
__device__ __forceinline__ const C2_CONST_AS T* kernarg() {
  return (const C2_CONST_AS T*)__builtin_amdgcn_kernarg_segment_ptr();
}
#define C2_KERNEL_BODY(call) call
#else
#define C2_KERNEL_BODY(call)
#endif

// -DC2_WAVE_TIMES (diagnostic build, tools/wave_times.py): every wave of the NL kernel logs when it started and ended (the 100 MHz
// constant clock) and where it ran (HW_ID, XCC_ID) -- how evenly a launch's waves start, progress and finish.
#ifdef C2_WAVE_TIMES
#ifndef C2_SINGLE_TU
#error "-DC2_WAVE_TIMES needs -DC2_SINGLE_TU (one code object: the log pointer is a __device__ global)"
#endif
__device__ unsigned long long* g_wave_log = nullptr;  // [wave][4]: start, end, HW_ID, XCC_ID
#define C2_WAVE_LOG_BEGIN const unsigned long long c2_t0 = __builtin_amdgcn_s_memrealtime();
#define C2_WAVE_LOG_END                                                                                         \
  if (g_wave_log && (threadIdx.x & 63) == 0) {                                                                  \
    unsigned long long* e = g_wave_log + 4 * (((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6);         \
    e[0] = c2_t0; e[1] = __builtin_amdgcn_s_memrealtime();                                                     \
    e[2] = __builtin_amdgcn_s_getreg((31 << 11) | 4); e[3] = __builtin_amdgcn_s_getreg((31 << 11) | 20);        \
  }
#else
#define C2_WAVE_LOG_BEGIN
#define C2_WAVE_LOG_END
#endif

// The NL variants without the evaporation branch fit 168 VGPRs (3 waves per SIMD) even with the two-level-deep
// prefetch; asking for it keeps the allocator from spending a few registers too many.  The others take what they need.
// (nl_waves_per_simd, cloudsc2_column.hpp)
template <unsigned F>
__global__ void __launch_bounds__(kBlock, nl_waves_per_simd(F)) nl_kernel(NlArgs args) {
  C2_KERNEL_BODY(C2_WAVE_LOG_BEGIN);
  C2_KERNEL_BODY((nl_column<F>(global_column(), kernarg<NlArgs>())));
  C2_KERNEL_BODY(C2_WAVE_LOG_END);
}
// SATUR + CLOUDSC2, and the adjoint's trajectory pass as a kernel of its own (C2F_CKPT).  The .NOT.LPHYLIN form exists for the plain
// sweep only: no shipped main uses it, the Taylor test's perturbed runs and the adjoint's trajectory pass belong to CLOUDSC2TL /
// CLOUDSC2AD, which have the LPHYLIN form alone; the trajectory pass differs from the plain NL sweep only with the evaporation
// branch: the cover checkpoint.
constexpr bool nl_variant_valid(unsigned f) {
  return (f & C2F_CKPT) ? ((f & C2F_EVAP) && !(f & (C2F_PERT | C2F_NOLIN))) : !((f & C2F_NOLIN) && (f & C2F_PERT));
}

// fp32 only: the TL variants with 32-bit offsets and without the evaporation branch need 173 VGPRs; held to 168 (3 waves
// per SIMD) they spill at most 7 dwords, and all 2500 waves of a 160 000-column launch are resident at once instead of
// 2048 + 452 (0.94 -> 0.88 ms).  Every other TL variant, and the fp64 ones, spill heavily below what they ask for.
// (tl_waves_per_simd, cloudsc2_column.hpp: every kernel over tl_column is built under this bound)
template <unsigned F>
__global__ void __launch_bounds__(kBlock, tl_waves_per_simd(F)) tl_kernel(TlArgs args) {
  C2_KERNEL_BODY(C2_WAVE_LOG_BEGIN);
  C2_KERNEL_BODY((tl_column<F>(global_column(), kernarg<TlArgs>())));
  C2_KERNEL_BODY(C2_WAVE_LOG_END);
}
// CLOUDSC2TL: every word below 64, and with C2F_SATLIN (SATUR differentiated in the sweep) -- without QSAT, TRAJ, SELFINC -- PRECISE x
// EVAP x OFF32
constexpr bool tl_variant_valid(unsigned f) { return f < 64u || (f & ~(C2F_PRECISE | C2F_EVAP | C2F_OFF32)) == C2F_SATLIN; }

// CLOUDSC2AD is launched fused (ad_kernel: one kernel runs a column's trajectory pass and then its reverse pass; waves in the
// bandwidth-heavy forward phase and waves in the arithmetic-heavy reverse phase share the CUs) or split (nl_kernel, then
// ad_reverse_kernel, in stream order).  fp64: the two forms measure the same at every size (both passes need one wave per
// SIMD's worth of registers in the fused kernel anyway), so it is always fused.  fp32: the trajectory pass alone runs six waves
// per SIMD instead of the fused kernel's two, which is worth 7 % when the whole launch is one round of waves (160 000 columns:
// 1.71 -> 1.59 ms) and nothing at 1 M columns (9.09 vs 9.17 ms), so launches of at most kAdSplitBelow columns are split.
constexpr bool kAdSplitSmall = sizeof(real_t) == 4;
constexpr long long kAdSplitBelow = 400000;
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, 64));
  return v;
}
__device__ __forceinline__ void atomic_max_pos(double* addr, double v) {
  // v >= 0: the IEEE bit pattern of non-negative doubles orders like unsigned integers
  atomicMax((unsigned long long*)addr, (unsigned long long)__double_as_longlong(v));
}
template <unsigned F>
__global__ void __launch_bounds__(kBlock, 1) ad_reverse_kernel(AdArgs args) {
  C2_KERNEL_BODY(C2_WAVE_LOG_BEGIN);
#if defined(__HIP_DEVICE_COMPILE__)
  if constexpr ((F & C2F_ADNORM) != 0) {  // the adjoint test's norms formed in the sweep: the wave's largest |norm3| joins the global one
    const double m = wave_max(ad_reverse_column<F>(global_column(), kernarg<AdArgs>()));
    if ((threadIdx.x & 63) == 0) atomic_max_pos(kernarg<AdArgs>()->gmax, m);
  } else {
    ad_reverse_column<F>(global_column(), kernarg<AdArgs>());
  }
#endif
  C2_KERNEL_BODY(C2_WAVE_LOG_END);
}
template <unsigned F>
__global__ void __launch_bounds__(kBlock, 1) ad_kernel(AdArgs args) {
  static_assert(!(F & C2F_VJP), "C2F_VJP is C2F_NOLIN to nl_column: the fused kernel has no vector-Jacobian form");
  C2_KERNEL_BODY(C2_WAVE_LOG_BEGIN);
  C2_KERNEL_BODY((nl_column<(F & ~C2F_ASSIGN) | C2F_CKPT>(global_column(), &kernarg<AdArgs>()->nl)));
  C2_KERNEL_BODY((ad_reverse_column<F>(global_column(), kernarg<AdArgs>())));
  C2_KERNEL_BODY(C2_WAVE_LOG_END);
}
// the reverse sweep alone, also as the vector-Jacobian product (C2F_VJP); with C2F_SATLIN the vector-Jacobian form with SATUR
// differentiated in the sweep -- ASSIGN | VJP, without QSAT: PRECISE x EVAP x OFF32
constexpr bool ad_reverse_variant_valid(unsigned f) {
  return (f & C2F_SATLIN) ? (f & ~(C2F_PRECISE | C2F_EVAP | C2F_OFF32)) == (C2F_SATLIN | C2F_ASSIGN | C2F_VJP)
                          : (!(f & C2F_ADNORM) || ((f & C2F_ASSIGN) && !(f & C2F_EVAP))) && (!(f & C2F_VJP) || ((f & C2F_ASSIGN) && !(f & C2F_ADNORM)));
}
constexpr bool ad_variant_valid(unsigned f) { return !(f & C2F_ADNORM); }  // both sweeps of CLOUDSC2AD

// The parameter forms (C2F_PARLIN; units tl_par, vjp_par): the same columns over the larger argument blocks, under their parents' launch
// bounds: CLOUDSC2TL with the tangents of the four tunable parameters, the vector-Jacobian form of the reverse sweep with their adjoints.
template <unsigned F>
__global__ void __launch_bounds__(kBlock, tl_waves_per_simd(F)) tl_par_kernel(TlParArgs args) {
  C2_KERNEL_BODY((tl_column<F>(global_column(), &kernarg<TlParArgs>()->a)));
}
template <unsigned F>
__global__ void __launch_bounds__(kBlock, 1) vjp_par_kernel(AdParArgs args) {
  C2_KERNEL_BODY((ad_reverse_column<F>(global_column(), &kernarg<AdParArgs>()->a)));
}
// their flag words: PARLIN with QSAT or with SATLIN (the reverse sweep: | ASSIGN | VJP), times PRECISE, EVAP, OFF32
constexpr bool par_variant_valid(unsigned f, unsigned form) {
  const unsigned rest = f & ~(C2F_PRECISE | C2F_EVAP | C2F_OFF32);
  return rest == (C2F_PARLIN | form | C2F_QSAT) || rest == (C2F_PARLIN | form | C2F_SATLIN);
}
constexpr bool tl_par_variant_valid(unsigned f) { return par_variant_valid(f, 0u); }
constexpr bool vjp_par_variant_valid(unsigned f) { return par_variant_valid(f, C2F_ASSIGN | C2F_VJP); }

// The sparse forms (C2F_SPARSE; units tl_sparse, vjp_sparse): the same columns over the argument blocks with the two plane masks, under
// their twins' launch bounds: the TL sweep without trajectory stores that reads and writes only the tangent planes of the launch's masks,
// the vector-Jacobian form of the reverse sweep that reads only the cotangent and writes only the gradient planes of them; qsat is a plane
// or SATUR is differentiated in the sweep.  Their variant word is the twin's without the bits every one of them has
// (SPARSE; the reverse sweep: ASSIGN | VJP too): QSAT or SATLIN, times PRECISE, EVAP, OFF32 -- 16 kernels per family and precision.  Not
// sweep families: no family number, no launch-log entry; launched directly, like parnormal_kernel.
template <unsigned F>
__global__ void __launch_bounds__(kBlock, tl_waves_per_simd(F)) tl_sparse_kernel(TlSparseArgs args) {
  C2_KERNEL_BODY((tl_column<F | C2F_SPARSE>(global_column(), &kernarg<TlSparseArgs>()->a)));
}
template <unsigned F>
__global__ void __launch_bounds__(kBlock, 1) vjp_sparse_kernel(AdSparseArgs args) {
  C2_KERNEL_BODY((ad_reverse_column<F | C2F_ASSIGN | C2F_VJP | C2F_SPARSE>(global_column(), &kernarg<AdSparseArgs>()->a)));
}
constexpr bool sparse_variant_valid(unsigned f) {
  const unsigned rest = f & ~(C2F_PRECISE | C2F_EVAP | C2F_OFF32);
  return rest == C2F_QSAT || rest == C2F_SATLIN;
}

// The column-sum forms (C2F_COLSUM; units {nl,tl,vjp}_colsum): the same columns over the argument blocks that carry the weight table and
// the sums -- no output, tangent or cotangent plane but the per-column weighted level sums (the reverse sweep: weight x the cotangent of
// the column's sum) -- under their twins' launch bounds (NL: nl_kernel's, TL / reverse sweep: the sparse kernels').  Variant words:
// NL: QSAT (or SATUR in the sweep), PRECISE, EVAP, OFF32, and CKPT for the form that keeps PFPLSL5 / PFPLSN5 and the cover checkpoint --
// 32 kernels per precision; TL / reverse sweep: the sparse forms' words, 16 each.  Not sweep families: no family number, no launch-log
// entry; launched directly, like the sparse kernels.
static_assert(kColsumLanes == kBlock, "one LDS slot per lane of the workgroup and sum");
template <unsigned F>
__global__ void __launch_bounds__(kBlock, nl_waves_per_simd(F)) nl_colsum_kernel(NlColsumArgs args) {
  C2_KERNEL_BODY((nl_column<F | C2F_COLSUM>(global_column(), &kernarg<NlColsumArgs>()->a)));
}
template <unsigned F>
__global__ void __launch_bounds__(kBlock, tl_waves_per_simd(F)) tl_colsum_kernel(TlColsumArgs args) {
  C2_KERNEL_BODY((tl_column<F | C2F_SPARSE | C2F_COLSUM>(global_column(), &kernarg<TlColsumArgs>()->a.a)));
}
template <unsigned F>
__global__ void __launch_bounds__(kBlock, 1) vjp_colsum_kernel(AdColsumArgs args) {
  C2_KERNEL_BODY((ad_reverse_column<F | C2F_ASSIGN | C2F_VJP | C2F_SPARSE | C2F_COLSUM>(global_column(), &kernarg<AdColsumArgs>()->a.a)));
}
constexpr bool nl_colsum_variant_valid(unsigned f) { return (f & ~(C2F_QSAT | C2F_PRECISE | C2F_EVAP | C2F_CKPT | C2F_OFF32)) == 0; }

// The ensemble forms (units {nl,tl,vjp}_ens): the same columns again, under their parents' launch bounds, over an
// argument block that lives in device memory -- one per member, written by ens_args_kernel (cloudsc2_launch.hip) in the launch before.
// The block's address comes from blockIdx and the kernel arguments alone (ens_locate), so it is workgroup-uniform and the constants
// are scalar loads as before: through the scalar cache from memory instead of from the kernel-argument segment.  Not sweep families:
// no family number, no pacing (fair = 0, pace_* = 0 in every block), no launch-log entry; launched directly, like parnormal_kernel.
template <class Args>
struct EnsArgs {
  const Args* blocks;        // [members]
  unsigned wgs_per_member;   // ceil(ncols_pad / kBlock)
};
typedef EnsArgs<NlArgs> NlEnsArgs;
typedef EnsArgs<TlParArgs> TlEnsArgs;
typedef EnsArgs<AdParArgs> VjpEnsArgs;
#if defined(__HIP_DEVICE_COMPILE__)
template <class Args>
__device__ __forceinline__ const C2_CONST_AS Args* ens_block(const C2_CONST_AS EnsArgs<Args>* e, long long& column) {
  unsigned member;
  ens_locate(blockIdx.x, e->wgs_per_member, threadIdx.x, blockDim.x, member, column);
  return (const C2_CONST_AS Args*)(e->blocks + member);
}
#endif
template <unsigned F>
__global__ void __launch_bounds__(kBlock, nl_waves_per_simd(F)) nl_ens_kernel(NlEnsArgs args) {
#if defined(__HIP_DEVICE_COMPILE__)
  long long column;
  const C2_CONST_AS NlArgs* a = ens_block(kernarg<NlEnsArgs>(), column);
  nl_column<F>(column, a);
#endif
}
template <unsigned F>
__global__ void __launch_bounds__(kBlock, tl_waves_per_simd(F)) tl_ens_kernel(TlEnsArgs args) {
#if defined(__HIP_DEVICE_COMPILE__)
  long long column;
  const C2_CONST_AS TlParArgs* a = ens_block(kernarg<TlEnsArgs>(), column);
  tl_column<F>(column, &a->a);
#endif
}
template <unsigned F>
__global__ void __launch_bounds__(kBlock, 1) vjp_ens_kernel(VjpEnsArgs args) {
#if defined(__HIP_DEVICE_COMPILE__)
  long long column;
  const C2_CONST_AS AdParArgs* a = ens_block(kernarg<VjpEnsArgs>(), column);
  ad_reverse_column<F>(column, &a->a);
#endif
}
// the NL words cloudsc2_ad_launch_forward can produce: QSAT, PRECISE, OFF32 free, the cover checkpoint exactly with the evaporation branch
constexpr bool nl_ens_variant_valid(unsigned f) {
  return (f & ~(C2F_QSAT | C2F_PRECISE | C2F_EVAP | C2F_CKPT | C2F_OFF32)) == 0 && ((f & C2F_CKPT) != 0) == ((f & C2F_EVAP) != 0);
}

// The column sums of an ensemble's members (C2F_MEMBER; units {nl,tl,vjp}_ens_colsum): the column-sum sweeps over member
// blocks in device memory, under their twins' launch bounds and with their twins' variant words (NL: nl_colsum_kernel's, TL / reverse
// sweep: the sparse forms').  The TL and the reverse sweep carry the parameter derivative (C2F_PARLIN).  Not sweep families: no family
// number, no pacing, no launch-log entry.  The NL family has a locate function of its own (ens_colsum_locate).
typedef EnsArgs<NlColsumArgs> NlEnsColsumArgs;
typedef EnsArgs<TlEnsColsumArgs> TlEnsColsumKArgs;
typedef EnsArgs<AdEnsColsumArgs> VjpEnsColsumKArgs;
template <unsigned F>
__global__ void __launch_bounds__(kBlock, nl_waves_per_simd(F)) nl_ens_colsum_kernel(NlEnsColsumArgs args) {
#if defined(__HIP_DEVICE_COMPILE__)
  const C2_CONST_AS NlEnsColsumArgs* e = kernarg<NlEnsColsumArgs>();
  unsigned member;
  long long column;
  ens_colsum_locate(blockIdx.x, e->wgs_per_member, gridDim.x, threadIdx.x, blockDim.x, member, column);
  nl_column<F | C2F_COLSUM | C2F_MEMBER>(column, &((const C2_CONST_AS NlColsumArgs*)(e->blocks + member))->a);
#endif
}
template <unsigned F>
__global__ void __launch_bounds__(kBlock, tl_waves_per_simd(F)) tl_ens_colsum_kernel(TlEnsColsumKArgs args) {
#if defined(__HIP_DEVICE_COMPILE__)
  long long column;
  const C2_CONST_AS TlEnsColsumArgs* a = ens_block(kernarg<TlEnsColsumKArgs>(), column);
  tl_column<F | C2F_PARLIN | C2F_SPARSE | C2F_COLSUM | C2F_MEMBER>(column, &a->a.a.a);
#endif
}
template <unsigned F>
__global__ void __launch_bounds__(kBlock, 1) vjp_ens_colsum_kernel(VjpEnsColsumKArgs args) {
#if defined(__HIP_DEVICE_COMPILE__)
  long long column;
  const C2_CONST_AS AdEnsColsumArgs* a = ens_block(kernarg<VjpEnsColsumKArgs>(), column);
  ad_reverse_column<F | C2F_ASSIGN | C2F_VJP | C2F_PARLIN | C2F_SPARSE | C2F_COLSUM>(column, &a->a.a.a);
#endif
}
// fp32 only.  With level_ad carrying the parameter sums, the fp32 device build packs and contracts the level of the sparse reverse sweep
// differently, and the field gradients of vjp_ens_colsum_kernel miss the column-sum twin's bits by up to two units in the last place
// (measured on the MI355X; its parameter adjoints are the parameter form's bits, and the fp64 build holds both).  So the fp32 launcher
// runs this kernel after it when a field gradient is wanted: the twin's own column function, ad_reverse_column without PARLIN, over the
// same member blocks (an AdEnsColsumArgs begins with the twin's AdColsumArgs), which stores the twin's bits over the planes.  The fp32
// reverse sweep of an ensemble's column sums therefore runs twice unless only the parameter adjoints are wanted.
template <unsigned F>
__global__ void __launch_bounds__(kBlock, 1) vjp_ens_colsum_fields_kernel(VjpEnsColsumKArgs args) {
#if defined(__HIP_DEVICE_COMPILE__)
  long long column;
  const C2_CONST_AS AdEnsColsumArgs* a = ens_block(kernarg<VjpEnsColsumKArgs>(), column);
  ad_reverse_column<F | C2F_ASSIGN | C2F_VJP | C2F_SPARSE | C2F_COLSUM>(column, &a->a.a.a);
#endif
}
constexpr bool kEnsColsumFieldsPass = sizeof(real_t) == 4;
constexpr bool vjp_ens_colsum_fields_variant_valid(unsigned f) { return kEnsColsumFieldsPass && sparse_variant_valid(f); }

// The batched TL and reverse sweeps (tl_batch_column, vjp_batch_column: up to kBatchMax directions over one trajectory).  One wave
// per SIMD in fp64 like their single-direction twins, whose registers they extend by the carries of the further directions and one
// more set of direction inputs; the fp32 builds take what they need (nothing is measured for them yet).
// (their variant word: G = F + 64 x directions of the launch, a compile-time count -- cloudsc2_column.hpp says why)
template <unsigned G>
__global__ void __launch_bounds__(kBlock, 1) tl_batch_kernel(TlBatchArgs args) {
  C2_KERNEL_BODY((tl_batch_column<G % 64u, (int)(G / 64u)>(global_column(), kernarg<TlBatchArgs>())));
}
template <unsigned G>
__global__ void __launch_bounds__(kBlock, 1) vjp_batch_kernel(VjpBatchArgs args) {
  C2_KERNEL_BODY((vjp_batch_column<G % 64u, (int)(G / 64u)>(global_column(), kernarg<VjpBatchArgs>())));
}
// the flag words of the batched sweeps: C2F_QSAT always, times PRECISE, EVAP, OFF32 (8 flag words per family and precision, times
// the direction counts 2..kBatchMax)
constexpr bool batch_variant_valid(unsigned f) {
  return (f & C2F_QSAT) != 0 && (f & ~(C2F_QSAT | C2F_PRECISE | C2F_EVAP | C2F_OFF32)) == 0;
}
constexpr bool batch_kernel_valid(unsigned g) {  // (one direction is tl_kernel's / ad_reverse_kernel's)
  return batch_variant_valid(g % 64u) && g / 64u >= 2u && g / 64u <= (unsigned)kBatchMax;
}

// The parameter Jacobian in one sweep (tl_parjac_column; unit tl_parjac): the batched TL sweep's structure and launch
// bounds, the direction count (3, or 4 with the evaporation branch) fixed by the flag word.  Flag words: PRECISE, EVAP, OFF32 times
// QSAT or SATUR evaluated in the sweep -- 16 kernels per precision.
template <unsigned F>
__global__ void __launch_bounds__(kBlock, 1) tl_parjac_kernel(TlParJacArgs args) {
  C2_KERNEL_BODY((tl_parjac_column<F>(global_column(), kernarg<TlParJacArgs>())));
}
constexpr bool parjac_variant_valid(unsigned f) { return (f & ~(C2F_QSAT | C2F_PRECISE | C2F_EVAP | C2F_OFF32)) == 0; }

// The normal equations of the parameters in one sweep (parnormal_column; unit parnormal): tl_parjac_kernel's launch
// bounds.  Flag words: QSAT, PRECISE, EVAP -- 8 kernels per precision, 64-bit offsets.  Not a sweep family: it has no family number, is
// not paced and is not in the launch log; cloudsc2_parnormal_launch launches it directly, like the fold that follows it.
template <unsigned F>
__global__ void __launch_bounds__(kBlock, 1) parnormal_kernel(ParNormalArgs args) {
  C2_KERNEL_BODY((parnormal_column<F>(global_column(), kernarg<ParNormalArgs>())));
}
constexpr bool parnormal_variant_valid(unsigned) { return true; }  // (every word of its table of 8)

// The parameter Jacobian and the normal equations of the column sums in one sweep (parcolsum_column; unit parcolsum):
// tl_parjac_kernel's launch bounds; the 32 KiB of LDS a 128-lane workgroup takes for its accumulators let two workgroups share a CU,
// which is what one wave per SIMD asks for.  Flag words: QSAT, PRECISE, EVAP, OFF32 times the two ends of the column (C2F_NORMAL) --
// 32 kernels per precision.  Not a sweep family: no family number, no pacing, no launch-log entry; launched directly, like
// parnormal_kernel.
template <unsigned F>
__global__ void __launch_bounds__(kBlock, 1) parcolsum_kernel(ParColsumArgs args) {
  C2_KERNEL_BODY((parcolsum_column<F>(global_column(), kernarg<ParColsumArgs>())));
}
constexpr bool parcolsum_variant_valid(unsigned f) { return (f & ~(C2F_QSAT | C2F_PRECISE | C2F_EVAP | C2F_OFF32 | C2F_NORMAL)) == 0; }

// The ten perturbed NL runs of the Taylor test in one sweep, the lambdas on the lanes (taylor_column): the grid is over THREADS,
// 64 per kTaylorCols columns.  A wave reads 6 columns = 48 bytes of every 128-byte line it touches, so two or three consecutive
// waves share each line -- the one sweep whose workgroups share data.  Blocks are dealt round-robin over the 8 XCDs (b and b + 8
// share one, each XCD with its own L2): consecutive LOGICAL blocks are therefore mapped to physical blocks 8 apart, so that the
// waves sharing a line sit on one XCD and its L2 fetches the line once (the grid is a multiple of 8 blocks; logical blocks past the
// end find no column and leave).  Measured (rocprofv3 --pmc FETCH_SIZE, 160 000 columns): see profiles/r03_taylor_sweep_ab.txt.
template <unsigned F>
__global__ void __launch_bounds__(kBlock) taylor_kernel(TaylorArgs args) {
#if defined(__HIP_DEVICE_COMPILE__)
  const unsigned per_xcd = gridDim.x >> 3;
  const long long block = (long long)(blockIdx.x & 7u) * per_xcd + (blockIdx.x >> 3);
  taylor_column<F>(block * blockDim.x + threadIdx.x, kernarg<TaylorArgs>());
#endif
}
constexpr bool taylor_variant_valid(unsigned f) { return !(f & (C2F_PERT | C2F_CKPT)); }

// ---------------------------------------------------------------------------------------------------------
// THE table of the variant tables: one row per table, the rows of one unit under C2_ROWS_<unit>.  A row is
//   X(name, Args, slots, valid, family, kernel, paced)
//     name    the accessor is name_variant(word), the kernel template name_kernel<word>
//     Args    the kernel's argument block
//     slots   words 0 .. slots-1; the batched tables' word is flags + 64 x directions, as in the launch log
//     valid   constexpr bool valid(word): the kernel is built (defined next to its kernel above)
//   and, for the host's registry (cloudsc2_policy.hip; the names are cloudsc2_host.hpp's and the C header's):
//     family  the number of cloudsc2_variant_built and the launch log (kFamNl ..), or kNone: not a sweep family, launched unlogged
//     kernel  the number of cloudsc2_kernel_occupancy (kFamNl .. kFamTlParjac, CLOUDSC2_KERNEL_*), or kNone
//     paced   device_prepare probes the pacing rule at every occupancy this table's kernels have
// A unit is compiled from cloudsc2_kern.hip with -DC2_FAMILY=<unit>; its name is also in the Makefile's FAMILIES, which
// tests/test_kernel_families.py holds to this table.  A new table is a row here (in a new or an existing unit); a new unit is also a line
// in C2_KERNEL_TABLES and a name in FAMILIES.
// ---------------------------------------------------------------------------------------------------------
#define C2_ROWS_nl(X) X(nl, NlArgs, 128, nl_variant_valid, kFamNl, kFamNl, false)
#define C2_ROWS_tl(X) X(tl, TlArgs, 256, tl_variant_valid, kFamTl, kFamTl, true)
#define C2_ROWS_ad(X)                                                                               \
  X(ad_reverse, AdArgs, 256, ad_reverse_variant_valid, kFamAdReverse, kFamAdReverse, true)          \
  X(ad, AdArgs, 64, ad_variant_valid, kFamAd, kFamAd, true)
#define C2_ROWS_taylor(X) X(taylor, TaylorArgs, 64, taylor_variant_valid, kFamTaylor, kNone, false)
#define C2_ROWS_tl_batch(X) X(tl_batch, TlBatchArgs, 64 * (kBatchMax + 1), batch_kernel_valid, kFamTlBatch, kFamTlBatch, true)
#define C2_ROWS_vjp_batch(X) X(vjp_batch, VjpBatchArgs, 64 * (kBatchMax + 1), batch_kernel_valid, kFamVjpBatch, kFamVjpBatch, true)
// (paced at launch, yet not probed: paced where a probed table's kernel has the same occupancy -- DESIGN.md 3, the table of variant tables)
#define C2_ROWS_tl_par(X) X(tl_par, TlParArgs, 512, tl_par_variant_valid, kFamTlPar, kNone, false)
#define C2_ROWS_vjp_par(X) X(vjp_par, AdParArgs, 512, vjp_par_variant_valid, kFamVjpPar, kNone, false)
#define C2_ROWS_tl_parjac(X) X(tl_parjac, TlParJacArgs, 64, parjac_variant_valid, kFamTlParjac, kFamTlParjac, true)
#define C2_ROWS_parnormal(X) X(parnormal, ParNormalArgs, 8, parnormal_variant_valid, kNone, kNone, false)
#define C2_ROWS_parcolsum(X) X(parcolsum, ParColsumArgs, 64, parcolsum_variant_valid, kNone, kNone, false)
#define C2_ROWS_nl_ens(X) X(nl_ens, NlEnsArgs, 64, nl_ens_variant_valid, kNone, kNone, false)
#define C2_ROWS_tl_ens(X) X(tl_ens, TlEnsArgs, 512, tl_par_variant_valid, kNone, kNone, false)
#define C2_ROWS_vjp_ens(X) X(vjp_ens, VjpEnsArgs, 512, vjp_par_variant_valid, kNone, kNone, false)
#define C2_ROWS_tl_sparse(X) X(tl_sparse, TlSparseArgs, 256, sparse_variant_valid, kNone, CLOUDSC2_KERNEL_TL_SPARSE, true)
#define C2_ROWS_vjp_sparse(X) X(vjp_sparse, AdSparseArgs, 256, sparse_variant_valid, kNone, CLOUDSC2_KERNEL_VJP_SPARSE, true)
#define C2_ROWS_nl_colsum(X) X(nl_colsum, NlColsumArgs, 64, nl_colsum_variant_valid, kNone, CLOUDSC2_KERNEL_NL_COLSUM, false)
#define C2_ROWS_tl_colsum(X) X(tl_colsum, TlColsumArgs, 256, sparse_variant_valid, kNone, CLOUDSC2_KERNEL_TL_COLSUM, true)
#define C2_ROWS_vjp_colsum(X) X(vjp_colsum, AdColsumArgs, 256, sparse_variant_valid, kNone, CLOUDSC2_KERNEL_VJP_COLSUM, true)
#define C2_ROWS_nl_ens_colsum(X) X(nl_ens_colsum, NlEnsColsumArgs, 64, nl_colsum_variant_valid, kNone, kNone, false)
#define C2_ROWS_tl_ens_colsum(X) X(tl_ens_colsum, TlEnsColsumKArgs, 256, sparse_variant_valid, kNone, kNone, false)
// (the second table: the fp32 library's pass that stores the field gradients in the column-sum twin's bits; empty in fp64)
#define C2_ROWS_vjp_ens_colsum(X)                                                                                     \
  X(vjp_ens_colsum, VjpEnsColsumKArgs, 256, sparse_variant_valid, kNone, kNone, false)                                \
  X(vjp_ens_colsum_fields, VjpEnsColsumKArgs, 256, vjp_ens_colsum_fields_variant_valid, kNone, kNone, false)
#define C2_KERNEL_TABLES(X)                                                                                           \
  C2_ROWS_nl(X) C2_ROWS_tl(X) C2_ROWS_ad(X) C2_ROWS_taylor(X) C2_ROWS_tl_batch(X) C2_ROWS_vjp_batch(X) C2_ROWS_tl_par(X) \
  C2_ROWS_vjp_par(X) C2_ROWS_tl_parjac(X) C2_ROWS_parnormal(X) C2_ROWS_parcolsum(X) C2_ROWS_nl_ens(X) C2_ROWS_tl_ens(X) \
  C2_ROWS_vjp_ens(X) C2_ROWS_tl_sparse(X) C2_ROWS_vjp_sparse(X) C2_ROWS_nl_colsum(X) C2_ROWS_tl_colsum(X)             \
  C2_ROWS_vjp_colsum(X) C2_ROWS_nl_ens_colsum(X) C2_ROWS_tl_ens_colsum(X) C2_ROWS_vjp_ens_colsum(X)

// The accessors: name_variant(word) is name_kernel<word>, or nullptr for a word past the table's slots or one that is not built.
template <class Args> using KernelFn = void (*)(Args);
#define C2_DECLARE_VARIANT(name, Args, slots, valid, family, kernel, paced) KernelFn<Args> name##_variant(unsigned word);
C2_KERNEL_TABLES(C2_DECLARE_VARIANT)
#undef C2_DECLARE_VARIANT

// A row's definitions, inside namespace cloudsc2: the table (name_kernel<F> for every valid F, indexed by F, which instantiates those
// kernels in this code object) and its accessor.  Expanded by cloudsc2_kern.hip for its unit's rows, and by cloudsc2_launch.hip for every
// row under -DC2_SINGLE_TU.
#define C2_DEFINE_VARIANT(name, Args, slots, valid, family, kernel, paced)                                          \
  namespace {                                                                                                         \
  template <unsigned F> constexpr KernelFn<Args> name##_entry() {                                                     \
    if constexpr (valid(F)) return name##_kernel<F>; else return nullptr;                                             \
  }                                                                                                                   \
  template <unsigned... F> constexpr std::array<KernelFn<Args>, sizeof...(F)> name##_make(                            \
      std::integer_sequence<unsigned, F...>) { return {{name##_entry<F>()...}}; }                                     \
  const std::array<KernelFn<Args>, slots> g_##name##_kernels = name##_make(std::make_integer_sequence<unsigned, slots>{}); \
  }                                                                                                                   \
  KernelFn<Args> name##_variant(unsigned word) { return word < g_##name##_kernels.size() ? g_##name##_kernels[word] : nullptr; }

}  // namespace cloudsc2
