// cloudsc2_sweep_kernels.hpp -- the __global__ wrappers of the column sweeps (NL, TL, AD, the Taylor test's lambda sweep), their
// compile-time variant tables and what they share.  The sweeps are built as one translation unit per kernel family so that an edit to
// one sweep does not rebuild every variant table (448 slots, ~70 s as one unit): cloudsc2_kern_<family>.hip for every name of the Makefile's FAMILIES, each of which
// instantiates its table and exports it through one accessor (nl_variant(F) ...); the host units are listed in cloudsc2_host.hpp.
// -DC2_SINGLE_TU puts the sweeps and their launchers into ONE code object again (cloudsc2_launch.hip then includes the family files):
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
template <unsigned F>
__global__ void __launch_bounds__(kBlock, (F & C2F_EVAP) ? 1 : 3) nl_kernel(NlArgs args) {
  C2_KERNEL_BODY(C2_WAVE_LOG_BEGIN);
  C2_KERNEL_BODY((nl_column<F>(global_column(), kernarg<NlArgs>())));
  C2_KERNEL_BODY(C2_WAVE_LOG_END);
}

// fp32 only: the TL variants with 32-bit offsets and without the evaporation branch need 173 VGPRs; held to 168 (3 waves
// per SIMD) they spill at most 7 dwords, and all 2500 waves of a 160 000-column launch are resident at once instead of
// 2048 + 452 (0.94 -> 0.88 ms).  Every other TL variant, and the fp64 ones, spill heavily below what they ask for.
template <unsigned F>
__global__ void __launch_bounds__(kBlock, (sizeof(real_t) == 4 && (F & C2F_OFF32) && !(F & C2F_EVAP)) ? 3 : 1)
tl_kernel(TlArgs args) {
  C2_KERNEL_BODY(C2_WAVE_LOG_BEGIN);
  C2_KERNEL_BODY((tl_column<F>(global_column(), kernarg<TlArgs>())));
  C2_KERNEL_BODY(C2_WAVE_LOG_END);
}

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

// The parameter forms (C2F_PARLIN; units cloudsc2_kern_tl_par.hip, cloudsc2_kern_vjp_par.hip): the same columns over the larger argument
// blocks, under their parents' launch bounds.
template <unsigned F>
__global__ void __launch_bounds__(kBlock, (sizeof(real_t) == 4 && (F & C2F_OFF32) && !(F & C2F_EVAP)) ? 3 : 1)
tl_par_kernel(TlParArgs args) {
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

// The sparse forms (C2F_SPARSE; units cloudsc2_kern_tl_sparse.hip, cloudsc2_kern_vjp_sparse.hip): the same columns over the argument blocks
// with the two plane masks, under their twins' launch bounds.  Their variant word is the twin's without the bits every one of them has
// (SPARSE; the reverse sweep: ASSIGN | VJP too): QSAT or SATLIN, times PRECISE, EVAP, OFF32 -- 16 kernels per family and precision.  Not
// sweep families: no family number, no launch-log entry; launched directly, like parnormal_kernel.
template <unsigned F>
__global__ void __launch_bounds__(kBlock, (sizeof(real_t) == 4 && (F & C2F_OFF32) && !(F & C2F_EVAP)) ? 3 : 1)
tl_sparse_kernel(TlSparseArgs args) {
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

// The column-sum forms (C2F_COLSUM; units cloudsc2_kern_{nl,tl,vjp}_colsum.hip): the same columns over the argument blocks that carry the
// weight table and the sums, under their twins' launch bounds (NL: nl_kernel's, TL / reverse sweep: the sparse kernels').  Variant words:
// NL: QSAT (or SATUR in the sweep), PRECISE, EVAP, OFF32, and CKPT for the form that keeps PFPLSL5 / PFPLSN5 and the cover checkpoint --
// 32 kernels per precision; TL / reverse sweep: the sparse forms' words, 16 each.  Not sweep families: no family number, no launch-log
// entry; launched directly, like the sparse kernels.
static_assert(kColsumLanes == kBlock, "one LDS slot per lane of the workgroup and sum");
template <unsigned F>
__global__ void __launch_bounds__(kBlock, (F & C2F_EVAP) ? 1 : 3) nl_colsum_kernel(NlColsumArgs args) {
  C2_KERNEL_BODY((nl_column<F | C2F_COLSUM>(global_column(), &kernarg<NlColsumArgs>()->a)));
}
template <unsigned F>
__global__ void __launch_bounds__(kBlock, (sizeof(real_t) == 4 && (F & C2F_OFF32) && !(F & C2F_EVAP)) ? 3 : 1)
tl_colsum_kernel(TlColsumArgs args) {
  C2_KERNEL_BODY((tl_column<F | C2F_SPARSE | C2F_COLSUM>(global_column(), &kernarg<TlColsumArgs>()->a.a)));
}
template <unsigned F>
__global__ void __launch_bounds__(kBlock, 1) vjp_colsum_kernel(AdColsumArgs args) {
  C2_KERNEL_BODY((ad_reverse_column<F | C2F_ASSIGN | C2F_VJP | C2F_SPARSE | C2F_COLSUM>(global_column(), &kernarg<AdColsumArgs>()->a.a)));
}
constexpr bool nl_colsum_variant_valid(unsigned f) { return (f & ~(C2F_QSAT | C2F_PRECISE | C2F_EVAP | C2F_CKPT | C2F_OFF32)) == 0; }

// The ensemble forms (units cloudsc2_kern_{nl,tl,vjp}_ens.hip): the same columns again, under their parents' launch bounds, over an
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
__global__ void __launch_bounds__(kBlock, (F & C2F_EVAP) ? 1 : 3) nl_ens_kernel(NlEnsArgs args) {
#if defined(__HIP_DEVICE_COMPILE__)
  long long column;
  const C2_CONST_AS NlArgs* a = ens_block(kernarg<NlEnsArgs>(), column);
  nl_column<F>(column, a);
#endif
}
template <unsigned F>
__global__ void __launch_bounds__(kBlock, (sizeof(real_t) == 4 && (F & C2F_OFF32) && !(F & C2F_EVAP)) ? 3 : 1)
tl_ens_kernel(TlEnsArgs args) {
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

// The column sums of an ensemble's members (C2F_MEMBER; units cloudsc2_kern_{nl,tl,vjp}_ens_colsum.hip): the column-sum sweeps over member
// blocks in device memory, under their twins' launch bounds and with their twins' variant words (NL: nl_colsum_kernel's, TL / reverse
// sweep: the sparse forms').  The TL and the reverse sweep carry the parameter derivative (C2F_PARLIN).  Not sweep families: no family
// number, no pacing, no launch-log entry.  The NL family has a locate function of its own (ens_colsum_locate).
typedef EnsArgs<NlColsumArgs> NlEnsColsumArgs;
typedef EnsArgs<TlEnsColsumArgs> TlEnsColsumKArgs;
typedef EnsArgs<AdEnsColsumArgs> VjpEnsColsumKArgs;
template <unsigned F>
__global__ void __launch_bounds__(kBlock, (F & C2F_EVAP) ? 1 : 3) nl_ens_colsum_kernel(NlEnsColsumArgs args) {
#if defined(__HIP_DEVICE_COMPILE__)
  const C2_CONST_AS NlEnsColsumArgs* e = kernarg<NlEnsColsumArgs>();
  unsigned member;
  long long column;
  ens_colsum_locate(blockIdx.x, e->wgs_per_member, gridDim.x, threadIdx.x, blockDim.x, member, column);
  nl_column<F | C2F_COLSUM | C2F_MEMBER>(column, &((const C2_CONST_AS NlColsumArgs*)(e->blocks + member))->a);
#endif
}
template <unsigned F>
__global__ void __launch_bounds__(kBlock, (sizeof(real_t) == 4 && (F & C2F_OFF32) && !(F & C2F_EVAP)) ? 3 : 1)
tl_ens_colsum_kernel(TlEnsColsumKArgs args) {
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

// The parameter Jacobian in one sweep (tl_parjac_column; unit cloudsc2_kern_tl_parjac.hip): the batched TL sweep's structure and launch
// bounds, the direction count (3, or 4 with the evaporation branch) fixed by the flag word.  Flag words: PRECISE, EVAP, OFF32 times
// QSAT or SATUR evaluated in the sweep -- 16 kernels per precision.
template <unsigned F>
__global__ void __launch_bounds__(kBlock, 1) tl_parjac_kernel(TlParJacArgs args) {
  C2_KERNEL_BODY((tl_parjac_column<F>(global_column(), kernarg<TlParJacArgs>())));
}
constexpr bool parjac_variant_valid(unsigned f) { return (f & ~(C2F_QSAT | C2F_PRECISE | C2F_EVAP | C2F_OFF32)) == 0; }

// The normal equations of the parameters in one sweep (parnormal_column; unit cloudsc2_kern_parnormal.hip): tl_parjac_kernel's launch
// bounds.  Flag words: QSAT, PRECISE, EVAP -- 8 kernels per precision, 64-bit offsets.  Not a sweep family: it has no family number, is
// not paced and is not in the launch log; cloudsc2_parnormal_launch launches it directly, like the fold that follows it.
template <unsigned F>
__global__ void __launch_bounds__(kBlock, 1) parnormal_kernel(ParNormalArgs args) {
  C2_KERNEL_BODY((parnormal_column<F>(global_column(), kernarg<ParNormalArgs>())));
}

// The parameter Jacobian and the normal equations of the column sums in one sweep (parcolsum_column; unit cloudsc2_kern_parcolsum.hip):
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

// Variant tables: kernel<F> for every valid flag combination F, indexed by F (see C2F_* in cloudsc2_column.hpp).
template <class Args> using KernelFn = void (*)(Args);
#define C2_VARIANT_TABLE(table, kern, Args, NF, valid_expr)                                                        \
  template <unsigned F> constexpr KernelFn<Args> table##_entry() {                                                 \
    if constexpr (valid_expr) return kern<F>; else return nullptr;                                                 \
  }                                                                                                                \
  template <unsigned... F> constexpr std::array<KernelFn<Args>, sizeof...(F)> table##_make(                        \
      std::integer_sequence<unsigned, F...>) { return {{table##_entry<F>()...}}; }                                 \
  [[maybe_unused]] const std::array<KernelFn<Args>, NF> table = table##_make(std::make_integer_sequence<unsigned, NF>{});
// (the trajectory pass differs from the plain NL sweep only with the evaporation branch: the cover checkpoint)

// the variant tables live in the family units; F past a table's size or a combination that is not built: nullptr
KernelFn<NlArgs> nl_variant(unsigned f);
KernelFn<TlArgs> tl_variant(unsigned f);
KernelFn<AdArgs> ad_variant(unsigned f);
KernelFn<AdArgs> ad_reverse_variant(unsigned f);
KernelFn<TaylorArgs> taylor_variant(unsigned f);
KernelFn<TlParArgs> tl_par_variant(unsigned f);
KernelFn<AdParArgs> vjp_par_variant(unsigned f);
KernelFn<TlBatchArgs> tl_batch_variant(unsigned f, int directions);
KernelFn<VjpBatchArgs> vjp_batch_variant(unsigned f, int directions);
KernelFn<TlParJacArgs> tl_parjac_variant(unsigned f);
KernelFn<ParNormalArgs> parnormal_variant(unsigned f);
KernelFn<ParColsumArgs> parcolsum_variant(unsigned f);
KernelFn<NlEnsArgs> nl_ens_variant(unsigned f);
KernelFn<TlEnsArgs> tl_ens_variant(unsigned f);
KernelFn<VjpEnsArgs> vjp_ens_variant(unsigned f);
KernelFn<TlSparseArgs> tl_sparse_variant(unsigned f);
KernelFn<AdSparseArgs> vjp_sparse_variant(unsigned f);
KernelFn<NlColsumArgs> nl_colsum_variant(unsigned f);
KernelFn<TlColsumArgs> tl_colsum_variant(unsigned f);
KernelFn<AdColsumArgs> vjp_colsum_variant(unsigned f);
KernelFn<NlEnsColsumArgs> nl_ens_colsum_variant(unsigned f);
KernelFn<TlEnsColsumKArgs> tl_ens_colsum_variant(unsigned f);
KernelFn<VjpEnsColsumKArgs> vjp_ens_colsum_variant(unsigned f);
KernelFn<VjpEnsColsumKArgs> vjp_ens_colsum_fields_variant(unsigned f);  // (built in the fp32 library only: kEnsColsumFieldsPass)

}  // namespace cloudsc2
