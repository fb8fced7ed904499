// cloudsc2_host.hpp -- what the host units of libcloudsc2_hip share (internal: not part of the C ABI, not installed).
//
//   cloudsc2_launch.hip   the C ABI launchers (sweeps, SATUR, expand / validate, Taylor sums and sweep, adjoint norms), the error
//                         state, the math mode, the level-table cache, the argument checks, and the small kernels they launch
//   cloudsc2_policy.hip   launch policy: the device probes, device_prepare and its verdicts, the occupancy lookup, the pacing rule,
//                         and the fair / nap / pacing decision of every launch (schedule)
//   cloudsc2_alloc.hip    the placement allocator behind cloudsc2_device_malloc*
//   cloudsc2_driver.hip   the host-array drivers and the resident state
//   cloudsc2_helpers.hip  host-only helpers of the C ABI (default parameters, offsets, validation text, the synthetic table, verdicts)
//   cloudsc2_parmap.hip   per-column parameter maps: cloudsc2_{nl,tl,vjp}_launch_parmap and their kernels (no family: see below)
//
// The sweeps' kernels are in the family units, cloudsc2_kern.hip compiled once per name of the Makefile's FAMILIES; the table of
// cloudsc2_sweep_kernels.hpp (C2_ROWS_<unit>) says which variant tables each holds and how the host numbers them.  Any other __global__
// kernel stays in the unit that launches it: without relocatable device code a kernel cannot be launched by name from another unit's code object.  Everything
// here has external linkage inside namespace cloudsc2; the link's version script (cloudsc2_hip.map) keeps it out of the dynamic symbol
// table, where only the C ABI appears.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <functional>
#include <initializer_list>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/cloudsc2_hip.h"
#include "cloudsc2_sweep_kernels.hpp"
#include "cloudsc2_fields.hpp"  // the field table: resolve_in / resolve_out, writable, outputs_given, ncols_pad

namespace cloudsc2 {

// ---- error state (cloudsc2_launch.hip) ---------------------------------------------------------------------------------------------
extern thread_local std::string g_err;  // cloudsc2_last_error()
int fail(int code, const char* msg);  // (declared by cloudsc2_fields.hpp too, which is built without this header by its test)

#define HIP_TRY(expr)                                                                     \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess) {                                                               \
      g_err = std::string(#expr) + ": " + hipGetErrorString(e_);                          \
      return (int)e_;                                                                     \
    }                                                                                     \
  } while (0)

bool device_ok();
int no_device();  // CLOUDSC2_ENODEVICE, with its message
inline int require_device() { return device_ok() ? 0 : no_device(); }

// ---- argument checks and launch helpers (cloudsc2_launch.hip) -----------------------------------------------------------------------
bool precise_of(const cloudsc2_params* prm);  // the arithmetic of one call: its own request, else the process default
int check_geom(const cloudsc2_params* prm, int nproma, int nlev, int ngptot, Geom& g);
int get_tables(const cloudsc2_params& p, const LevelTab** dev, int* kb0, int* kb1);
int validate_launch_impl(const cloudsc2_real* table, int klon, int period, long long start, int nlevx, int ndim, int nproma,
                         long long ngptot, cloudsc2_field field, double* workspace, double* stats, void* stream, long long ncols_minmax);

// the part of check_geom that needs no device (a launcher that refuses its whole call before it looks for one)
int check_geom_args(const cloudsc2_params* prm, int nproma, int nlev, int ngptot);
void fill_geom(Geom& g, int nproma, int nlev, int ngptot);  // what check_geom leaves in g (fair = 0, no pacing)
// refusals several launchers share (each entry point keeps its own order of them)
int check_satur(int satur);
int require_qsat(int satur, const cloudsc2_inputs* traj_in);

inline unsigned grid_for(long long ncols, int block) { return (unsigned)((ncols + block - 1) / block); }

// The start every sweep launcher shares: check (the geometry; `missing`: the message for a NULL argument block) -> resolve (the
// trajectory's inputs and outputs; a launcher resolves its own further blocks after these) -> tables -> constants -> common flags.
struct Sweep {
  Geom g;
  Strides s = {0, 0, 0, 0, 0};
  InPtrs in;
  OutPtrs out;
  const LevelTab* tab = nullptr;
  Consts c;
  unsigned f = 0;

  int begin(const cloudsc2_params* prm, int nproma, int nlev, int ngptot, const char* missing) {
    const int rc = check_geom(prm, nproma, nlev, ngptot, g);
    return rc ? rc : missing ? fail(CLOUDSC2_EINVAL, missing) : 0;
  }
  int trajectory(const cloudsc2_inputs& ti, const cloudsc2_outputs& to, bool out_required) {
    const int rc = resolve_in(ti, false, s, in);
    return rc ? rc : resolve_out(to, out_required, s, out);
  }
  // C2F_QSAT, C2F_PRECISE, C2F_EVAP, and C2F_OFF32 (32-bit byte offsets) when every buffer the sweep touches -- the trajectory's and
  // those of the `more` strides -- is smaller than 4 GiB
  int finish(const cloudsc2_params& prm, double ptsphy, bool qsat, std::initializer_list<long long> more) {
    if (int rc = get_tables(prm, &tab, &g.kb0, &g.kb1)) return rc;
    c = make_consts(prm, ptsphy);
    if (qsat) f |= C2F_QSAT;
    if (precise_of(&prm)) f |= C2F_PRECISE;
    if (c.evap) f |= C2F_EVAP;
    static const bool allow32 = !(getenv("CLOUDSC2_OFF32") && atoi(getenv("CLOUDSC2_OFF32")) == 0);  // 0: measurements only
    long long stride = std::max({s.full, s.half, s.cml, s.clv, s.loc});
    for (long long x : more) stride = std::max(stride, x);
    const long long span = stride * (g.ncols_pad / g.nproma) + (long long)g.nproma * (g.nlev + 2);
    if (allow32 && span * (long long)sizeof(real_t) < (1LL << 32)) f |= C2F_OFF32;
    return 0;
  }
  // the NL sweep's argument block (no zero plane, no perturbation, no checkpoint)
  NlArgs nl() const {
    NlArgs a;
    a.c = c; a.g = g; a.s = s; a.in = in; a.out = out; a.tab = tab;
    a.zero_plane = nullptr; a.zero_stride = 0; a.lam = 0.0; a.ckpt = nullptr;
    return a;
  }
};

// The ten numbered kernel families of the sweeps, as cloudsc2_variant_built and the launch log number them; cloudsc2_kernel_occupancy
// knows the first seven under the same numbers and five unnumbered tables as CLOUDSC2_KERNEL_* (10..14).  The rows of the table in
// cloudsc2_sweep_kernels.hpp name these in their `family` and `kernel` columns (kNone: no number); the registry of cloudsc2_policy.hip
// asserts that the rows' family numbers are exactly 0 .. kFamCount-1.
enum SweepFamily {
  kFamNl = 0, kFamTl = 1, kFamAd = 2, kFamAdReverse = 3, kFamTlBatch = 4, kFamVjpBatch = 5, kFamTlParjac = 6, kFamTlPar = 7,
  kFamVjpPar = 8, kFamTaylor = 9, kFamCount = 10
};
constexpr int kNone = -1;
// the variant's entry point (nullptr: not built, or no such family); a walk of the registry (cloudsc2_policy.hip)
const void* variant_entry(int family, unsigned word);
// The calling thread's launch log (cloudsc2_debug_launch_log): a thread-local array of plain integers, no device call -- harmless
// during stream capture.  Every launch of a numbered family passes launch_variant, which records the kernel it has enqueued.
void log_launch(int family, unsigned word);

// THE launch of a sweep kernel: `workgroups` of kBlock threads over the one by-value argument block.  The unnumbered tables' launchers
// call it directly (nothing is logged for them), the numbered families' through launch_variant.
template <class Args>
int launch_kernel(KernelFn<Args> fn, const Args& args, unsigned workgroups, hipStream_t st) {
  if (!fn) return fail(CLOUDSC2_EINVAL, "kernel variant not built");
  Args a = args;
  void* argv[] = {&a};
  HIP_TRY(hipLaunchKernel((const void*)fn, dim3(workgroups), dim3(kBlock), argv, 0, st));
  return 0;
}
template <class Args>
int launch_variant(SweepFamily family, unsigned word, KernelFn<Args> fn, const Args& args, long long ncols, hipStream_t st) {
  if (int rc = launch_kernel(fn, args, grid_for(ncols, kBlock), st)) return rc;
  log_launch(family, word);
  return 0;
}

// ---- launch policy (cloudsc2_policy.hip) --------------------------------------------------------------------------------------------
// The scheduling fields of one launch's Geom (fair, pace_slots, pace_first, pace_recip_q16), set from nothing but the launch's size, the
// kernels' occupancy and the cached device verdicts (it never touches the device):
//   fair  the kernel whose waves keep abreast when the launch is one round of them (nullptr: fair = 0),
//   nap   the lighter SIMDs of the fullest CUs may nap on top of that (the NL sweep's own launches),
//   pace  the kernel whose launch of a few partial rounds of workgroups is paced (nullptr: not paced).
void schedule(Geom& g, const void* fair, bool nap, const void* pace);
// A launch over tl_column with flag word f: the fp32 variants that run three waves per SIMD (tl_waves_per_simd) share their SIMDs like
// the NL kernel does: -3.7 % at 160 000 columns with the waves kept abreast; the fp64 TL and both adjoints run one wave per SIMD and
// lose 1-5 % (profiles/r03_wave_times.txt); they are paced instead.
inline void schedule_tl(Geom& g, unsigned f, const void* fn) {
  const bool abreast = tl_waves_per_simd(f) == 3;
  schedule(g, abreast ? fn : nullptr, false, abreast ? nullptr : fn);
}
int device_prepare();  // the synchronous moment: probes the current device once per process, caches the verdicts

// ---- placement allocator (cloudsc2_alloc.hip) ---------------------------------------------------------------------------------------
bool device_is_shared();  // do other processes use this device at the same time?  (read once per process)
// the caller's own sweep, which the placement search times on every candidate (a pass over the buffer on the null stream)
using ProbeFn = std::function<void(void* base, size_t bytes)>;
// kPlaceSearch: the search (resident states, cloudsc2_device_malloc*); kPlaceOnRequest: one plain hipMalloc unless CLOUDSC2_PLACE=1
// (the host-array drivers' workspace); kPlacePlain: never searched (staging buffers)
enum PlacePolicy { kPlaceSearch = 0, kPlaceOnRequest = 1, kPlacePlain = 2 };
int device_malloc_impl(void** out, size_t bytes, const ProbeFn* custom = nullptr, PlacePolicy policy = kPlaceSearch);
int device_free_impl(void* p);

}  // namespace cloudsc2
