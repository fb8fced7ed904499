/*
 * cloudsc2_hip.h -- C ABI of the MI355X-native CLOUDSC2 NL / TL / AD column-physics engine.
 *
 * This is the drop-in boundary for the hot path of ecmwf-ifs/dwarf-p-cloudsc2-tl-ad.  The reference has
 * no FFI layer; its de-facto boundary is the three driver procedures and the F77-style kernels they call
 * (SURVEY.md 8b).  Every entry point below cites the reference interface it replaces (paths relative to
 * the reference checkout).  All arrays are `cloudsc2_real` = JPRB (src/common/module/parkind1.F90:40-44): fp64 in
 * libcloudsc2_hip.so, fp32 in libcloudsc2_hip_sp.so (this header compiled with -DCLOUDSC2_SINGLE, the reference's
 * -DSINGLE; same entry points, cloudsc2_real_bytes() tells the two apart).  Constants, time step, test statistics and
 * norms are `double` in both.  Layout: the reference's NPROMA-blocked one, column index fastest:
 *
 *     field(NPROMA, NLEV or NLEV+1, NBLOCKS)         f[jl + NPROMA*(jk + NLEVx*ibl)]
 *     B_CML / B_LOC (NPROMA, NLEV, 8, NBLOCKS)       planes T=0, A=1, Q=2, CLD(QL,QI,QR,QS,QV)=3..7
 *                                                    (src/common/module/cloudsc2_array_state_mod.F90:129-151)
 *     PCLV (NPROMA, NLEV, 5, NBLOCKS)                planes QL=0, QI=1 used (yoecldp.F90:86-91)
 *
 * No torch types, no C++ types: plain pointers and sizes.  Return value 0 = OK, otherwise a negative
 * CLOUDSC2_E* code or a positive hipError_t; cloudsc2_last_error() gives the text.  The library has NO CPU
 * fallback: without a HIP device every launch/run entry point fails with CLOUDSC2_ENODEVICE.
 */
#ifndef CLOUDSC2_HIP_H
#define CLOUDSC2_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#ifdef CLOUDSC2_SINGLE
typedef float cloudsc2_real;
#else
typedef double cloudsc2_real;
#endif

#define CLOUDSC2_MAX_NLEV 200 /* the reference's own limit, src/cloudsc2_nl/dwarf_cloudsc.F90:87 */

#define CLOUDSC2_EINVAL    (-1)
#define CLOUDSC2_ENODEVICE (-2)
#define CLOUDSC2_ETLWRONG  (-3) /* "TL is totally wrong" STOP of cloudsc_driver_tl_mod.F90:247-249 */

/* Constants and switches the reference keeps in modules and loads from input.h5:
 * YOMCST (yomcst.F90:167-177), YOETHF (yoethf.F90:79-99), YOECLDP (yoecldp.F90:247-250,...),
 * YOEPHLI (yoephli.F90:79-97), YOECLD%CETA (dwarf_cloudsc.F90:100-102), YRPHNC%LEVAPLS2 (:105),
 * YRNCL%LREGCL (src/cloudsc2_tl/dwarf_cloudsc.F90:105), LDRAIN1D (cloudsc_driver_mod.F90:61).
 * The first 30 doubles are also the order oracle/ref_harness.F90 takes them in. */
typedef struct cloudsc2_params {
  double rg, rd, rcpd, retv, rlvtt, rlstt, rlmlt, rtt;                         /* YOMCST  */
  double r2es, r3les, r3ies, r4les, r4ies, r5les, r5ies, r5alvcp, r5alscp,     /* YOETHF  */
         ralvdcp, ralsdcp, rtwat, rtice, rtwat_rtice_r, rvtmp2;
  double rclcrit, rkconv, rlmin, rpecons;                                      /* YOECLDP */
  double rlptrc;                                                               /* YOEPHLI */
  double rticecu, rtwat_rticecu_r;                                             /* YOETHF, dead branches only */
  int lphylin;   /* YREPHLI%LPHYLIN: 1 in every reference main (dwarf_cloudsc.F90:107).  0 selects the FOEALFA / FOEEWM form of the NL
                  * sweep's saturation pressure (cloudsc2.F90:349,365-369; unless ldrain1d); CLOUDSC2TL / CLOUDSC2AD and the driver's
                  * SATUR call (cloudsc_driver_mod.F90:91: LDPHYLIN=.TRUE.) do not depend on it: cloudsc2_tl_launch* and
                  * cloudsc2_ad_launch* IGNORE this field and run the LPHYLIN form, as the reference's TL / AD do
                  * (cloudsc2tl.F90 / cloudsc2ad.F90 have no other); cloudsc2_nl_launch with pert_lambda != 0 (a perturbed run of
                  * the Taylor test) refuses lphylin = 0 with CLOUDSC2_EINVAL */
  int levapls2;  /* precipitation evaporation on/off (LEVAPLS2 .OR. LDRAIN1D, cloudsc2.F90:557) */
  int lregcl;    /* TL/AD regularisation (cloudsc2tl.F90:575,657,754,794,998) */
  int ldrain1d;
  int nlev;
  int math_mode; /* arithmetic of THIS call: 0 = the process default (cloudsc2_set_math_mode), 1 = fast, 2 = precise */
  double ceta[CLOUDSC2_MAX_NLEV];
} cloudsc2_params;

/* Fill *p with the standard IFS constants and the reference mains' switches; nlev and ceta
 * are left for the caller (ceta(jk) = PAP(1,jk,1)/PAPH(1,nlev+1,1), dwarf_cloudsc.F90:100-102). */
void cloudsc2_params_default(cloudsc2_params* p);

const char* cloudsc2_last_error(void);
/* 1 if a HIP device is usable by this process, else 0. */
int cloudsc2_device_available(void);
/* ordinal of the calling thread's current HIP device (what the Fortran timing table prints where the reference's prints the
 * core a thread ran on, timer_mod.F90:97,159-162); 0 when there is no device */
int cloudsc2_current_device(void);
/* sizeof(cloudsc2_real) of THIS build of the library: 8, or 4 for the -DCLOUDSC2_SINGLE build. */
int cloudsc2_real_bytes(void);

/* Arithmetic of the kernels.  Every call carries its own mode in cloudsc2_params.math_mode (1 fast, 2 precise); 0 there
 * means the process default set here (initial value from the environment variable CLOUDSC2_MATH=fast|precise).  The
 * default is only READ by the launchers, never changed by the library, so concurrent calls do not influence each other.
 *   fast (default): quotients on shared / batch-inverted v_rcp_f64 reciprocals refined by one third-order step, a
 *     branch-free exp, tanh from one exp -- a few ulp from the correctly rounded values;
 *   precise: the reference's own operation order with IEEE division and libm exp/tanh/cosh.
 * cloudsc2_tl_taylor_run evaluates in precise mode unless params.math_mode asks for fast explicitly: its verdict is
 * decided by round-off noise (the fast-mode verdict is recorded by tests/test_gpu_parity.py). */
void cloudsc2_set_math_mode(int precise);
int cloudsc2_get_math_mode(void);

/* Device memory for callers that keep the state resident (and what the library uses for its own buffers).
 * On MI355X write streams run 10-20 % slower into some parts of the HBM than into others, whatever the access pattern
 * (profiles/r02_hbm_placement.md): 0.81 vs 0.96 ms for the NL kernel at 160 000 columns, decided by where the OUTPUT arrays
 * happen to lie.  This allocator places what it hands out: for a request of 256 MiB or more it makes candidate hipMalloc
 * allocations of the full size -- enough of them to span 96 GiB together (12 to 64, never more than fit 60 % of the free memory;
 * 85 % for requests above 12 GiB) -- times two probe streams over each (the sweeps' write stream and the NL sweep's whole
 * read/write pattern), keeps the best and frees the others (about 10 ms per candidate, once per allocation).
 * The mixed stream reads the first 59 % of the buffer and writes the last 41 %: put what your sweeps WRITE at the end of the
 * buffer (a sweep that wrote at 23-39 % of a buffer placed this way ran at 5.0 instead of 5.8 TB/s).
 * Allocate a state -- inputs AND outputs -- as ONE request (an arena): that is what was measured to land in
 * the fast class 8 times of 8, whereas placing only the written arrays and leaving the inputs elsewhere does not (0.88-0.93 ms;
 * profiles/r02_placement/z_one_arena_vs_split.txt).  The pointer is ordinary hipMalloc memory of the current device; free it with
 * cloudsc2_device_free.  cloudsc2_device_malloc_info reports the last placement: number of
 * candidates and the probe time of the best, the median and the worst of them (0 when there was no choice).
 * There is no reference counterpart: the reference's arrays are host ALLOCATABLEs (cloudsc2_array_state_mod.F90:97-151). */
#include <stddef.h>
int cloudsc2_device_malloc(void** ptr, size_t bytes);
void cloudsc2_device_malloc_info(int* candidates, double* best_ms, double* median_ms, double* worst_ms);
/* Who is searched.  cloudsc2_device_malloc, cloudsc2_device_malloc_state and the resident states (cloudsc2_state_create and the
 * scratch of their self-tests): yes.  The workspace of the HOST-ARRAY drivers cloudsc2_nl_run / cloudsc2_tl_taylor_run /
 * cloudsc2_ad_symmetry_run: one plain hipMalloc -- those calls are PCIe-bound (55-71 ms per 160 000 columns against a 0.1 ms
 * difference of the kernel), and a host model's free HBM is not taken transiently on their behalf; CLOUDSC2_PLACE=1 in the
 * environment asks for the search there too.  Staging buffers of re-blocked transfers and the validator's workspace: never.
 * CLOUDSC2_PLACE=0 switches every search off.  The counters say how many allocations of this process were searched (more than
 * one candidate) and how many were plain. */
void cloudsc2_device_malloc_counts(long long* searched, long long* plain);
int cloudsc2_device_free(void* ptr);
/* The same for a buffer that will hold a state of (nproma, nlev, ngptot) at its start (and whatever the caller keeps behind it:
 * perturbation sets, scratch): the placement search times the NL kernel itself on a zero-filled state laid out in every candidate
 * -- read-only arrays first (PT PQ PAP PLU PLUDE PMFU PMFD PSUPSAT PAPH B_CML PCLV), then what the sweeps write (PA PCOVPTOT QSAT
 * PFPLSL PFPLSN PFHPSL PFHPSN B_LOC), each 256-byte aligned, the layout cloudsc2_state_* uses -- instead of the two generic probe
 * streams, which stop predicting the kernel at 1 M columns (profiles/r02_placement/r_1m_probe_vs_kernel.txt).  When more than
 * 256 MiB follow the state the two generic streams over the whole buffer judge instead (a buffer's speed is a property of the
 * whole, and the NL sweep sees only its first part).  `bytes` must cover the state; the buffer comes back zero-filled only by
 * accident, clear what you need.  Free with cloudsc2_device_free. */
int cloudsc2_device_malloc_state(void** ptr, size_t bytes, int nproma, int nlev, int ngptot);
/* Diagnostic: times one of the allocator's probe streams over [ptr, ptr+bytes) and OVERWRITES it.  kind 0: the sweeps' write
 * stream (what the placement search uses); kind 1: the NL sweep's whole pattern -- 16 planes read, 11 written per level, the
 * buffer taken as 27 planes.  *ms = median of `rounds` launches after one warm-up (tools/probe_vs_kernel.py). */
int cloudsc2_device_probe(void* ptr, size_t bytes, int kind, int rounds, double* ms);

/* ------------------------------------------------------------------------------------------------
 * Kernel level: DEVICE pointers, asynchronous on `stream` (a hipStream_t, NULL = default stream).
 * One field = base pointer + stride between NPROMA blocks (in elements); level stride is NPROMA,
 * column stride 1.  A (NPROMA,NLEV,NBLOCKS) array has block_stride NPROMA*NLEV; plane p of B_CML has
 * ptr = b_cml + p*NPROMA*NLEV and block_stride 8*NPROMA*NLEV.
 * ------------------------------------------------------------------------------------------------ */
typedef struct cloudsc2_field {
  cloudsc2_real* ptr;
  long long block_stride;
} cloudsc2_field;

/* The 16 inputs of CLOUDSC2 in the dummy-argument order of src/cloudsc2_nl/cloudsc2.F90:13-16:
 * PAPHP1(NLEV+1) PAPP1 PQM1 PQS PTM1 PL PI PLUDE PLU PMFU PMFD PGTENT PGTENQ PGTENL PGTENI PSUPSAT. */
typedef struct cloudsc2_inputs {
  cloudsc2_field paph, pap, q, qsat, t, l, i, lude, lu, mfu, mfd, gtent, gtenq, gtenl, gteni, supsat;
} cloudsc2_inputs;

/* The 10 outputs (cloudsc2.F90:15-18): PTENT PTENQ PTENL PTENI PCLC PFPLSL PFPLSN PFHPSL PFHPSN
 * (fluxes NLEV+1) PCOVPTOT. */
typedef struct cloudsc2_outputs {
  cloudsc2_field tent, tenq, tenl, teni, clc, fplsl, fplsn, fhpsl, fhpsn, covptot;
} cloudsc2_outputs;

/* SATUR + CLOUDSC2 for all blocks: replaces the body of the block loop of
 * src/cloudsc2_nl/cloudsc_driver_mod.F90:82-111 (SATUR call :91, CLOUDSC2 call :94-107).
 * in->qsat.ptr == NULL  => PQS is computed in-kernel from PAP,PT (SATUR fused, satur.F90:106-123);
 * in->qsat.ptr != NULL  => PQS is read (the TL/AD test drivers perturb it independently).
 * zero_plane (optional, may have ptr NULL): an extra (NPROMA,NLEV) plane per block that is zero-filled,
 * i.e. TENDENCY_LOC(IBL)%cld(:,:,NCLV)=0 of cloudsc_driver_mod.F90:88.
 * pert_lambda != 0: every input x is replaced on load by x + pert_lambda*(0.01*x), the perturbed state
 * of the Taylor test (cloudsc_driver_tl_mod.F90:156-171,200-215); with fused SATUR, PQS is perturbed the
 * same way after SATUR on the unperturbed PAP,PT (:159,:203).
 * Asynchronous on `stream`, always: no launcher of this library allocates, copies or synchronises on behalf of the launch
 * heuristics below -- they only read what cloudsc2_device_prepare cached.  (The one thing a launcher may create is the device copy
 * of the per-level table of a CETA it sees for the first time: a 3 KB allocation and a copy through a private non-blocking stream,
 * with the thread's capture mode relaxed; a launch on a stream that is ITSELF being captured needs that table to exist already --
 * any earlier launch or driver call with the same CETA made it.) */
int cloudsc2_nl_launch(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot,
                       const cloudsc2_inputs* in, const cloudsc2_outputs* out, cloudsc2_field zero_plane,
                       double pert_lambda, void* stream);

/* SATUR only (satur.F90:106-123, LDPHYLIN branch): qsat(NPROMA,NLEV,NBLOCKS) from pap, t. */
int cloudsc2_satur_launch(const cloudsc2_params* prm, int nproma, int nlev, int ngptot,
                          cloudsc2_field pap, cloudsc2_field t, cloudsc2_field qsat, void* stream);

/* SATUR and its two partial derivatives (satur.F90:106-123, LDPHYLIN branch, differentiated as written; the reference ships no
 * SATURTL / SATURAD, so these are this library's own derivative code): dqs_dpap, dqs_dt (NPROMA,NLEV,NBLOCKS) receive d(qsat)/d(pap)
 * and d(qsat)/d(t), qsat the bits of cloudsc2_satur_launch (qsat.ptr may be NULL: partials only).  Where the ZQMAX clamp acts
 * (foeew/pap > 0.5) both partials are exactly 0; at the kinks (t == RTICE, t == RTWAT, foeew/pap == 0.5) they take the one-sided
 * value of the formulas in cloudsc2_level.hpp (satur_lin_point).  All planes share one block stride; padded tail columns are not
 * written.  Asynchronous, no allocation, no synchronisation. */
int cloudsc2_satur_lin_launch(const cloudsc2_params* prm, int nproma, int nlev, int ngptot,
                              cloudsc2_field pap, cloudsc2_field t, cloudsc2_field qsat,
                              cloudsc2_field dqs_dpap, cloudsc2_field dqs_dt, void* stream);

/* CLOUDSC2TL (src/cloudsc2_tl/cloudsc2tl.F90:10-24): trajectory in -> trajectory out (give all ten traj_out
 * fields, or all NULL to skip the trajectory stores), perturbation in -> perturbation out.  traj_in->qsat NULL => fused
 * SATUR for PQS5.  pert_in must give all 16 fields.
 * Launch pacing (TL and AD sweeps; results unaffected): these kernels run one wave per SIMD, so a launch is a number of rounds of
 * workgroups on the device's slots; when it is two to eight whole rounds plus a partial one that fills at most half of the slots
 * (160 000 columns on MI355X: 1250 workgroups on 512 slots), the workgroups whose slot has one workgroup less to run nap at every
 * level for 1/k of the level's measured time, leaving their share of the bandwidth to the slots on the critical path: TL -5 %, AD
 * -7 % at 160 000 columns (profiles/r04_pacing_ab.txt) -- on a device whose dispatcher cloudsc2_device_prepare
 * (below) has seen to be in-order and slot-stable, which is what the rule rests on.  CLOUDSC2_PACE=0 in the environment switches it off,
 * CLOUDSC2_PACE_VERBOSE=1 reports paced launches on stderr.  cloudsc2_pace_plan is the rule itself (pure arithmetic, no device):
 * for `workgroups` (of 128 threads) on `slots` workgroup slots it returns 1 when the launch would be paced, with the number of whole
 * rounds, the number of leading positions of every round that form the fast class, and 65536 / k (the nap as a share of a level). */
int cloudsc2_pace_plan(long long workgroups, long long slots, int* whole_rounds, int* fast_first, int* nap_recip_q16);
/* The NL sweep's counterpart for launches that are ONE round of waves (all resident at once; 160 000 columns on MI355X): inside the
 * CUs that carry the most workgroups, the waves on SIMDs with fewer waves than the CU's fullest SIMD nap 15 % of every level
 * (CLOUDSC2_NL_LIGHT=percent, 0 = off): -2 % at 160 000 columns, results unaffected.  How many waves share a SIMD follows from the
 * block index alone; cloudsc2_simd_population is that rule (pure arithmetic, no device): for wave `wave_in_block` (0 or 1) of block
 * `block` of a launch of `workgroups` 128-thread blocks on `cus` CUs, *mine = waves of the launch on its SIMD, *most = on the fullest
 * SIMD of its CU.  tools/wave_times.py checks it against the hardware's own record (HW_ID) wave by wave. */
int cloudsc2_simd_population(long long workgroups, int cus, long long block, int wave_in_block, int* mine, int* most);
/* The library takes neither rule on trust, and checks neither from a launch.  cloudsc2_device_prepare is the one SYNCHRONOUS moment:
 * on the calling thread's current device, once per device and process (later calls return at once), it runs
 *   - the dispatch probe of the NL rule: a 40 us launch of the NL kernel's shape whose waves record where they run (HW_ID); the
 *     rule is checked wave by wave, one miss -- another dispatcher, other work on the device at that moment -- and the lighter
 *     SIMDs' nap stays off for the device;
 *   - the pace probe of the TL / AD rule, for every occupancy (workgroups per CU) a TL / AD kernel of this build has: a 130 us launch
 *     of 2.44 rounds of workgroups that do nothing but stay as long as their class would (fast 40 us; napping 60 us) and record
 *     where and when they ran; per CU the workgroups it ran must be (k+1) of the fast class per fast workgroup of its first round
 *     and k of the slow class per slow one, and the whole first round must have been resident at once.  One miss -- a dispatcher
 *     that is not in-order and slot-stable, CU masking, another partition mode's queueing -- and TL / AD launches are not paced.
 * Each probe: one small allocation, two launches on a private non-blocking stream, one copy back, with the thread's stream-capture
 * mode relaxed meanwhile (a graph capture going on elsewhere in the process is not disturbed); a probe that ends in a HIP error
 * leaves no verdict and is repeated by the next call.  The library calls it from every entry point that allocates device memory
 * (cloudsc2_device_malloc*, cloudsc2_state_create, the host-array drivers' workspace), so callers of those never need to.  A caller
 * that brings its OWN device memory to the kernel-level entry points and wants the naps calls cloudsc2_device_prepare once at
 * start-up; without it every launch simply runs unpaced (results are the same bits either way).  CLOUDSC2_PACE_VERBOSE=1 prints
 * the verdicts.  cloudsc2_dispatch_probe / cloudsc2_pace_probe run one probe and return its counts without caching anything (GPU
 * tests); cloudsc2_device_rules returns the cached verdicts of the current device (1 on, 0 off, -1 never probed);
 * cloudsc2_kernel_occupancy the workgroups per CU of one kernel variant (kernel 0 NL, 1 TL, 2 AD both sweeps, 3 AD reverse sweep,
 * 4 batched TL, 5 batched reverse sweep, 6 the parameter Jacobian's sweep; flags = its C2F_* variant bits, cloudsc2_column.hpp; for the batched sweeps, whose kernels
 * are built per direction count, plus 64 x the directions of the launch, 2..cloudsc2_batch_max()) as the runtime reports them
 * (the sweeps of cloudsc2_tl_launch_satur / cloudsc2_vjp_launch_satur: kernel 1 / 3 with C2F_SATLIN = 128 among the flags).
 * Kernels 10..14 are the CLOUDSC2_KERNEL_* numbers below (sparse and column-sum sweeps); 7, 8, 9 and anything else are refused.
 * The numbering is one column of the table of variant tables in csrc/cloudsc2_sweep_kernels.hpp.
 *
 * What a caller with its own hipMalloc should expect.  The same kernel on the same data runs 0.78 or 0.92 ms (NL, 160 000 columns:
 * 0.73 vs 0.63 of the HBM peak) depending on WHERE in the HBM the state lies (profiles/r02_hbm_placement.md); cloudsc2_device_malloc*
 * search for a good place, a plain first hipMalloc of a process typically lands on a slow one (bench line:
 * roofline.unplaced_first_allocation).  A host model that allocates its own state gets the kernels' full rate by taking that one
 * allocation from cloudsc2_device_malloc_state (ordinary hipMalloc memory, freed with cloudsc2_device_free), or by allocating
 * candidates itself and keeping the one cloudsc2_device_probe times fastest. */
int cloudsc2_device_prepare(void);
int cloudsc2_dispatch_probe(long long* waves_checked, long long* waves_wrong);
int cloudsc2_pace_probe(int workgroups_per_cu, long long* workgroups_checked, long long* workgroups_wrong);
int cloudsc2_device_rules(int workgroups_per_cu, int* nl_nap, int* pacing);
int cloudsc2_kernel_occupancy(int kernel, int flags, int* workgroups_per_cu);
int cloudsc2_tl_launch(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot,
                       const cloudsc2_inputs* traj_in, const cloudsc2_outputs* traj_out,
                       const cloudsc2_inputs* pert_in, const cloudsc2_outputs* pert_out, void* stream);

/* CLOUDSC2TL with the increments of the reference's two test drivers, dx = 0.01*x for every input
 * (cloudsc_driver_tl_mod.F90:156-171; cloudsc_driver_ad_mod.F90:124-139, where ZSUPSAT = 0): they are formed from the
 * trajectory inputs the sweep reads anyway, so no increment arrays exist (17.5 KB per column less to read, and nothing to
 * fill first).  supsat_increment: the factor of the PSUPSAT increment (0.01 Taylor test, 0 adjoint test).
 * yy: NULL, or NBLOCKS*NPROMA device doubles receiving <y,y> of each active column's TL outputs -- the adjoint test's norm1
 * (cloudsc_driver_ad_mod.F90:184-195), formed while the outputs are in registers. */
int cloudsc2_tl_launch_self(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot,
                            const cloudsc2_inputs* traj_in, const cloudsc2_outputs* traj_out, double supsat_increment,
                            const cloudsc2_outputs* pert_out, double* yy, void* stream);

/* CLOUDSC2AD (src/cloudsc2_ad/cloudsc2ad.F90:10-24): trajectory in -> trajectory out; adj_out holds the
 * output adjoints on entry and is zeroed on return (:917-919,955-966,1173,1572,1678-1691); adj_in is
 * accumulated (+=, :1723-1738) except PSUPSAT which is assigned PTSPHY*zqp1 exactly as the reference does
 * (:1733).  `scratch` must hold (ngptot rounded up to NPROMA blocks) * nlev elements: the precipitation-cover
 * carry checkpoints, written and re-read only when LEVAPLS2 .OR. LDRAIN1D (the evaporation branch is the carried
 * cover's one reader); otherwise it is not touched and may be NULL. */
int cloudsc2_ad_launch(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot,
                       const cloudsc2_inputs* traj_in, const cloudsc2_outputs* traj_out,
                       const cloudsc2_inputs* adj_in, const cloudsc2_outputs* adj_out,
                       cloudsc2_real* scratch, void* stream);

/* The same with the input adjoints ASSIGNED instead of accumulated: adj_in = A^T adj_out, the old contents of adj_in are
 * neither read nor required to be zero (16 planes of reads less per level).  This is what "zero the increments, then call
 * CLOUDSC2AD" (cloudsc_driver_ad_mod.F90:198-237) amounts to; cloudsc2_ad_symmetry_run uses it.  Padded tail columns of the
 * last block are not written. */
int cloudsc2_ad_launch_assign(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot,
                              const cloudsc2_inputs* traj_in, const cloudsc2_outputs* traj_out,
                              const cloudsc2_inputs* adj_in, const cloudsc2_outputs* adj_out,
                              cloudsc2_real* scratch, void* stream);

/* CLOUDSC2AD as its two sweeps.  _forward is the forward sweep (cloudsc2ad.F90:366-866): trajectory in -> trajectory out
 * (+ the cover checkpoints in `scratch` when LEVAPLS2 .OR. LDRAIN1D).  _reverse is the reverse sweep (:877-1740): it re-reads
 * the trajectory inputs, takes the rain / snow flux carried into every level from traj_out->fplsl / fplsn (PFPLSL5, PFPLSN5;
 * the other traj_out fields are not read and may be NULL) and, with the evaporation branch only, the cover from `scratch`;
 * adj_out / adj_in as for cloudsc2_ad_launch (assign != 0: as for cloudsc2_ad_launch_assign).  _forward + _reverse on one
 * stream equals cloudsc2_ad_launch bit for bit.  A caller whose PFPLSL5 / PFPLSN5 are already on the device -- any NL or TL
 * sweep over the same state wrote them, e.g. the TL leg of the adjoint test (cloudsc_driver_ad_mod.F90:160-181) -- runs
 * _reverse alone and saves the trajectory pass (28.5 KB per column of traffic). */
int cloudsc2_ad_launch_forward(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot,
                               const cloudsc2_inputs* traj_in, const cloudsc2_outputs* traj_out,
                               cloudsc2_real* scratch, void* stream);
int cloudsc2_ad_launch_reverse(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot,
                               const cloudsc2_inputs* traj_in, const cloudsc2_outputs* traj_out,
                               const cloudsc2_inputs* adj_in, const cloudsc2_outputs* adj_out,
                               const cloudsc2_real* scratch, int assign, void* stream);

/* The vector-Jacobian product of the NL sweep, for reverse-mode differentiation (the package's autograd op): the reverse sweep of
 * cloudsc2_ad_launch_reverse in the assign form, adj_in = J^T adj_out, with two differences:
 *   - adj_out is READ ONLY: the output adjoints are not zeroed (cloudsc2_ad_launch* consume them), so a caller's gradients stay
 *     as they are and need no copy;
 *   - the PSUPSAT adjoint is the true derivative zqp1, not PTSPHY*zqp1.  The reference's TL forms
 *     ZQP1 = PQM1 + PTSPHY*PGTENQ + PSUPSAT (cloudsc2tl.F90:345: coefficient 1), its AD assigns PSUPSAT = PTSPHY*ZQP1
 *     (cloudsc2ad.F90:1733); its adjoint test never sees this, its PSUPSAT increment being 0 (cloudsc_driver_ad_mod.F90:139).
 *     Every other input adjoint equals cloudsc2_ad_launch_assign's bit for bit, and fl(PTSPHY * adj_in->supsat) equals its PSUPSAT.
 * traj_out->fplsl / fplsn (PFPLSL5, PFPLSN5) are read, the other traj_out fields may be NULL.  `scratch` holds the cover checkpoints
 * cloudsc2_ad_launch_forward wrote; it is read with LEVAPLS2 .OR. LDRAIN1D only (otherwise it may be NULL).  Padded tail columns of the
 * last block are not written.  Strides, pacing and first-use behaviour are those of the other launchers: it takes one block stride
 * per layout group, and apart from the CETA table every launcher uploads on a grid's first use (see cloudsc2_nl_launch) it neither
 * allocates nor synchronises. */
int cloudsc2_vjp_launch(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot,
                        const cloudsc2_inputs* traj_in, const cloudsc2_outputs* traj_out,
                        const cloudsc2_inputs* adj_in, const cloudsc2_outputs* adj_out,
                        const cloudsc2_real* scratch, void* stream);

/* The derivative of what the drivers compute, pap, t -> SATUR -> CLOUDSC2 (cloudsc_driver_mod.F90:91), with SATUR differentiated
 * inside the sweeps (satur.F90:106-123, see cloudsc2_satur_lin_launch; CLOUDSC2TL / CLOUDSC2AD of the reference treat PQSAT as an
 * independent input and it has no SATURTL / SATURAD).  No qsat plane exists on any side: 2 planes per level less than
 * cloudsc2_tl_launch / cloudsc2_vjp_launch read and write.
 *   cloudsc2_tl_launch_satur: cloudsc2_tl_launch without trajectory stores; traj_in->qsat and pert_in->qsat must both be NULL
 *     (else CLOUDSC2_EINVAL), the other 15 fields of each are required; the tangent of qsat is dqs/dpap dpap + dqs/dt dt.
 *   cloudsc2_vjp_launch_satur: cloudsc2_vjp_launch (adj_out read only, true PSUPSAT derivative, padded tail not written);
 *     traj_in->qsat and adj_in->qsat must both be NULL; adj_in->pap and adj_in->t carry SATUR's contribution
 *     (pap += dqs/dpap qsat_adj, t += dqs/dt qsat_adj).
 * New entry points rather than a new meaning of NULL in the existing ones, where traj_in->qsat == NULL already says "fused SATUR,
 * independent qsat tangent / adjoint".  Strides, pacing, stream capture and first-use behaviour are those of the other launchers. */
int cloudsc2_tl_launch_satur(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot,
                             const cloudsc2_inputs* traj_in, const cloudsc2_inputs* pert_in, const cloudsc2_outputs* pert_out,
                             void* stream);
int cloudsc2_vjp_launch_satur(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot,
                              const cloudsc2_inputs* traj_in, const cloudsc2_outputs* traj_out,
                              const cloudsc2_inputs* adj_in, const cloudsc2_outputs* adj_out,
                              const cloudsc2_real* scratch, void* stream);

/* Sparse TL and reverse sweeps: only the planes a loss touches are moved.  The twins are cloudsc2_tl_launch (without trajectory stores)
 * / cloudsc2_vjp_launch with satur = 0, cloudsc2_tl_launch_satur / cloudsc2_vjp_launch_satur with satur = 1; here a field of the
 * derivative blocks may have a NULL ptr:
 *   pert_in   a zero tangent, not read            pert_out  a tangent not stored
 *   adj_out   a zero cotangent, not read          adj_in    a gradient not wanted, not written
 * Every plane that is present has the bits of the twin given zero planes for the absent ones (a stored -0 becomes +0 exactly as
 * there).  The trajectory stays complete: the 16 inputs (satur = 1: 15, every qsat field NULL; satur = 0: traj_in->qsat required,
 * pert_in->qsat and adj_in->qsat ordinary optional planes), PFPLSL5 / PFPLSN5 and, with LEVAPLS2 .OR. LDRAIN1D, `scratch`.  The
 * present members of one layout group share one block stride (full-level and half-level: across both derivative blocks); a group
 * with no member present needs none.  pert_in may be all NULL: the result is the zero tangent's, bit for bit the twin's.
 * CLOUDSC2_EINVAL, before the device is looked for: a NULL block, an incomplete trajectory, no plane present in pert_out, in adj_out
 * or in adj_in, different strides in one group, a written plane given twice, a qsat field with satur = 1, satur outside {0, 1},
 * prm->lphylin = 0, a missing scratch with the evaporation branch.  Neither launcher allocates or synchronises (apart from the CETA
 * table of a grid's first use); both are plain kernel nodes under stream capture; padded tail columns are not written.  New entry
 * points rather than a new meaning of NULL in the existing ones, which refuse a NULL field.  The kernels are not a kernel family of
 * cloudsc2_variant_built and do not appear in the launch log; cloudsc2_kernel_occupancy knows them as kernel
 * CLOUDSC2_KERNEL_TL_SPARSE and CLOUDSC2_KERNEL_VJP_SPARSE, flags = C2F_QSAT or C2F_SATLIN, times C2F_PRECISE, C2F_EVAP, C2F_OFF32. */
#define CLOUDSC2_KERNEL_TL_SPARSE 10
#define CLOUDSC2_KERNEL_VJP_SPARSE 11
int cloudsc2_tl_launch_sparse(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, int satur,
                              const cloudsc2_inputs* traj_in, const cloudsc2_inputs* pert_in, const cloudsc2_outputs* pert_out,
                              void* stream);
int cloudsc2_vjp_launch_sparse(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, int satur,
                               const cloudsc2_inputs* traj_in, const cloudsc2_outputs* traj_out,
                               const cloudsc2_inputs* adj_in, const cloudsc2_outputs* adj_out,
                               const cloudsc2_real* scratch, void* stream);

/* Column sums of the outputs, formed in the sweeps: y_n[c] = sum_k w_n[k] out_n[k, c] for the outputs n that are given, one number per
 * column instead of a plane.  `weights` is a device table of 10 x (nlev + 1) cloudsc2_real, row n (the order of cloudsc2_outputs) at
 * weights + n (nlev + 1), entry k of a row the weight of the plane's level index k: k = 0 .. nlev - 1 for the full-level outputs (the
 * last entry is unused), k = 0 .. nlev for the four fluxes, k = 0 the top half level.  The rows of absent sums are not read.  Weights
 * must be finite (not checked).  The blocks `sums`, `pert_sums`, `adj_sums` are cloudsc2_outputs whose fields point at
 * (nblocks, nproma) arrays; the present ones share one block_stride >= nproma; a NULL ptr means absent.  The definition, to the bit,
 * for every active column in the library's real type: acc = +0; for k = 0 .. nlevx - 1: acc = fl(acc + fl(w[k] out[k])), out the bits
 * of the dense launch's output, the product rounded before the add (no fused multiply-add).  The top half level of a flux is an exact
 * zero and contributes nothing.  Padded tail columns are not written.
 *   cloudsc2_nl_launch_colsum   the NL sweep (LPHYLIN form; in->qsat.ptr NULL: SATUR in the sweep, as in cloudsc2_nl_launch).  keep NULL:
 *                               the sums are stored and nothing else.  keep given: its fplsl and fplsn fields (both, with the stride of
 *                               in->paph; its other fields are ignored) receive PFPLSL5 / PFPLSN5 in the bits of
 *                               cloudsc2_ad_launch_forward, and with LEVAPLS2 .OR. LDRAIN1D `scratch` the cover checkpoints: what the
 *                               reverse sweep re-reads.  Without the evaporation branch scratch is not touched.
 *   cloudsc2_tl_launch_colsum   the sparse TL sweep (a NULL field of pert_in is a zero tangent, not read: the rule of
 *                               cloudsc2_tl_launch_sparse); no tangent plane is stored, pert_sums receives the sums of the output tangents.
 *   cloudsc2_vjp_launch_colsum  the sparse reverse sweep (the gradients wanted are the non-NULL fields of adj_in) in which the cotangent
 *                               of output n at level k is not loaded from a plane but formed as fl(w_n[k] ybar_n[c]) from the table and
 *                               the per-column adj_sums (read only; NULL: a zero cotangent).  Every gradient has the bits of
 *                               cloudsc2_vjp_launch_sparse given those products as planes.
 * CLOUDSC2_EINVAL, before the device is looked for: a NULL block, bad geometry, prm->lphylin = 0, a NULL table, no sum given or wanted
 * (TL: every pert_sums field NULL; reverse: every adj_sums or every adj_in field NULL), sums of different strides or a stride below
 * nproma, keep with only one of the two planes, keep with the evaporation branch and no scratch, satur outside {0, 1}, satur = 1
 * together with a qsat plane, an incomplete trajectory.  No launcher allocates or synchronises (apart from the CETA table of a grid's
 * first use); all are plain kernel nodes under stream capture.  The kernels are no kernel family of cloudsc2_variant_built and do not
 * appear in the launch log; cloudsc2_kernel_occupancy knows them as CLOUDSC2_KERNEL_{NL,TL,VJP}_COLSUM (flags: NL C2F_QSAT, C2F_PRECISE,
 * C2F_EVAP, C2F_OFF32 and C2F_CKPT = 16 for the keep form; TL / reverse: the sparse kernels' flags). */
#define CLOUDSC2_KERNEL_NL_COLSUM 12
#define CLOUDSC2_KERNEL_TL_COLSUM 13
#define CLOUDSC2_KERNEL_VJP_COLSUM 14
int cloudsc2_nl_launch_colsum(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot,
                              const cloudsc2_inputs* in, const cloudsc2_real* weights, const cloudsc2_outputs* sums,
                              const cloudsc2_outputs* keep, cloudsc2_real* scratch, void* stream);
int cloudsc2_tl_launch_colsum(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, int satur,
                              const cloudsc2_inputs* traj_in, const cloudsc2_inputs* pert_in, const cloudsc2_real* weights,
                              const cloudsc2_outputs* pert_sums, void* stream);
int cloudsc2_vjp_launch_colsum(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, int satur,
                               const cloudsc2_inputs* traj_in, const cloudsc2_outputs* traj_out, const cloudsc2_inputs* adj_in,
                               const cloudsc2_real* weights, const cloudsc2_outputs* adj_sums, const cloudsc2_real* scratch,
                               void* stream);

/* The derivative with respect to the scheme's tunable parameters, next to the derivative with respect to its fields.  Four constants
 * of cloudsc2_params enter CLOUDSC2 smoothly, in this order (CLOUDSC2_NPAR):
 *   rkconv   the autoconversion rate, ZCKCODTL = 2 RKCONV PTSPHY, ZCKCODTI = 5 RKCONV PTSPHY (cloudsc2.F90:235-236)
 *   rclcrit  the autoconversion threshold, ZLCRIT = 2 RCLCRIT; with LEVAPLS2 .OR. LDRAIN1D 1.9 RCLCRIT for liquid and the constant 1e-4 for
 *            ice, which then does not depend on it (:505-509,522-526)
 *   rlptrc   the mixed-phase fraction ZOEALFAW = 0.545 (tanh(0.17 (T - RLPTRC)) + 1) at cold points (:350)
 *   rpecons  the evaporation of precipitation, ZBETA = RG RPECONS (...)^0.5777, with LEVAPLS2 .OR. LDRAIN1D only (:566)
 * (rlmin enters a comparison only; the thermodynamic constants and ptsphy are not tunables.  None of the four enters SATUR.)  The
 * reference has no parameter derivative; this one is the library's own.  The local partials are exact derivatives of the NL sweep's
 * statements; the resulting perturbation travels down the column through the same linearisation as the field tangents.  So with
 * prm->lregcl the parameter derivative is regularised exactly where CLOUDSC2TL is (cloudsc2tl.F90:575,657,754,794,998) and is not the
 * exact derivative; with lregcl = 0 it is.  Exact zeros: clc and covptot depend on none of the four; without the evaporation branch
 * nothing depends on rpecons; with it teni does not depend on rclcrit.
 *   satur = 0: traj_in->qsat (and pert_in->qsat / adj_in->qsat) required, as for cloudsc2_tl_launch / cloudsc2_vjp_launch;
 *   satur = 1: every qsat field NULL, SATUR differentiated in the sweep, as for the _satur pair.  Any other value: CLOUDSC2_EINVAL.
 *   With the evaporation branch rpecons must not be 0 (its partial is formed as ZBETA / RPECONS): CLOUDSC2_EINVAL.
 * cloudsc2_tl_launch_par: cloudsc2_tl_launch without trajectory stores (cloudsc2_tl_launch_satur), plus the source terms of the four
 *   parameter tangents dpar (host doubles, read during the call: they travel in the kernel-argument segment like every constant).
 * cloudsc2_vjp_launch_par: cloudsc2_vjp_launch (cloudsc2_vjp_launch_satur): the field adjoints it writes are the bits the plain launcher
 *   writes.  Every active column's four sums over its levels go to `work` (device, cloudsc2_par_work_doubles() doubles, the caller's;
 *   formed in double in both builds), and a second kernel folds them in a fixed order into par_adj (device, CLOUDSC2_NPAR doubles,
 *   assigned): no floating-point atomics, the same bits from run to run.  Padded tail columns write nothing and are not summed.
 * Like every launcher they take the caller's stream and one block stride per layout group, neither allocate nor synchronise (apart from
 * the CETA table of a grid's first use), are plain kernel nodes under stream capture (one, and a pair), and are paced like their parents. */
#define CLOUDSC2_NPAR 4
int cloudsc2_par_work_doubles(int nproma, int ngptot, long long* n);
int cloudsc2_tl_launch_par(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, int satur,
                           const cloudsc2_inputs* traj_in, const cloudsc2_inputs* pert_in, const double* dpar /* [CLOUDSC2_NPAR], host */,
                           const cloudsc2_outputs* pert_out, void* stream);
int cloudsc2_vjp_launch_par(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, int satur,
                            const cloudsc2_inputs* traj_in, const cloudsc2_outputs* traj_out,
                            const cloudsc2_inputs* adj_in, const cloudsc2_outputs* adj_out /* read only */,
                            const cloudsc2_real* scratch, double* work, double* par_adj /* device, [CLOUDSC2_NPAR] */, void* stream);

/* The whole parameter Jacobian in one sweep -- what a Gauss-Newton or Levenberg-Marquardt calibration of the four parameters needs.
 * cloudsc2_tl_launch_parjac replaces one cloudsc2_tl_launch_par call per parameter, each with all-zero tangent planes and the unit
 * tangent e_k as dpar: pert_out[k] receives d out / d p_k, k in CLOUDSC2_NPAR order, and every block is the bits that call gives
 * (satur = 0).  The trajectory planes are read once, no tangent plane is read (bytes per column, NLEV 137, fp64:
 * NP x 46 080 -> 17 544 + NP x 10 992, NP = the directions run).
 *   traj_in->qsat may be NULL: SATUR is then evaluated in the sweep (none of the four enters SATUR and the field tangents are zero,
 *   so the tangent of qsat is zero either way); the other 15 fields are required.
 *   With LEVAPLS2 .OR. LDRAIN1D all four blocks are required and rpecons must not be 0 (CLOUDSC2_EINVAL).  Without the evaporation
 *   branch nothing depends on rpecons: three directions are run, and pert_out[3] is neither read nor written (its fields may be NULL).
 *   A NULL field elsewhere, prm->lphylin = 0, bad shapes, or blocks whose strides per layout group differ: CLOUDSC2_EINVAL (reported
 *   before the device is looked for).  Without a device: CLOUDSC2_ENODEVICE.  Padded tail columns are not written.
 * Like every launcher it takes the caller's stream and one block stride per layout group, neither allocates nor synchronises (apart from
 * the CETA table of a grid's first use), is one plain kernel node under stream capture, and is paced like the batched sweeps. */
int cloudsc2_tl_launch_parjac(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot,
                              const cloudsc2_inputs* traj_in, const cloudsc2_outputs* pert_out /* [CLOUDSC2_NPAR] */, void* stream);

/* The Gauss-Newton normal equations of the four parameters in one sweep.  A Gauss-Newton or Levenberg-Marquardt step needs
 * H = J^T W J (CLOUDSC2_NPAR x CLOUDSC2_NPAR) and g = J^T W r, never J = d out / d p itself: r = model - observation, W a diagonal weight,
 * the sums over every active column, level and observed output.  cloudsc2_parnormal_launch forms them without a sensitivity plane
 * ever being written: the sweep of cloudsc2_tl_launch_parjac keeps a level's sensitivities in registers, reads that level's residuals
 * and weights and sums the products per column in double (both builds); a second kernel folds the columns' sums in a fixed order
 * (that of cloudsc2_vjp_launch_par): no atomics, the same bits from run to run.  Bytes per column (NLEV 137, fp64, ten outputs observed
 * and weighted): 17 544 + 2 x 10 992 + 14 x 8 = 39 640, where cloudsc2_tl_launch_parjac alone writes 17 544 + 4 x 10 992 = 61 512.
 *   traj_in  as for cloudsc2_tl_launch_parjac (qsat may be NULL: SATUR evaluated in the sweep).
 *   resid    read only.  A field with a NULL pointer is an output that is not observed; at least one must be given.
 *   weight   read only; may be NULL.  A NULL field is weight 1; a field given for an output that is not observed is an error.
 *            clc and covptot depend on none of the parameters: observed, they contribute exact zeros and their planes are not read.
 *            Half level 0 of the four fluxes (the zero flux at the model top) is not read either, nor any value of a padded tail column.
 *   work     device, cloudsc2_parnormal_work_doubles() doubles (CLOUDSC2_NNORMAL x the padded column count), the caller's.
 *   normal   device, CLOUDSC2_NNORMAL doubles, assigned: the upper triangle of H row by row in CLOUDSC2_NPAR order (10), then g (4).
 *   Without LEVAPLS2 .OR. LDRAIN1D three directions run and every entry that involves rpecons is assigned exactly 0.0.
 * CLOUDSC2_EINVAL (reported before the device is looked for): a NULL prm, traj_in, resid, work or normal; prm->lphylin = 0; the evaporation
 * branch with rpecons = 0; no observed output; a weight for an unobserved output; residual or weight fields whose block strides per
 * layout group differ, among themselves or from each other; bad shapes.  Without a device: CLOUDSC2_ENODEVICE.
 * It takes the caller's stream, neither allocates nor synchronises (apart from the CETA table of a grid's first use) and is two plain
 * kernel nodes in a chain under stream capture.  It is not paced, has 64-bit offsets only, and is no kernel family of
 * cloudsc2_variant_built / cloudsc2_kernel_occupancy / the launch log. */
#define CLOUDSC2_NNORMAL (CLOUDSC2_NPAR * (CLOUDSC2_NPAR + 1) / 2 + CLOUDSC2_NPAR) /* 14 */
int cloudsc2_parnormal_work_doubles(int nproma, int ngptot, long long* n);
int cloudsc2_parnormal_launch(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot,
                              const cloudsc2_inputs* traj_in, const cloudsc2_outputs* resid, const cloudsc2_outputs* weight,
                              double* work, double* normal /* device, [CLOUDSC2_NNORMAL] */, void* stream);

/* The parameter Jacobian and the normal equations of COLUMN SUMS in one sweep.  Observations of a cloud scheme are sums over the column,
 * y_n[c] = sum_k w_n[k] out_n[k, c] (cloudsc2_nl_launch_colsum): surface rain and snow, column-integrated heating.  Their sensitivities
 * s[a][n][c] = sum_k w_n[k] (d out_n / d p_a)[k, c] need only the level loop of cloudsc2_tl_launch_parjac: its sensitivities are folded
 * into per-lane accumulators, the fold of the column-sum sweeps to the bit (acc = +0; acc = fl(acc + fl(w_n[k] J[k])), half level 0 of a
 * flux skipped), and no sensitivity plane exists.  Bytes per column (NLEV 137, fp64): 17 544 read plus 8 per stored sum, against
 * 17 544 + NP x 10 992 of cloudsc2_tl_launch_parjac plus the reads of a fold over its planes.
 *   wtable     device, the table of the column-sum launchers: ten rows of nlev + 1 in the order of cloudsc2_outputs.  The rows of clc
 *              and covptot, which depend on no parameter, are not read.
 *   cloudsc2_parjac_launch_colsum     sens_sums[a] (a in CLOUDSC2_NPAR order): 2-D (nblocks, nproma) fields, a NULL field is an absent sum;
 *              the same fields must be present in every block that is looked at and all must share one block stride >= nproma.  Every
 *              active column of a present sum is assigned; a clc or covptot sum receives exact zeros; the padded tail is not written.
 *              Without LEVAPLS2 .OR. LDRAIN1D three directions run and sens_sums[CLOUDSC2_NPAR - 1] (rpecons) is not looked at.
 *   cloudsc2_parnormal_launch_colsum  resid / weight: 2-D (nblocks, nproma) fields, read only: the column's residual (model sum -
 *              observed sum) and diagonal weight per observed sum; a NULL residual is an unobserved sum, weight NULL or a NULL weight
 *              field is weight 1.  Per active column the observed sums are taken in the order of cloudsc2_outputs and
 *              H[a][b] += (w s_a) s_b, g[a] += (w s_a) r are formed in double; work and normal are those of cloudsc2_parnormal_launch
 *              (cloudsc2_parnormal_work_doubles), the same fold over the columns, the rpecons entries exactly 0.0 without the
 *              evaporation branch.
 * CLOUDSC2_EINVAL (reported before the device is looked for, the message names the launcher): a NULL prm, traj_in, wtable, sens_sums /
 * resid, work or normal; prm->lphylin = 0; the evaporation branch with rpecons = 0; no sum present / observed; a weight without its
 * residual; block strides that differ inside one call or lie below nproma; blocks of sens_sums with different fields present; a kernel
 * variant that is not built; bad shapes.  Without a device: CLOUDSC2_ENODEVICE.
 * Both take the caller's stream, neither allocate nor synchronise (apart from the CETA table of a grid's first use) and are plain kernel
 * nodes under stream capture (one, and two in a chain).  Not paced; no kernel family of cloudsc2_variant_built /
 * cloudsc2_kernel_occupancy / the launch log. */
int cloudsc2_parjac_launch_colsum(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot,
                                  const cloudsc2_inputs* traj_in, const cloudsc2_real* wtable,
                                  const cloudsc2_outputs* sens_sums /* [CLOUDSC2_NPAR] */, void* stream);
int cloudsc2_parnormal_launch_colsum(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot,
                                     const cloudsc2_inputs* traj_in, const cloudsc2_real* wtable, const cloudsc2_outputs* resid,
                                     const cloudsc2_outputs* weight, double* work, double* normal /* device, [CLOUDSC2_NNORMAL] */,
                                     void* stream);

/* Perturbed-parameter ensembles: `members` parameter sets over one state (or one state each) in ONE call, the four parameters read on the
 * DEVICE.  The launchers above carry the parameters inside the constants of the kernel-argument segment, so the host must know their
 * values; these three put one argument block per member into device memory instead: a first kernel derives member k's block from the
 * template the host builds from prm (pointers advanced by k x the field's member stride, constants from row k of params_dev, the
 * expressions of the host's derivation in their order), the sweep then runs members x ceil(ncols_pad / 128) workgroups, workgroup b for
 * member b / ceil(ncols_pad / 128).  Member k's results are the bits the parent launcher gives for a prm holding row k's values:
 *   cloudsc2_nl_launch_ens   cloudsc2_ad_launch_forward (the NL sweep, with the cover checkpoint when LEVAPLS2 .OR. LDRAIN1D),
 *   cloudsc2_tl_launch_ens   cloudsc2_tl_launch_par, the parameter tangents row k of dparams_dev,
 *   cloudsc2_vjp_launch_ens  cloudsc2_vjp_launch_par, the parameter adjoints assigned to row k of par_adj; its fold runs once per member
 *                            in cloudsc2_vjp_launch_par's order.
 *   params_dev, dparams_dev, par_adj   device, (members, CLOUDSC2_NPAR) doubles in CLOUDSC2_NPAR order; read / written by the kernels only.
 *   *_mstride   per argument block an array of member strides in ELEMENTS, one per field in the order of the block's struct (16 for
 *               cloudsc2_inputs, 10 for cloudsc2_outputs); 0: all members share the field; NULL: all zero.  The block itself holds
 *               member 0's pointers and the block strides, which all members share.  A field the members write (traj_out and scratch of the NL
 *               sweep, pert_out, adj_in) must not be shared by more than one member: CLOUDSC2_EINVAL.
 *   scratch, scratch_mstride   the cover-checkpoint plane(s), as for the parents (required with the evaporation branch).
 *   workspace   device, cloudsc2_ens_workspace_bytes() bytes, the caller's, 256-byte aligned: the members' argument blocks and, for
 *               the reverse sweep, members x CLOUDSC2_NPAR x the padded column count doubles.  One query serves all three.
 *   With the evaporation branch every member's rpecons must not be 0; the values live on the device, so this is NOT checked.
 * 1 <= members <= 65535 and members x ceil(ncols_pad / 128) < 2^31, else CLOUDSC2_EINVAL; prm->lphylin = 0: CLOUDSC2_EINVAL; the other
 * errors are the parents'.  No launcher allocates, copies or synchronises (apart from the CETA table of a grid's first use); each is two
 * plain kernel nodes in a chain under stream capture, the reverse sweep three.  They are not paced (fair = 0, no pacing fields), are no
 * kernel family of cloudsc2_variant_built / cloudsc2_kernel_occupancy and do not appear in the launch log. */
long long cloudsc2_ens_workspace_bytes(int members, int nproma, int nlev, int ngptot); /* < 0: CLOUDSC2_EINVAL */
int cloudsc2_nl_launch_ens(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, int members,
                           const double* params_dev, const cloudsc2_inputs* traj_in, const long long* traj_in_mstride,
                           const cloudsc2_outputs* traj_out, const long long* traj_out_mstride, cloudsc2_real* scratch,
                           long long scratch_mstride, void* workspace, void* stream);
int cloudsc2_tl_launch_ens(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, int satur, int members,
                           const double* params_dev, const double* dparams_dev, const cloudsc2_inputs* traj_in,
                           const long long* traj_in_mstride, const cloudsc2_inputs* pert_in, const long long* pert_in_mstride,
                           const cloudsc2_outputs* pert_out, const long long* pert_out_mstride, void* workspace, void* stream);
int cloudsc2_vjp_launch_ens(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, int satur, int members,
                            const double* params_dev, const cloudsc2_inputs* traj_in, const long long* traj_in_mstride,
                            const cloudsc2_outputs* traj_out, const long long* traj_out_mstride, const cloudsc2_inputs* adj_in,
                            const long long* adj_in_mstride, const cloudsc2_outputs* adj_out /* read only */,
                            const long long* adj_out_mstride, const cloudsc2_real* scratch, long long scratch_mstride, void* workspace,
                            double* par_adj, void* stream);

/* Per-column parameter maps: rkconv, rclcrit, rlptrc, rpecons as (nblocks, nproma) FIELDS, read on the device.  The spatial counterpart
 * of the ensemble launchers: there a member has its own four values, here a column has.  A lane loads its four doubles before the level
 * loop and derives its constants with the expressions of the host's derivation in their order, so column c of everything a launcher
 * writes is the bits its scalar parent gives for a prm holding column c's four values:
 *   cloudsc2_nl_launch_parmap   cloudsc2_ad_launch_forward (qsat given, or NULL: SATUR evaluated in the sweep; the cover checkpoint
 *                               `scratch` is kept exactly with LEVAPLS2 .OR. LDRAIN1D),
 *   cloudsc2_tl_launch_parmap   cloudsc2_tl_launch_par, the parameter tangents column c of dpar_dev,
 *   cloudsc2_vjp_launch_parmap  cloudsc2_vjp_launch_par; column c of par_adj_dev is ASSIGNED that column's row of the parent's
 *                               workspace, in every active column.  There is no fold.
 *   par_dev, dpar_dev, par_adj_dev   device, (CLOUDSC2_NPAR, ncols_pad) doubles, ncols_pad = nblocks x nproma: row k is parameter k in
 *                               CLOUDSC2_NPAR order, indexed by padded column number block x nproma + lane (the layout of the parent's
 *                               workspace).  Read / written by the kernels only, in active columns only: the padded tail is not touched.
 *   With the evaporation branch every column's rpecons must not be 0; the values live on the device, so this is NOT checked.
 * CLOUDSC2_EINVAL, before a device is looked for: a NULL table, satur other than 0 or 1, prm->lphylin = 0, a NULL argument block or
 * required field, block strides that differ within a layout group, and the parents' other refusals.  No launcher allocates, copies or
 * synchronises (apart from the CETA table of a grid's first use); each is one plain kernel node under stream capture.  Not paced, no
 * kernel family of cloudsc2_variant_built / cloudsc2_kernel_occupancy, no launch-log entry. */
int cloudsc2_nl_launch_parmap(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, const double* par_dev,
                              const cloudsc2_inputs* traj_in, const cloudsc2_outputs* traj_out, cloudsc2_real* scratch, void* stream);
int cloudsc2_tl_launch_parmap(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, int satur,
                              const double* par_dev, const double* dpar_dev, const cloudsc2_inputs* traj_in,
                              const cloudsc2_inputs* pert_in, const cloudsc2_outputs* pert_out, void* stream);
int cloudsc2_vjp_launch_parmap(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, int satur,
                               const double* par_dev, const cloudsc2_inputs* traj_in, const cloudsc2_outputs* traj_out,
                               const cloudsc2_inputs* adj_in, const cloudsc2_outputs* adj_out /* read only */,
                               const cloudsc2_real* scratch, double* par_adj_dev, void* stream);

/* Column sums of an ensemble's members: the column-sum launchers for `members` parameter sets in ONE call, the parameters read on the
 * device, no output, cotangent or tangent plane.  What a calibration needs of a member is K x (a few) x one value per column; the
 * dense ensemble writes ten planes per member.  Argument blocks, member strides, params_dev / dparams_dev / par_adj and the workspace
 * (the same query) are those of the ensemble launchers above; weights (shared by the members), sums, keep and the definition of a sum
 * are those of the column-sum launchers.  Member k's results are the bits of the parent for a prm holding row k's values:
 *   cloudsc2_nl_launch_ens_colsum   cloudsc2_nl_launch_colsum.  keep given: every member keeps its PFPLSL5 / PFPLSN5 (keep_mstride, the
 *                                   two entries of fplsl / fplsn; never shared) and, with the evaporation branch, its cover checkpoint.
 *   cloudsc2_tl_launch_ens_colsum   cloudsc2_tl_launch_colsum plus the source terms of the parameter tangents, row k of dparams_dev: each
 *                                   sum is the column-sum fold of cloudsc2_tl_launch_par's output tangent.  pert_in may have every
 *                                   field NULL (parameter tangents alone).
 *   cloudsc2_vjp_launch_ens_colsum  cloudsc2_vjp_launch_colsum for the field gradients given in adj_in, and row k of par_adj the bits of
 *                                   cloudsc2_vjp_launch_par given the planes fl(w_n[k] ybar_n[c]).  adj_in may have every field NULL:
 *                                   the parameter adjoints alone, no plane is written (the calibration case).
 *   (The fp32 library runs the reverse sweep twice when a field gradient is wanted: once for the parameter adjoints, once more without
 *   them for the field gradients, which only then have the parent's bits on the MI355X -- one more kernel node.)
 *   sums_mstride   the member strides of the sums / cotangent sums, in elements, per field of cloudsc2_outputs.  Sums the members write
 *                  must not be shared; cotangent sums may be (stride 0).
 * The refusals are the parents': CLOUDSC2_EINVAL for a NULL block, a sum with no weight table, no sum given, members < 1, members x
 * ceil(ncols_pad / 128) >= 2^31, a written field shared by the members, and the column-sum launchers' own list.  No launcher allocates,
 * copies or synchronises; two plain kernel nodes in a chain under stream capture, the reverse sweep three.  Not paced, no kernel family,
 * no launch-log entry. */
int cloudsc2_nl_launch_ens_colsum(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, int members,
                                  const double* params_dev, const cloudsc2_inputs* in, const long long* in_mstride,
                                  const cloudsc2_real* weights, const cloudsc2_outputs* sums, const long long* sums_mstride,
                                  const cloudsc2_outputs* keep, const long long* keep_mstride, cloudsc2_real* scratch,
                                  long long scratch_mstride, void* workspace, void* stream);
int cloudsc2_tl_launch_ens_colsum(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, int satur, int members,
                                  const double* params_dev, const double* dparams_dev, const cloudsc2_inputs* traj_in,
                                  const long long* traj_in_mstride, const cloudsc2_inputs* pert_in, const long long* pert_in_mstride,
                                  const cloudsc2_real* weights, const cloudsc2_outputs* pert_sums, const long long* sums_mstride,
                                  void* workspace, void* stream);
int cloudsc2_vjp_launch_ens_colsum(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, int satur, int members,
                                   const double* params_dev, const cloudsc2_inputs* traj_in, const long long* traj_in_mstride,
                                   const cloudsc2_outputs* traj_out, const long long* traj_out_mstride, const cloudsc2_inputs* adj_in,
                                   const long long* adj_in_mstride, const cloudsc2_real* weights,
                                   const cloudsc2_outputs* adj_sums /* read only */, const long long* sums_mstride,
                                   const cloudsc2_real* scratch, long long scratch_mstride, void* workspace, double* par_adj,
                                   void* stream);

/* Several tangents or cotangents over ONE trajectory -- a Jacobian block, a singular-vector iteration, an ensemble of perturbations.
 * cloudsc2_tl_launch_batch replaces nbatch calls of cloudsc2_tl_launch without trajectory stores (traj_out all NULL),
 * cloudsc2_vjp_launch_batch nbatch calls of cloudsc2_vjp_launch, over the same traj_in: every direction's results are the bits those
 * calls give.  The trajectory planes are read once per launch instead of once per direction (bytes per column and direction, NLEV 137, fp64: 46 080 -> 28 536 + 17 544 / n for TL, 48 240 -> 28 504 + 19 736 / n
 * for the reverse sweep, n = directions per launch).
 *   pert_in / pert_out, adj_in / adj_out: arrays of nbatch argument blocks, one element per direction, used as by the single
 *   launchers (adj_out read only; padded tail columns not written).  Every direction must have the same block stride per layout
 *   group, and traj_in->qsat is required (there is no fused SATUR here): otherwise CLOUDSC2_EINVAL, as for nbatch < 1 or a NULL
 *   field.  Without a device: CLOUDSC2_ENODEVICE.
 * A launch carries at most cloudsc2_batch_max() directions (4 in this build: what the fp64 kernels hold in registers without
 * scratch at one wave per SIMD); a larger nbatch is split into balanced chunks in stream order (5 -> 3 + 2, 9 -> 3 + 3 + 3), and
 * nbatch = 1 is the single launcher itself.  Strides, pacing, stream capture and first-use behaviour are those of the other
 * launchers: apart from the CETA table they neither allocate device memory nor synchronise. */
int cloudsc2_batch_max(void);
int cloudsc2_tl_launch_batch(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot,
                             const cloudsc2_inputs* traj_in, int nbatch,
                             const cloudsc2_inputs* pert_in /* [nbatch] */, const cloudsc2_outputs* pert_out /* [nbatch] */,
                             void* stream);
int cloudsc2_vjp_launch_batch(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot,
                              const cloudsc2_inputs* traj_in, const cloudsc2_outputs* traj_out, int nbatch,
                              const cloudsc2_inputs* adj_in /* [nbatch] */, const cloudsc2_outputs* adj_out /* [nbatch], read only */,
                              const cloudsc2_real* scratch, void* stream);

/* The AD leg of the adjoint test with its norms formed in the sweep (cloudsc_driver_ad_mod.F90:198-267): the reverse sweep alone
 * in the assign form (zeroed input adjoints + CLOUDSC2AD), and for every active column norm2 = <x0, x_adj> with x0 = 0.01 * the
 * trajectory inputs (ZSUPSAT0 = 0, :139,240-256) and norm3 = |norm1 - norm2| / EPSILON(1._8) [/ norm2] (:258-264), taken while
 * x_adj is in registers instead of re-reading 32 planes.  norms(3, NBLOCKS*NPROMA) device doubles: row 0 = norm1 on entry
 * (cloudsc2_tl_launch_self's yy, or cloudsc2_adjoint_norms_launch's first half), rows 1-2 written; *blockmax (device double,
 * zero or an earlier maximum on entry) is raised to the largest |norm3| (NaN counts as +inf).  Not with LEVAPLS2 / LDRAIN1D
 * (the reverse sweep alone lacks the cover checkpoints: cloudsc2_ad_launch_assign + cloudsc2_adjoint_norms_launch then). */
int cloudsc2_ad_launch_reverse_norms(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot,
                                     const cloudsc2_inputs* traj_in, const cloudsc2_outputs* traj_out,
                                     const cloudsc2_inputs* adj_in, const cloudsc2_outputs* adj_out,
                                     double* norms, double* blockmax, void* stream);

/* Taylor-test statistics for one lambda (ERROR_NORM, cloudsc_driver_tl_mod.F90:21-31, calls :233-244):
 * for each NPROMA block and each of the 10 output fields, sums over the block's active columns and all
 * levels of (F(x)-F(x+lambda dx)) and of (TL dx * lambda).  sums(NBLOCKS,10,2) device doubles. */
int cloudsc2_taylor_sums_launch(int nproma, int nlev, int ngptot, const cloudsc2_outputs* f,
                                const cloudsc2_outputs* f_pert, const cloudsc2_outputs* tl, double lambda,
                                double* sums, void* stream);

/* The lambda loop of the Taylor test in one sweep (cloudsc_driver_tl_mod.F90:197-244: the ten perturbed CLOUDSC2 calls,
 * ZLAMBDA = 10^-1 .. 10^-10, each followed by the ten ERROR_NORM calls).  The lambdas lie on the lanes of a wave -- 6 columns x
 * 10 lambdas per wave64 --, every lane runs the NL sweep of its column on x + lambda*(0.01*x) (:200-215), compares each level's
 * outputs with the BASE run's (`out`, read) in registers and sums TL output field k of its column; a second small kernel sums
 * the per-column results over the active columns of each block of the statistic (`nproma_stat`: the caller's NPROMA, which may
 * differ from the arrays' blocking `nproma`).  The state is read once for all ten runs and no perturbed outputs are written.
 *   in   the unperturbed state (qsat: the SATUR result, or NULL = SATUR in the sweep)
 *   out  the outputs of the base run (cloudsc2_nl_launch on the same state), tl the TL outputs (cloudsc2_tl_launch)
 *   work device scratch of cloudsc2_taylor_sweep_work_doubles(nproma, ngptot) doubles
 *   sums(2, 10, nblocks_stat, 10) device doubles, the layout of ten cloudsc2_taylor_sums_launch calls one after the other:
 *        sums[((il*nblocks_stat + ibl)*10 + f)*2 + {0,1}] = { sum(F - F5(lambda_il)), sum(TL)*lambda_il }. */
int cloudsc2_taylor_sweep_work_doubles(int nproma, int ngptot, long long* n);
int cloudsc2_taylor_sweep_launch(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, int nproma_stat,
                                 const cloudsc2_inputs* in, const cloudsc2_outputs* out, const cloudsc2_outputs* tl,
                                 double* work, double* sums, void* stream);

/* Adjoint-test norms per column (cloudsc_driver_ad_mod.F90:184-195,240-264):
 * norm1 = sum_lev sum_10 y*y, norm2 = sum_lev sum_16 (0.01*x_traj)*x_adj (PSUPSAT term uses x0=0, :139),
 * norm3 = |n1-n2|/eps [/n2].  norms(3, ncols_padded) device doubles; *blockmax (device double) receives
 * max(norm3) over all columns via atomic max (must be zeroed by the caller). */
int cloudsc2_adjoint_norms_launch(int nproma, int nlev, int ngptot, const cloudsc2_inputs* traj_in,
                                  const cloudsc2_field* qsat, const cloudsc2_outputs* y,
                                  const cloudsc2_inputs* x_adj, double* norms, double* blockmax, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Driver level: HOST pointers in the GLOBAL_STATE layout, synchronous.  These are what the Fortran
 * drivers with the reference signatures bind through ISO_C_BINDING.  Device buffers
 * are owned by the library and cached between calls (cloudsc2_release_workspace frees them).
 * Argument order follows CLOUDSC_DRIVER (src/cloudsc2_nl/cloudsc_driver_mod.F90:22-30):
 *   PT PQ TENDENCY_CML TENDENCY_LOC PAP PAPH PLU PLUDE PMFU PMFD PA PCLV PSUPSAT PCOVPTOT PFPLSL PFPLSN
 *   PFHPSL PFHPSN, with TENDENCY_* passed as the base address of B_CML / B_LOC.
 * kernel_ms (optional): device time of the kernels only (hipEvent), excluding H2D/D2H.
 * Only what the kernels read is uploaded and only what they write is downloaded (17.5 + 12.1 KB per column);
 * everything else keeps its host value, as under the reference.  cloudsc2_nl_run processes the blocks in slabs of
 * ~16384 columns, uploading slab i+1 from a helper thread while slab i is computed and downloaded (kernel_ms is then
 * the sum over the slabs' launches).
 * ------------------------------------------------------------------------------------------------ */
int cloudsc2_nl_run(const cloudsc2_params* prm, int nproma, int nlev, int ngptot, double ptsphy,
                    const cloudsc2_real* pt, const cloudsc2_real* pq, const cloudsc2_real* b_cml, cloudsc2_real* b_loc,
                    const cloudsc2_real* pap, const cloudsc2_real* paph, const cloudsc2_real* plu, const cloudsc2_real* plude,
                    const cloudsc2_real* pmfu, const cloudsc2_real* pmfd, cloudsc2_real* pa, const cloudsc2_real* pclv,
                    const cloudsc2_real* psupsat, cloudsc2_real* pcovptot, cloudsc2_real* pfplsl, cloudsc2_real* pfplsn,
                    cloudsc2_real* pfhpsl, cloudsc2_real* pfhpsn, double* kernel_ms);

/* CLOUDSC_DRIVER_TL (src/cloudsc2_tl/cloudsc_driver_tl_mod.F90:33-314): NL, 1 % increments, TL, ten
 * perturbed NL runs, ERROR_NORM per block, max over blocks.  znormg[10] receives the raw ratios
 * (the values printed at :275).  Returns CLOUDSC2_ETLWRONG where the reference STOPs (:247-249). */
int cloudsc2_tl_taylor_run(const cloudsc2_params* prm, int nproma, int nlev, int ngptot, double ptsphy,
                           const cloudsc2_real* pt, const cloudsc2_real* pq, const cloudsc2_real* b_cml, cloudsc2_real* b_loc,
                           const cloudsc2_real* pap, const cloudsc2_real* paph, const cloudsc2_real* plu, const cloudsc2_real* plude,
                           const cloudsc2_real* pmfu, const cloudsc2_real* pmfd, cloudsc2_real* pa, const cloudsc2_real* pclv,
                           const cloudsc2_real* psupsat, cloudsc2_real* pcovptot, cloudsc2_real* pfplsl, cloudsc2_real* pfplsn,
                           cloudsc2_real* pfhpsl, cloudsc2_real* pfhpsn, double znormg[10], double* kernel_ms);

/* CLOUDSC_DRIVER_AD (src/cloudsc2_ad/cloudsc_driver_ad_mod.F90:22-297): TL, norm1, zero, AD, norm2,
 * norm3; *znormg = max over columns of norm3 (the value printed at :287). */
int cloudsc2_ad_symmetry_run(const cloudsc2_params* prm, int nproma, int nlev, int ngptot, double ptsphy,
                             const cloudsc2_real* pt, const cloudsc2_real* pq, const cloudsc2_real* b_cml, cloudsc2_real* b_loc,
                             const cloudsc2_real* pap, const cloudsc2_real* paph, const cloudsc2_real* plu, const cloudsc2_real* plude,
                             const cloudsc2_real* pmfu, const cloudsc2_real* pmfd, cloudsc2_real* pa, const cloudsc2_real* pclv,
                             const cloudsc2_real* psupsat, cloudsc2_real* pcovptot, cloudsc2_real* pfplsl, cloudsc2_real* pfplsn,
                             cloudsc2_real* pfhpsl, cloudsc2_real* pfhpsn, double* znormg, double* kernel_ms);

void cloudsc2_release_workspace(void);

/* ------------------------------------------------------------------------------------------------
 * Resident state: a GLOBAL_STATE (cloudsc2_array_state_mod.F90:26-79) that lives on the device and is owned by the
 * library -- for callers whose model keeps its physics state in HBM, and for the Fortran mains' CLOUDSC2_RESIDENT=1 mode.
 * The host-pointer entry points above spend 98 % of their time on PCIe; with a handle the flow of the reference main
 * (LOAD -> driver -> VALIDATE) never builds the NPROMA-blocked arrays on the host:
 *   cloudsc2_state_create     allocates all arrays as ONE placed allocation (cloudsc2_device_malloc), zero-filled
 *                             (FIELD_INIT, :186-190); the layout is the reference's (include file header).
 *   cloudsc2_state_expand     EXPAND_R2 (expand_mod.F90:270-302) of one field from a KLON-column HOST table (KLON, NLEVx),
 *                             `period`/`start` as cloudsc2_expand_offsets gives them; repeated calls fill the state.
 *   cloudsc2_state_upload / _download   the same transfers as the host-pointer drivers (what the kernels read / write).
 *   cloudsc2_state_nl         SATUR + CLOUDSC2 over all blocks, `repeats` times back to back; *kernel_ms = mean device time.
 *   cloudsc2_state_tl_taylor, cloudsc2_state_ad_symmetry   the two self-tests of cloudsc2_tl_taylor_run / _ad_symmetry_run
 *                             on the resident state (their scratch arrays are a second allocation owned by the handle).
 *   cloudsc2_state_validate   VALIDATE_R2/R3 (validate_mod.F90:165-261) of one field against a KLON-column HOST reference
 *                             table (KLON, NLEVx, ndim): stats[5] as cloudsc2_validate_launch.
 *   cloudsc2_state_field      the device pointer + block stride of one field, for the kernel-level entry points -- in the
 *                             DEVICE blocking (cloudsc2_state_blocking), which is the library's choice, see below.
 * Blocking.  `nproma` of cloudsc2_state_create is the CALLER's NPROMA: the blocking of the host arrays of _upload / _download, the
 * block ERROR_NORM of the Taylor test sums over (cloudsc_driver_tl_mod.F90:21-31) and the blocks whose padding MINVAL / MAXVAL of
 * the validator see (validate_mod.F90:186-187).  The device arrays themselves are blocked for the kernels: the caller's NPROMA
 * when it is a multiple of 64, else 128 (CLOUDSC2_STATE_NPROMA=0: always the caller's) -- every column is independent, so the
 * results are the same bits whatever the blocking, and NPROMA 32 (the reference README's) or 100 cost the TL / AD sweeps 8 %.
 * A handle belongs to the HIP device that was current when it was created; calls are synchronous.
 * ------------------------------------------------------------------------------------------------ */
typedef struct cloudsc2_state cloudsc2_state;
enum {
  CLOUDSC2_F_PT = 0, CLOUDSC2_F_PQ, CLOUDSC2_F_PAP, CLOUDSC2_F_PAPH, CLOUDSC2_F_PLU, CLOUDSC2_F_PLUDE, CLOUDSC2_F_PMFU,
  CLOUDSC2_F_PMFD, CLOUDSC2_F_PA, CLOUDSC2_F_PSUPSAT, CLOUDSC2_F_PCOVPTOT,                  /* 0..10  */
  CLOUDSC2_F_PFPLSL, CLOUDSC2_F_PFPLSN, CLOUDSC2_F_PFHPSL, CLOUDSC2_F_PFHPSN, CLOUDSC2_F_QSAT, /* 11..15 */
  CLOUDSC2_F_CML_T = 16, /* + plane: T A Q QL QI QR QS QV = 16..23 (TENDENCY_CML) */
  CLOUDSC2_F_LOC_T = 24, /* 24..31 (TENDENCY_LOC) */
  CLOUDSC2_F_PCLV_QL = 32 /* 32..36 (PCLV: QL QI QR QS QV) */
};
int cloudsc2_state_create(int nproma, int nlev, int ngptot, cloudsc2_state** state);
void cloudsc2_state_destroy(cloudsc2_state* state);
int cloudsc2_state_field(const cloudsc2_state* state, int field, cloudsc2_field* f);
int cloudsc2_state_blocking(const cloudsc2_state* state, int* nproma_device, int* nproma_caller);
int cloudsc2_state_expand(cloudsc2_state* state, int field, const cloudsc2_real* table, int klon, int period, long long start);
int cloudsc2_state_upload(cloudsc2_state* state,
                          const cloudsc2_real* pt, const cloudsc2_real* pq, const cloudsc2_real* b_cml, cloudsc2_real* b_loc,
                          const cloudsc2_real* pap, const cloudsc2_real* paph, const cloudsc2_real* plu, const cloudsc2_real* plude,
                          const cloudsc2_real* pmfu, const cloudsc2_real* pmfd, cloudsc2_real* pa, const cloudsc2_real* pclv,
                          const cloudsc2_real* psupsat, cloudsc2_real* pcovptot, cloudsc2_real* pfplsl, cloudsc2_real* pfplsn,
                          cloudsc2_real* pfhpsl, cloudsc2_real* pfhpsn);
int cloudsc2_state_download(cloudsc2_state* state, cloudsc2_real* b_loc, cloudsc2_real* pa, cloudsc2_real* pcovptot,
                            cloudsc2_real* pfplsl, cloudsc2_real* pfplsn, cloudsc2_real* pfhpsl, cloudsc2_real* pfhpsn);
int cloudsc2_state_nl(cloudsc2_state* state, const cloudsc2_params* prm, double ptsphy, int repeats, double* kernel_ms);
int cloudsc2_state_tl_taylor(cloudsc2_state* state, const cloudsc2_params* prm, double ptsphy, double znormg[10], double* kernel_ms);
int cloudsc2_state_ad_symmetry(cloudsc2_state* state, const cloudsc2_params* prm, double ptsphy, double* znormg, double* kernel_ms);
int cloudsc2_state_validate(cloudsc2_state* state, int field, int ndim, const cloudsc2_real* ref_table, int klon, int period,
                            long long start, double stats[5]);

/* The synthetic KLON-column atmosphere every front end of this repository loads when config-files/input.h5 is absent (it is not
 * distributed with the reference: .MISSING_LARGE_BLOBS) -- what CLOUDSC2_ARRAY_STATE_LOAD (cloudsc2_array_state_mod.F90:153-204) would
 * read from the file: PT PQ PAP PAPH(nlev+1) PLU PLUDE PMFU PMFD PCLV(QL) PCLV(QI) TENDENCY_CML%T TENDENCY_CML%Q, each (nlev[+1], klon)
 * row-major = Fortran (KLON, KLEV[+1]), always double; everything else of the state is zero.  Pure host code, one implementation for
 * the Fortran mains and the Python harness: the Taylor test's verdict is decided by round-off, so tables that differ
 * in the last place (numpy's, flang's and glibc's exp / pow do) give different verdicts for the same library and size.  rd, rv, rtt:
 * YOMCST's RD, RV, RTT (287.0597, 461.5250, 273.16). */
int cloudsc2_synthetic_table(int klon, int nlev, double rd, double rv, double rtt, double* pt, double* pq, double* pap, double* paph,
                             double* plu, double* plude, double* pmfu, double* pmfd, double* pql, double* pqi, double* tend_t,
                             double* tend_q);

/* Verdict logic of the two self-tests, pure host code (no device needed).
 * cloudsc2_taylor_verdict: cloudsc_driver_tl_mod.F90:272-311; znormg = raw ratios; returns 1 = PASSED;
 *   *itest = penalty / error code (13 when no lambda <= 1e-4 reaches |1-ratio| < 0.5).
 * cloudsc2_adjoint_verdict: cloudsc_driver_ad_mod.F90:289; returns 1 = TEST OK. */
int cloudsc2_taylor_verdict(const double znormg[10], int* itest);
int cloudsc2_adjoint_verdict(double znormg);

/* --------------------------------------------------------------------------------------------------
 * Data formats either side of the path, device side.  The HDF5 files hold
 * KLON-column tables, stored (…, KLON) in C order = Fortran (KLON, …) (hdf5_file_mod.F90); the file
 * reader/writer itself is include/cloudsc2_io.h (libcloudsc2_io.so, needs libhdf5).
 *
 * cloudsc2_expand_launch  replaces EXPAND_R2/R3 (src/common/module/expand_mod.F90:270-335) for data that
 *   stays on the GPU: field(jl,jk,jm,ibl) = table((start + (ibl*NPROMA + jl) mod period) mod KLON, jk, jm), zero in
 *   the padded tail of the last block.  `table` (device) is (KLON, nlevx, ndim) column-fastest; `period` and
 *   `start` are GET_OFFSETS' size and start-1 (expand_mod.F90:30-46; see cloudsc2_expand_offsets): the rank's
 *   table slice START..END tiled with period SIZE, as LOAD_AND_EXPAND does (:101-116).  (For those pairs start + period
 *   <= KLON and the outer mod never acts; with period = KLON any start >= 0 continues the periodic tiling at global
 *   column `start`.)  The
 *   reference indexes out of bounds when a block starts at a multiple of KLON other than KLON itself
 *   (MOD(gidx,nlon) = 0, :289); this implements the periodic tiling it intends.
 * cloudsc2_validate_launch  replaces VALIDATE_R2/R3 (src/common/module/validate_mod.F90:165-261) without
 *   expanding the reference: stats[5] (device) = { min FIELD, max FIELD (whole blocks, padding included),
 *   max |FIELD-REF|, sum |FIELD-REF|, sum |REF| (active columns) }.  `workspace` (device) needs
 *   cloudsc2_validate_workspace_doubles() doubles.  Sums are folded in a fixed order (deterministic).
 * ------------------------------------------------------------------------------------------------ */
int cloudsc2_expand_launch(const cloudsc2_real* table, int klon, int period, long long start, int nlevx, int ndim,
                           int nproma, long long ngptot, cloudsc2_field field, void* stream);
int cloudsc2_validate_workspace_doubles(void);
int cloudsc2_validate_launch(const cloudsc2_real* table, int klon, int period, long long start, int nlevx, int ndim,
                             int nproma, long long ngptot, cloudsc2_field field, double* workspace,
                             double* stats, void* stream);
/* GET_OFFSETS (expand_mod.F90:30-46): which table columns rank `irank` of `numproc` tiles from.
 * ngptotg <= 0 means "not given".  *start is 0-based. */
void cloudsc2_expand_offsets(int klon, long long ngptot, long long ngptotg, int irank, int numproc,
                             long long* start, int* period);
/* ERROR_PRINT (validate_mod.F90:263-296): relative error in percent, option code 1..3, and whether the
 * line carries the "!!!!" warning (relative error > 10 eps).  Pure host code.  zavgpgp = esum / ngptotg. */
double cloudsc2_validate_relerr(double esum, double rsum, int* iopt, int* warn);
/* The line ERROR_PRINT writes, FORMAT(1X,A20,1X,I1,'D',I1,5(1X,E20.13),A); buf needs >= 160 bytes. */
int cloudsc2_validate_format(const char* name, int ndim, const double stats[5], long long ngptotg,
                             char* buf, int buflen);
/* The header line CLOUDSC2_ARRAY_STATE_VALIDATE prints first (cloudsc2_array_state_mod.F90:226-229). */
int cloudsc2_validate_header(char* buf, int buflen);

/* --------------------------------------------------------------------------------------------------
 * Debug: what the tests use to see which kernel variant a launch ran (host code only; the -DC2_WAVE_TIMES diagnostic build adds
 * cloudsc2_debug_wave_log, tools/wave_times.py).
 *
 * cloudsc2_variant_built  1 if the kernel variant exists in this build, 0 if not; CLOUDSC2_EINVAL for an unknown family.  No device
 *   needed.  family 0..6 as cloudsc2_kernel_occupancy's `kernel` (0 NL, 1 TL, 2 AD both sweeps, 3 AD reverse sweep, 4 batched TL,
 *   5 batched reverse sweep, 6 the parameter Jacobian's sweep), 7 TL with the parameter tangents, 8 reverse sweep with the parameter
 *   adjoints, 9 the Taylor sweep; flags = the variant's C2F_* word (cloudsc2_column.hpp), for families 4 and 5 plus 64 x directions.
 *   (The `family` column of the table of variant tables in csrc/cloudsc2_sweep_kernels.hpp; the other tables have no number.)
 * cloudsc2_debug_launch_log  the sweep kernels the CALLING THREAD's launcher calls have enqueued since its last
 *   cloudsc2_debug_launch_log_reset, in order: returns their number and writes the (family, word) pairs of the first min(max, 64) of
 *   them.  The log keeps 64 entries; further launches are counted but not recorded, so a return value above 64 says that the record
 *   is incomplete.  Only a launch the runtime accepted is logged: a launcher that returns an argument error or
 *   CLOUDSC2_ENODEVICE logs nothing.  The log is a thread-local array of integers: it makes no device call, costs nothing
 *   measurable, and is harmless during stream capture (what is logged then is the kernel captured).  max < 0, or max > 0 with a
 *   NULL array: CLOUDSC2_EINVAL.  The small kernels around the sweeps (SATUR, the folds and sums) are not logged.
 * ------------------------------------------------------------------------------------------------ */
int cloudsc2_variant_built(int family, unsigned flags);
void cloudsc2_debug_launch_log_reset(void);
int cloudsc2_debug_launch_log(int* families, unsigned* flags, int max);

#ifdef __cplusplus
}
#endif
#endif /* CLOUDSC2_HIP_H */
