// cloudsc2_policy.hip -- launch policy: which launches keep their waves abreast ("fair"), nap their lighter SIMDs or pace their
// partial rounds, and the device probes behind those decisions.  Every launcher asks schedule() once per launch (cloudsc2_host.hpp).

#include "cloudsc2_host.hpp"

using namespace cloudsc2;

namespace {

// The knobs of the policy, read once per process (measurements only; include/cloudsc2_hip.h)
struct Knobs {
  bool pace_off;  // CLOUDSC2_PACE=0: TL / AD launches are not paced, and nothing is probed for it
  int nl_light;   // CLOUDSC2_NL_LIGHT: the NL light-SIMD nap in % of a level's measured time (0 = off; 10 / 15 / 20 measured: 15 best)
  bool verbose;   // CLOUDSC2_PACE_VERBOSE: probes and paced launches reported on stderr
};
const Knobs& knobs() {
  static const char *pace = getenv("CLOUDSC2_PACE"), *light = getenv("CLOUDSC2_NL_LIGHT");
  static const Knobs k = {pace && atoi(pace) == 0, light ? atoi(light) : 15, getenv("CLOUDSC2_PACE_VERBOSE") != nullptr};
  return k;
}

hipError_t current_cus(int* dev, int* cus) {
  hipError_t e = hipGetDevice(dev);
  if (e == hipSuccess) e = hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, *dev);
  return e;
}

// (kernel, device) -> CUs, workgroups of the kernel per CU, as the runtime reports them (asked once per kernel and device; no device work)
struct Occupancy { const void* fn; int dev, cus, per_cu; };
std::mutex g_occ_mutex;
std::vector<Occupancy> g_occ;
hipError_t occupancy(const void* fn, Occupancy* o) {
  int dev = 0, cus = 0;
  hipError_t e = current_cus(&dev, &cus);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> lock(g_occ_mutex);
  for (auto& x : g_occ)
    if (x.fn == fn && x.dev == dev) { *o = x; return hipSuccess; }
  *o = Occupancy{fn, dev, cus, 0};
  if ((e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&o->per_cu, fn, kBlock, 0)) != hipSuccess) return e;
  g_occ.push_back(*o);
  return hipSuccess;
}
// for the decisions: false (and the error cleared) when the runtime has no answer
bool occupancy_known(const void* fn, Occupancy* o) {
  if (fn && occupancy(fn, o) == hipSuccess && o->cus > 0 && o->per_cu > 0) return true;
  (void)hipGetLastError();
  return false;
}

// ---------------------------------------------------------------------------------------------------------
// What the two launch heuristics take for granted about the device's dispatcher, checked on the device -- at a SYNCHRONOUS moment
// (cloudsc2_device_prepare: called by every allocating entry point of the library and by the host-array drivers, or by the caller
// itself), never from a launch: the launchers only read the cached verdicts, and a device nobody prepared runs without the naps.
//
// (1) NL, one round of waves: does the device place the waves the way simd_population (cloudsc2_column.hpp) says?  A launch of the NL
//     kernel's shape (128-thread workgroups, all resident at once; five workgroups on most CUs, four on the rest) whose waves record
//     where they run (HW_ID / XCC_ID) and stay for ~30 us so that nothing is placed into a freed slot.  Any wave whose SIMD carries
//     another number of waves than predicted -- another dispatcher, other work on the device during the probe -- and the lighter
//     SIMDs' nap stays off for this device.
// (2) TL / AD, a few rounds of workgroups at `per_cu` workgroups per CU: Pace::begin decides from blockIdx mod slots alone which
//     workgroups sit on a slot that has one workgroup more to run.  That holds when (a) the first `slots` workgroups are all
//     resident at once, one per slot, and (b) a freed slot receives the next workgroup in index order.  The probe is a launch of
//     that shape (2 rounds + 0.44 of one; `per_cu` workgroups per CU enforced through LDS) whose workgroups do nothing but stay
//     for the time their class would -- 40 us the fast class (blockIdx mod slots < rem), 60 us the napping class (k = 2: 1 + 1/k) --
//     and record where they ran and when they started.  Checked per CU: it must have run (k+1) workgroups of the fast class for
//     each fast workgroup it received in the first round and k of the slow class for each slow one, and every first-round
//     workgroup must have started before the first one left.  One miss and TL / AD launches on this device are not paced.
// Each probe costs an 8-40 KB allocation, two launches on a private non-blocking stream and a copy back; the thread's capture mode
// is relaxed meanwhile, so that a graph capture going on elsewhere in the process is not invalidated.
// ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) dispatch_probe_kernel(unsigned long long* out) {
#if defined(__HIP_DEVICE_COMPILE__)
  extern __shared__ unsigned probe_lds[];
  if (threadIdx.x == 0) probe_lds[0] = blockIdx.x;  // (the allocation must not be optimised away)
  if ((threadIdx.x & 63) == 0) {
    const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4), xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20);
    out[((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6] = ((unsigned long long)xcc << 32) | hw;
  }
  for (int i = 0; i < 8; ++i) __builtin_amdgcn_s_sleep(127);  // ~65 000 clocks: every workgroup of the probe is dispatched meanwhile
#endif
}
// out[2*b] = start (100 MHz constant clock), out[2*b+1] = XCC_ID << 32 | HW_ID of workgroup b's first wave
[[maybe_unused]] constexpr unsigned kPaceProbeFastTicks = 4000u, kPaceProbeSlowTicks = 6000u;  // 40 us / 60 us: k = 2 whole rounds, nap = 1/k
__global__ void __launch_bounds__(kBlock) pace_probe_kernel(unsigned long long* out, unsigned slots, unsigned first) {
#if defined(__HIP_DEVICE_COMPILE__)
  extern __shared__ unsigned probe_lds[];
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  if (threadIdx.x == 0) {
    probe_lds[0] = blockIdx.x;
    const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4), xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20);
    out[2ull * blockIdx.x] = t0;
    out[2ull * blockIdx.x + 1] = ((unsigned long long)xcc << 32) | hw;
  }
  const unsigned stay = (blockIdx.x % slots) < first ? kPaceProbeFastTicks : kPaceProbeSlowTicks;
  for (int i = 0; i < 4096 && __builtin_amdgcn_s_memrealtime() - t0 < stay; ++i) __builtin_amdgcn_s_sleep(16);  // (bounded: every wave leaves)
#endif
}

// a probe's surroundings: relaxed capture mode for this thread, a private non-blocking stream, a device buffer
struct ProbeScope {
  hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
  bool exchanged = false;
  hipStream_t stream = nullptr;
  unsigned long long* dev = nullptr;
  hipError_t open(size_t bytes) {
    if (hipThreadExchangeStreamCaptureMode(&mode) == hipSuccess) exchanged = true; else (void)hipGetLastError();
    hipError_t e = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc((void**)&dev, bytes);
    if (e == hipSuccess) e = hipMemsetAsync(dev, 0, bytes, stream);
    return e;
  }
  hipError_t fetch(void* host, size_t bytes) {
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    return e;
  }
  ~ProbeScope() {
    if (dev) (void)hipFree(dev);
    if (stream) (void)hipStreamDestroy(stream);
    if (exchanged) (void)hipThreadExchangeStreamCaptureMode(&mode);
    (void)hipGetLastError();
  }
};

int probe_dispatch(int cus, long long* checked, long long* wrong) {
  const long long wgs = 5LL * cus - cus / 8 - 2, nwaves = 2 * wgs;  // five workgroups on most CUs, four on the rest (1250 on 256 CUs)
  std::vector<unsigned long long> rec((size_t)nwaves, 0ull);
  ProbeScope ps;
  hipError_t e = ps.open((size_t)nwaves * sizeof(unsigned long long));
  // (26 KiB of dynamic LDS per workgroup: six workgroups = three waves per SIMD fit a CU, the NL kernel's own occupancy -- a probe
  //  that could pile more waves on a SIMD is placed differently)
  // twice: the first launch of a kernel in a process loads its code object while its first workgroups already run and leave -- its
  // placement says nothing (measured: 384 of 2492 waves off on the first launch, 0 on every later one)
  for (int rep = 0; rep < 2 && e == hipSuccess; ++rep)
    hipLaunchKernelGGL(dispatch_probe_kernel, dim3((unsigned)wgs), dim3(kBlock), 26 * 1024, ps.stream, ps.dev);
  if (e == hipSuccess) e = ps.fetch(rec.data(), (size_t)nwaves * sizeof(unsigned long long));
  if (e != hipSuccess) { g_err = std::string("dispatch probe: ") + hipGetErrorString(e); return (int)e; }
  // waves of the launch per SIMD, from the hardware's record: XCC_ID[3:0] | HW_ID: se [15:13], sh [12], cu [11:8], simd [5:4]
  std::vector<unsigned long long> key((size_t)nwaves);
  for (long long w = 0; w < nwaves; ++w) key[w] = ((rec[w] >> 32) & 0xfull) << 16 | (rec[w] & 0xff30ull);
  std::vector<unsigned long long> sorted(key);
  std::sort(sorted.begin(), sorted.end());
  *checked = nwaves; *wrong = 0;
  const long long q = wgs / cus, r = wgs % cus;
  for (long long w = 0; w < nwaves; ++w) {
    const long long i = w / 2, c = i % cus, j = i / cus;
    unsigned mine = 0, most = 0;
    simd_population((unsigned)(q + (c < r ? 1 : 0)), (unsigned)j, (unsigned)(w & 1), mine, most);
    const auto range = std::equal_range(sorted.begin(), sorted.end(), key[w]);
    if ((long long)(range.second - range.first) != (long long)mine) ++*wrong;
  }
  return 0;
}

// LDS per workgroup that lets exactly `per_cu` workgroups of the probe share a CU (asked of the runtime, not assumed); 0 = none found
size_t pace_probe_lds(int per_cu) {
  if (per_cu < 1 || per_cu > 8) return 0;
  const size_t cands[] = {(size_t)(160 * 1024) / (size_t)per_cu, (size_t)(128 * 1024) / (size_t)per_cu, (size_t)(64 * 1024) / (size_t)per_cu};
  for (size_t lds : cands) {
    lds &= ~(size_t)1023;
    if (lds == 0) continue;
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute((const void*)pace_probe_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
      (void)hipGetLastError();
      continue;
    }
    int got = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&got, (const void*)pace_probe_kernel, kBlock, lds) != hipSuccess) { (void)hipGetLastError(); continue; }
    if (got == per_cu) return lds;
  }
  return 0;
}

// *checked = workgroups of the probe launch, *wrong = workgroups off the rule (or that started late); returns 0, a hipError_t, or
// CLOUDSC2_EINVAL when no probe of that shape can be built (then there is no verdict and no pacing)
int probe_pace(int cus, int per_cu, long long* checked, long long* wrong) {
  const size_t lds = pace_probe_lds(per_cu);
  if (!lds) return fail(CLOUDSC2_EINVAL, "pace probe: no LDS size gives the probe this many workgroups per CU");
  const long long slots = (long long)cus * per_cu, k = 2, rem = slots * 113 / 256, wgs = k * slots + rem;  // 512 slots: 1250 workgroups, 226 fast
  if (rem < 1) return fail(CLOUDSC2_EINVAL, "pace probe: device too small");
  std::vector<unsigned long long> rec((size_t)(2 * wgs), 0ull);
  ProbeScope ps;
  hipError_t e = ps.open(rec.size() * sizeof(unsigned long long));
  for (int rep = 0; rep < 2 && e == hipSuccess; ++rep)  // (twice: see probe_dispatch)
    hipLaunchKernelGGL(pace_probe_kernel, dim3((unsigned)wgs), dim3(kBlock), lds, ps.stream, ps.dev, (unsigned)slots, (unsigned)rem);
  if (e == hipSuccess) e = ps.fetch(rec.data(), rec.size() * sizeof(unsigned long long));
  if (e != hipSuccess) { g_err = std::string("pace probe: ") + hipGetErrorString(e); return (int)e; }
  *checked = wgs; *wrong = 0;
  // (a) the whole first round resident at once: started before the first workgroup can have left
  unsigned long long t_min = ~0ull;
  for (long long b = 0; b < wgs; ++b) t_min = std::min(t_min, rec[2 * b]);
  for (long long b = 0; b < slots; ++b)
    if (rec[2 * b] - t_min >= kPaceProbeFastTicks / 2) ++*wrong;
  // (b) per CU (XCC_ID[3:0] | HW_ID se [15:13], sh [12], cu [11:8]): the classes it received in the first round decide what it runs later
  struct CuCount { long long fast1 = 0, slow1 = 0, fast = 0, slow = 0; };
  std::vector<std::pair<unsigned long long, CuCount>> cu_tab;
  auto at = [&](unsigned long long key) -> CuCount& {
    for (auto& c : cu_tab) if (c.first == key) return c.second;
    cu_tab.emplace_back(key, CuCount());
    return cu_tab.back().second;
  };
  for (long long b = 0; b < wgs; ++b) {
    const unsigned long long key = ((rec[2 * b + 1] >> 32) & 0xfull) << 16 | (rec[2 * b + 1] & 0xff00ull);
    CuCount& c = at(key);
    const bool fast = (b % slots) < rem;
    (fast ? c.fast : c.slow) += 1;
    if (b < slots) (fast ? c.fast1 : c.slow1) += 1;
  }
  if ((long long)cu_tab.size() != cus) *wrong += std::llabs((long long)cu_tab.size() - cus) * per_cu;
  for (auto& c : cu_tab) {
    if (c.second.fast1 + c.second.slow1 != per_cu) *wrong += std::llabs(c.second.fast1 + c.second.slow1 - per_cu);
    *wrong += std::llabs(c.second.fast - (k + 1) * c.second.fast1) + std::llabs(c.second.slow - k * c.second.slow1);
  }
  return 0;
}

// cached verdicts: 1 = holds, 0 = does not; absent = never probed (or the probe itself failed)
struct DeviceRules {
  int device;
  int nl_rule = -1;
  std::vector<std::pair<int, int>> pace;  // (workgroups per CU, verdict)
  int pace_of(int per_cu) const {
    for (auto& p : pace) if (p.first == per_cu) return p.second;
    return -1;
  }
};
std::mutex g_rule_mutex;
std::vector<DeviceRules> g_rules;

// read-only, for the launchers: nothing here touches the device.  (NL nap verdict, pacing verdict at `per_cu` workgroups per CU)
std::pair<int, int> cached_rules(int device, int per_cu) {
  std::lock_guard<std::mutex> lock(g_rule_mutex);
  for (auto& e : g_rules) if (e.device == device) return {e.nl_rule, e.pace_of(per_cu)};
  return {-1, -1};
}

// The registry: the host's columns of the table in cloudsc2_sweep_kernels.hpp, one entry per variant table (pure host: the tables
// themselves are the family units')
struct KernelTable {
  int family;      // cloudsc2_variant_built's and the launch log's number, or kNone
  int kernel;      // cloudsc2_kernel_occupancy's number, or kNone
  bool paced;      // device_prepare probes the pacing rule at its kernels' occupancies
  unsigned slots;  // words 0 .. slots-1
  const void* (*entry)(unsigned word);
};
#define C2_REGISTER(name, Args, slots, valid, family, kernel, paced) \
  {family, kernel, paced, slots, [](unsigned word) { return (const void*)name##_variant(word); }},
constexpr KernelTable kTables[] = {C2_KERNEL_TABLES(C2_REGISTER)};
#undef C2_REGISTER
constexpr bool families_numbered() {  // every number 0 .. kFamCount-1 names exactly one table
  for (int family = 0; family < kFamCount; ++family) {
    int n = 0;
    for (const KernelTable& t : kTables) n += t.family == family;
    if (n != 1) return false;
  }
  for (const KernelTable& t : kTables)
    if (t.family != kNone && (t.family < 0 || t.family >= kFamCount)) return false;
  return true;
}
static_assert(families_numbered(), "the rows' family numbers are enum SweepFamily's: 0 .. kFamCount-1, each once");
// the entry of the one table whose column `number` (&KernelTable::family or ::kernel) holds `id`; nullptr: no such table, word not built
const void* table_entry(int KernelTable::*number, int id, unsigned word) {
  if (id != kNone)
    for (const KernelTable& t : kTables)
      if (t.*number == id) return t.entry(word);
  return nullptr;
}

// workgroups per CU of every TL / AD variant that a launch may pace (their occupancy, asked of the runtime), distinct: every slot of
// the paced tables (occupancy_known skips one that is not built)
std::vector<int> paced_kernel_occupancies() {
  std::vector<int> out;
  for (const KernelTable& t : kTables) {
    if (!t.paced) continue;
    for (unsigned word = 0; word < t.slots; ++word) {
      Occupancy o;
      if (occupancy_known(t.entry(word), &o) && std::find(out.begin(), out.end(), o.per_cu) == out.end()) out.push_back(o.per_cu);
    }
  }
  return out;
}

// The rule itself (pure arithmetic; cloudsc2_pace_plan exposes it to the tests): `wgs` workgroups on `slots` slots.
// Returns false = not paced.
bool pace_plan(long long wgs, long long slots, int* first, int* recip_q16) {
  if (slots <= 0 || wgs <= 0) return false;
  const long long k = wgs / slots, rem = wgs % slots;
  // Where it pays (profiles/r04_pacing_ab.txt, TL / AD in % of time; k whole rounds, f = the partial round's share of the slots):
  //   k 2 f 0.14: -7.7 / -6.0   k 2 f 0.44 (160 000 columns): -4.9 / -7.6   k 3 f 0.05: -7.6 / -8.0   k 5 f 0.04: -1.7 / -7.1
  //   k 6 f 0.10: -0.9 / -6.9   but k 1 f 0.53: +2.3 / +2.8   k 1 f 0.83: +1.8 / +0.5   k 2 f 0.75: +1.9 / +0.5
  //   k 3 f 0.82: +1.3 / +0.7   k 4 f 0.58: +2.6 / -1.8
  // i.e. at least two whole rounds and a partial round that leaves half of the machine or more idle; beyond eight rounds the
  // imbalance is a few per cent of the launch and the sweeps are left alone.  The nap is 1/k of a level.
  if (k < 2 || k > 8 || rem == 0 || (double)rem > 0.5 * (double)slots) return false;
  *first = (int)rem;
  *recip_q16 = (int)(65536.0 / (double)k);
  return true;
}

// One-round NL launches: the lighter SIMDs of the fullest CUs yield (struct Pace: begin_light).  On only where every premise of
// simd_population holds for THIS launch: the variant really runs three waves per SIMD (six workgroups per CU: its own occupancy --
// the evaporation variants run two and are left alone), all workgroups are resident at once, the fullest CUs carry unequal numbers
// of waves on their SIMDs (2 x workgroups not a multiple of 4: otherwise nobody would nap and the launch is the plain one), the
// device is this process's alone, and its dispatcher was seen to follow the rule (cached verdict of device_prepare; never probed here).
void light_nap(Geom& g, long long wgs, const Occupancy& o) {
  const int nl_light = knobs().nl_light;
  if (nl_light <= 0 || kBlock != 128 || o.per_cu != 6 || wgs > (long long)o.cus * o.per_cu) return;
  const long long q = wgs / o.cus, r = wgs % o.cus, fullest = q + (r ? 1 : 0);
  if ((2 * fullest) % 4 == 0) return;  // equal SIMD loads in the CUs the launch ends with
  if (cached_rules(o.dev, 0).first != 1) return;  // (a shared device is recorded as "rule off" by device_prepare)
  g.pace_slots = o.cus; g.pace_first = (int)q; g.pace_recip_q16 = (int)(65536.0 * nl_light / 100.0);
  g.fair |= 4 | ((int)r << 8);
}

// Pacing of a TL / AD launch (cloudsc2_column.hpp: struct Pace): on when the launch is two to eight whole rounds of workgroups on the
// slots the device has for THIS kernel (its occupancy) plus a partial round that fills at most half of them -- and the device's
// dispatcher was seen to behave as the rule needs (probe_pace above; read from the cache here, never probed from a launch).
void pace(Geom& g, long long wgs, const Occupancy& o) {
  const long long slots = (long long)o.cus * o.per_cu;
  int first = 0, recip = 0;
  if (!pace_plan(wgs, slots, &first, &recip)) return;
  const int rule = cached_rules(o.dev, o.per_cu).second;
  if (rule != 1) {
    static std::atomic<int> told{0};
    if (knobs().verbose && told.fetch_add(1) < 4)
      fprintf(stderr, "cloudsc2: launch of %lld workgroups on %lld slots NOT paced: %s\n", wgs, slots,
              rule == 0 ? "the pace probe found this device's dispatcher off the rule" : "device not prepared (cloudsc2_device_prepare)");
    return;
  }
  g.pace_slots = (int)slots; g.pace_first = first; g.pace_recip_q16 = recip;
  if (knobs().verbose)
    fprintf(stderr, "cloudsc2: launch of %lld workgroups on %lld slots paced: %lld whole rounds + %d workgroups; the other %lld slots nap 1/%lld of every level\n",
            wgs, slots, wgs / slots, first, slots - first, wgs / slots);
}

}  // namespace

namespace cloudsc2 {

// `fair`: should the waves of this launch yield to each other by progress (cloudsc2_column.hpp: progress_priority)?  Yes when the launch
// is ONE round of waves of a kernel that runs several waves per SIMD: no more workgroups than the device holds at THIS variant's own
// occupancy (the plain and, since their block runs in fast arithmetic, the evaporation NL variants hold six workgroups = three waves
// per SIMD; a variant that holds one wave per SIMD has nothing to keep abreast).  Measured (profiles/r03_wave_times.txt): 100 000
// ... 190 000 columns -1 ... -4 % (160 000: 0.815 -> 0.783 ms), 65 536 -3 %, 196 608 (exactly 3 per SIMD) +-1 %; the evaporation
// variant 160 000: 0.842 -> 0.785 ms, 100 000 -3 %, 65 536 -5 % (profiles/r05_evap_fast_ab.txt); with more than one round the age
// order is better (262 144 columns +4 %, 1 M +2 %): off there.
void schedule(Geom& g, const void* fair, bool nap, const void* pace_fn) {
  g.fair = 0;
  g.pace_slots = g.pace_first = g.pace_recip_q16 = 0;
  const long long wgs = (g.ncols_pad + kBlock - 1) / kBlock;
  Occupancy o;
  if (fair && occupancy_known(fair, &o)) {
    g.fair = o.per_cu >= 4 && wgs <= (long long)o.per_cu * o.cus;  // (fewer than four workgroups per CU: one wave per SIMD)
    if (nap && g.fair) light_nap(g, wgs, o);
  }
  // (a device that other processes use at the same time: the slots are not this launch's alone, the rule's premise is gone)
  if (pace_fn && !knobs().pace_off && !device_is_shared() && occupancy_known(pace_fn, &o)) pace(g, wgs, o);
}

// The synchronous moment.  Idempotent and cheap after the first call on a device (one mutex, one table lookup).  A dispatch probe that
// ends in a HIP error leaves no verdict, and the next call probes the device again; once the dispatch probe has a verdict the device
// counts as prepared, and a pace probe that ended in a HIP error is not repeated: that occupancy stays without a verdict (unpaced).
int device_prepare() {
  static std::mutex one_at_a_time;  // (two threads probing one device at once would disturb each other's placement)
  std::lock_guard<std::mutex> serial(one_at_a_time);
  int dev = 0, cus = 0;
  if (current_cus(&dev, &cus) != hipSuccess || cus <= 0) {
    (void)hipGetLastError();
    return 0;  // (the callers' own HIP calls report what is wrong with the device)
  }
  {
    std::lock_guard<std::mutex> lock(g_rule_mutex);
    for (auto& e : g_rules)
      if (e.device == dev && e.nl_rule >= 0) return 0;  // prepared (pace verdicts are taken in the same pass)
  }
  const Knobs& kn = knobs();
  DeviceRules r;
  r.device = dev;
  if (device_is_shared()) {  // the slots are not one launch's alone: both rules' premise is gone, nothing to probe
    r.nl_rule = 0;
  } else {
    long long checked = 0, wrong = 0;
    if (kn.nl_light == 0) r.nl_rule = 0;
    else if (probe_dispatch(cus, &checked, &wrong) == 0) {
      r.nl_rule = wrong == 0 ? 1 : 0;
      if (kn.verbose)
        fprintf(stderr, "cloudsc2: dispatch probe on device %d: %lld of %lld waves sit on a SIMD with the predicted number of waves -> the lighter SIMDs' nap is %s\n",
                dev, checked - wrong, checked, r.nl_rule ? "on" : "off");
    } else if (kn.verbose) fprintf(stderr, "cloudsc2: dispatch probe on device %d failed (%s): no verdict, no nap\n", dev, g_err.c_str());
    if (!kn.pace_off) {
      for (int per_cu : paced_kernel_occupancies()) {
        const int rc = probe_pace(cus, per_cu, &checked, &wrong);
        if (rc == 0) r.pace.emplace_back(per_cu, wrong == 0 ? 1 : 0);
        if (kn.verbose) {
          if (rc == 0)
            fprintf(stderr, "cloudsc2: pace probe on device %d, %d workgroup(s) per CU: %lld of %lld workgroups ran where blockIdx mod slots says -> TL / AD pacing is %s\n",
                    dev, per_cu, checked - wrong, checked, wrong == 0 ? "on" : "off");
          else fprintf(stderr, "cloudsc2: pace probe on device %d, %d workgroup(s) per CU: no verdict (%s), no pacing\n", dev, per_cu, g_err.c_str());
        }
      }
    }
  }
  if (r.nl_rule < 0) return 0;  // the dispatch probe itself failed: ask again at the next synchronous moment
  std::lock_guard<std::mutex> lock(g_rule_mutex);
  for (auto& e : g_rules)
    if (e.device == dev) { e = r; return 0; }
  g_rules.push_back(r);
  return 0;
}

const void* variant_entry(int family, unsigned word) { return table_entry(&KernelTable::family, family, word); }

}  // namespace cloudsc2

extern "C" {

int cloudsc2_simd_population(long long workgroups, int cus, long long block, int wave_in_block, int* mine, int* most) {
  if (workgroups < 1 || cus < 1 || block < 0 || block >= workgroups || wave_in_block < 0 || wave_in_block > 1 || !mine || !most)
    return fail(CLOUDSC2_EINVAL, "cloudsc2_simd_population: bad argument");
  const long long q = workgroups / cus, r = workgroups % cus, c = block % cus, j = block / cus;
  unsigned a = 0, b = 0;
  simd_population((unsigned)(q + (c < r ? 1 : 0)), (unsigned)j, (unsigned)wave_in_block, a, b);
  *mine = (int)a; *most = (int)b;
  return 0;
}

int cloudsc2_dispatch_probe(long long* waves_checked, long long* waves_wrong) {
  if (!waves_checked || !waves_wrong) return fail(CLOUDSC2_EINVAL, "cloudsc2_dispatch_probe: NULL argument");
  if (int rc = require_device()) return rc;
  int dev = 0, cus = 0;
  HIP_TRY(current_cus(&dev, &cus));
  return probe_dispatch(cus, waves_checked, waves_wrong);
}

int cloudsc2_pace_probe(int workgroups_per_cu, long long* workgroups_checked, long long* workgroups_wrong) {
  if (!workgroups_checked || !workgroups_wrong) return fail(CLOUDSC2_EINVAL, "cloudsc2_pace_probe: NULL argument");
  if (int rc = require_device()) return rc;
  int dev = 0, cus = 0;
  HIP_TRY(current_cus(&dev, &cus));
  return probe_pace(cus, workgroups_per_cu, workgroups_checked, workgroups_wrong);
}

int cloudsc2_device_prepare(void) {
  if (int rc = require_device()) return rc;
  return device_prepare();
}

int cloudsc2_device_rules(int workgroups_per_cu, int* nl_nap, int* pacing) {
  int dev = 0;
  if (!device_ok() || hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return no_device(); }
  const std::pair<int, int> r = cached_rules(dev, workgroups_per_cu);
  if (nl_nap) *nl_nap = r.first;
  if (pacing) *pacing = r.second;
  return 0;
}

int cloudsc2_kernel_occupancy(int kernel, int flags, int* workgroups_per_cu) {
  if (!workgroups_per_cu) return fail(CLOUDSC2_EINVAL, "cloudsc2_kernel_occupancy: NULL argument");
  if (int rc = require_device()) return rc;
  // (the registry's `kernel` column: families 0..6 under their own numbers, the sparse and column-sum tables under the header's)
  const void* fn = table_entry(&KernelTable::kernel, kernel, (unsigned)flags);
  if (!fn) return fail(CLOUDSC2_EINVAL, "cloudsc2_kernel_occupancy: no such kernel variant in this build");
  Occupancy o;
  HIP_TRY(occupancy(fn, &o));
  *workgroups_per_cu = o.per_cu;
  return 0;
}

int cloudsc2_variant_built(int family, unsigned flags) {
  if (family < 0 || family >= kFamCount) return fail(CLOUDSC2_EINVAL, "cloudsc2_variant_built: family must be 0..9");
  return variant_entry(family, flags) ? 1 : 0;
}

int cloudsc2_pace_plan(long long workgroups, long long slots, int* whole_rounds, int* fast_first, int* nap_recip_q16) {
  int first = 0, recip = 0;
  const bool on = pace_plan(workgroups, slots, &first, &recip);
  if (whole_rounds) *whole_rounds = slots > 0 ? (int)(workgroups / slots) : 0;
  if (fast_first) *fast_first = on ? first : 0;
  if (nap_recip_q16) *nap_recip_q16 = on ? recip : 0;
  return on ? 1 : 0;
}

}  // extern "C"
