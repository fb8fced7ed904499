// cloudsc2_alloc.hip -- device memory for the state: the placement allocator behind cloudsc2_device_malloc*.
//
// Why the library has its own allocator.  On MI355X, WRITE streams run 10-20 % slower into some parts of the HBM than into
// others (profiles/r02_hbm_placement.md; tools/hbm_probe.cpp, hbm_state.cpp, hbm_alloc2.cpp, hbm_vmm*.cpp):
//   * two persistent classes among 150 separate 1.4 GB allocations of one process (4.8 vs 5.7 TB/s for the NL sweep's plane
//     writes; 0.81 vs 0.96 ms for the whole NL kernel at 160 000 columns), in runs of neighbouring allocations (tens of GB),
//     different on every box; the class is a property of WHERE the memory is: it survives freeing everything else, and
//     fresh allocations that reuse a freed place inherit its class;
//   * every write pattern is affected, a plain contiguous 16-byte-per-lane fill included, so it is not the AoSoA layout
//     of B_LOC (plane-major output arrays measure the same two classes); reads do not care;
//   * the L2 -> fabric counters (TCC_EA0_WRREQ*, per channel) show equal request counts, equal mean write latency and no
//     extra credit stalls in the slow class -- fewer writes are in flight, nothing is visibly stuck;
//   * hipMalloc and hipMemCreate memory write alike in a stand-alone fill, but on memory mapped from hipMemCreate chunks a kernel's
//     time changes when another kernel rewrites the buffer (see device_malloc_impl) -- only hipMalloc memory can be placed.
// Hence the remedy is placement at the scale of the buffer, done here once per allocation instead of in every caller: for a large
// request the allocator makes several candidate hipMalloc allocations of the full size, times a sweep over each -- the caller's own
// (the NL kernel on a state laid out in the candidate: cloudsc2_device_malloc_state, cloudsc2_driver.hip state_probe) or two
// generic streams (the sweeps' write stream: 1 KiB rows of 5 of 8 planes, one workgroup per 1096 KiB block; and the NL sweep's
// whole read/write pattern) -- keeps the best and frees the others.
// Environment (measurements only): CLOUDSC2_PLACE=0 no search, CLOUDSC2_PLACE_SPAN_GB (96), CLOUDSC2_PLACE_CANDIDATES,
// CLOUDSC2_PLACE_PROBE=write|mixed|generic, CLOUDSC2_PLACE_MODE=chunks, CLOUDSC2_PLACE_VERBOSE=1.
// Footprint.  The search is TRANSIENT memory: candidates of the requested size, all freed but one before the call returns.  It is
// bounded by a share of the memory that is free when the call starts (60 %; 85 % for requests above 12 GiB, of which few fit; the
// second batch included) and by CLOUDSC2_PLACE_MAX_GB / CLOUDSC2_PLACE_MAX_SHARE where the host model sets them; nothing is searched
// (one plain hipMalloc) when several ranks share the device -- LOCAL_WORLD_SIZE above the number of visible devices, the shm
// rehearsal of libcloudsc2_comm.so, or CLOUDSC2_PLACE_SHARED=1 -- because hipMemGetInfo and hipMalloc are not coordinated between
// processes.  A search that cannot get a single candidate frees everything and retries one plain hipMalloc before reporting OOM.

#include <array>
#include "cloudsc2_host.hpp"

using namespace cloudsc2;

namespace {

struct DevAlloc {
  size_t bytes = 0;
  size_t chunk = 0;                                      // > 0: a reserved range backed by hipMemCreate chunks (composed mode)
  std::vector<hipMemGenericAllocationHandle_t> handles;
};
size_t env_gib(const char* name, size_t dflt) {
  const char* e = getenv(name);
  return (e && atoll(e) > 0) ? (size_t)atoll(e) : dflt;
}
std::mutex g_alloc_mutex;
std::vector<std::pair<void*, DevAlloc>> g_allocs;

// bytes the placement search may hold at once, given what is free now
size_t search_budget(size_t bytes, size_t free_b) {
  double share = bytes > (env_gib("CLOUDSC2_PLACE_WHOLE_MAX_GB", 12) << 30) ? 0.85 : 0.6;
  if (const char* e = getenv("CLOUDSC2_PLACE_MAX_SHARE")) { const double v = atof(e); if (v > 0.0 && v <= 1.0) share = v; }
  size_t budget = (size_t)(share * (double)free_b);
  const size_t cap = env_gib("CLOUDSC2_PLACE_MAX_GB", 0) << 30;
  if (cap) budget = std::min(budget, cap);
  return budget;
}

// the NL sweep's write stream into B_LOC: per 1096 KiB block, 137 rows of 1 KiB in planes 0,2,3,4,7 of 8
constexpr long long kProbeBlockBytes = 8LL * 137 * 128 * 8;
__global__ void __launch_bounds__(128) place_probe_kernel(double* base, long long nblocks) {
  const long long b = blockIdx.x;
  if (b >= nblocks) return;
  double* blk = base + b * (kProbeBlockBytes / 8) + threadIdx.x;
  for (int jk = 0; jk < 137; ++jk)
    for (int pl : {0, 2, 3, 4, 7}) __builtin_nontemporal_store(0.0, blk + (long long)pl * 137 * 128 + jk * 128);
}

// the NL sweep's whole memory pattern on a buffer taken as 27 planes of (128 columns, 138 levels, nblocks): one lane per column,
// 137 dependent levels, 16 planes read one level ahead (the first 16/27 of the buffer), 11 written (the rest), non-temporal
constexpr int kMixIn = 16, kMixOut = 11;
constexpr long long kMixBlockElems = 138LL * 128;
__global__ void __launch_bounds__(128) place_probe_mixed_kernel(double* base, long long nblocks) {
  const long long plane = nblocks * kMixBlockElems;
  const long long off = (long long)blockIdx.x * kMixBlockElems + threadIdx.x;
  const double* in = base + off;
  double* out = base + kMixIn * plane + off;
  double cur[kMixIn], nxt[kMixIn];
#pragma unroll
  for (int p = 0; p < kMixIn; ++p) cur[p] = __builtin_nontemporal_load(in + p * plane);
  double carry = 0.0;
#pragma unroll 1
  for (int jk = 0; jk < 137; ++jk) {
    if (jk + 1 < 137) {
#pragma unroll
      for (int p = 0; p < kMixIn; ++p) nxt[p] = __builtin_nontemporal_load(in + p * plane + (jk + 1) * 128);
    }
    double acc = carry;
#pragma unroll
    for (int p = 0; p < kMixIn; ++p) acc = fma(cur[p], 0.5, acc);
    carry = acc * 0.5;
#pragma unroll
    for (int q = 0; q < kMixOut; ++q) __builtin_nontemporal_store(acc, out + q * plane + jk * 128);
#pragma unroll
    for (int p = 0; p < kMixIn; ++p) cur[p] = nxt[p];
  }
}

// The probes of the placement search: kind 0 the sweeps' write stream, kind 1 the NL sweep's whole pattern.  Candidates that no
// caller's sweep judges are ranked by BOTH (the mixed stream's time plus a fifth of the write stream's, each relative to the best
// candidate's): on one box the NL kernel's time on 20 consecutive allocations of one process correlated 0.999 with the mixed probe (two clean classes, 1.10 vs 1.29 ms, noise < 1 %)
// and 0.93-0.96 with the write stream (0.70-0.74 vs 0.74-0.80 ms: a gap of 1 %, which costs misses); on another box the write
// stream saw no difference between 16 candidates and the kernel still came out at 0.81 or 0.96 ms; on a third the mixed probe's
// choice ran at 0.94 ms once while the write stream's choices did not miss (profiles/r02_placement/o_probe_vs_kernel.txt).
// CLOUDSC2_PLACE_PROBE=write|mixed ranks by one of them (measurements only).  2 GiB chunks of the composed form are ranked by the
// write stream alone (the mixed pattern inside one chunk says less about the composition: 4.96-5.04 vs 4.98-5.38 ms at 1 M columns).
// kProbeCustom: the caller's own sweep (a std::function that launches ONE pass over a buffer on the null stream).  The state-level
// allocations use it with the real NL kernel on a state laid out in the candidate (cloudsc2_driver.hip: state_probe): at 1 M
// columns neither generic stream predicts the kernel (correlation 0.5-0.8 over five 42 GB allocations; a composition that probed
// at 6.98 ms ran the kernel at 5.43 ms, one at 7.40 ms ran it at 4.87 ms: profiles/r02_placement/r_1m_probe_vs_kernel.txt).
enum ProbeKind { kProbeWrite = 0, kProbeMixed = 1, kProbeCustom = 2 };
const ProbeFn* g_custom_probe = nullptr;  // set for the duration of one device_malloc_impl call (under g_place_mutex)
std::mutex g_place_mutex;
void launch_probe(void* p, size_t bytes, int kind) {
  if (kind == kProbeCustom) { (*g_custom_probe)(p, bytes); return; }
  const long long nmix = (long long)(bytes / (size_t)((kMixIn + kMixOut) * kMixBlockElems * 8));
  if (kind == kProbeWrite || nmix < 1) {
    const long long nblocks = (long long)(bytes / (size_t)kProbeBlockBytes);
    if (nblocks > 0) hipLaunchKernelGGL(place_probe_kernel, dim3((unsigned)nblocks), dim3(128), 0, nullptr, (double*)p, nblocks);
  } else {
    hipLaunchKernelGGL(place_probe_mixed_kernel, dim3((unsigned)nmix), dim3(128), 0, nullptr, (double*)p, nmix);
  }
}
// median-of-3 probe times (after one untimed round that touches every buffer for the first time and brings the GPU out of idle) of
// `n` buffers of `bytes` each, buffer k at base(k)
template <class Base>
hipError_t probe_all(size_t n, size_t bytes, int kind, Base&& base, std::vector<double>& ms) {
  hipEvent_t ea = nullptr, eb = nullptr;
  hipError_t e = hipEventCreate(&ea);
  if (e == hipSuccess) e = hipEventCreate(&eb);
  std::vector<std::array<float, 3>> t(n);
  for (int rnd = 0; rnd < 4 && e == hipSuccess; ++rnd)
    for (size_t k = 0; k < n && e == hipSuccess; ++k) {
      (void)hipEventRecord(ea, nullptr);
      launch_probe(base(k), bytes, kind);
      (void)hipEventRecord(eb, nullptr);
      e = hipEventSynchronize(eb);
      float f = 0;
      if (e == hipSuccess) e = hipEventElapsedTime(&f, ea, eb);
      if (rnd > 0) t[k][rnd - 1] = f;
    }
  if (ea) (void)hipEventDestroy(ea);
  if (eb) (void)hipEventDestroy(eb);
  ms.assign(n, 0.0);
  for (size_t k = 0; k < n && e == hipSuccess; ++k) { std::sort(t[k].begin(), t[k].end()); ms[k] = t[k][1]; }
  return e;
}

struct PlaceStats { int candidates = 0; double best_ms = 0, median_ms = 0, worst_ms = 0; };
PlaceStats g_last_place;  // of the most recent placed allocation (cloudsc2_device_malloc_info)

// CLOUDSC2_PLACE_MODE=chunks: the buffer is COMPOSED of physical chunks (hipMemCreate, CLOUDSC2_PLACE_CHUNK_GB, default 2 GiB)
// mapped side by side (hipMemMap) into one address range.  Unlike whole-size candidates this also works for requests that are a
// large part of the memory (a 41 GB state: only 4 whole candidates fit).  A pool of chunks (3x the need, at least the span, within
// 85 % of the free memory) is created; every chunk is timed alone with the write stream; then COMPOSITIONS of the needed number of
// chunks are mapped one after the other and timed as a whole with both probes, like whole-size candidates: the chunks that are
// fastest one by one ("greedy": round 2's first form, which lands at 4.9-5.15 ms for NL at 1 M columns two times in three and at
// 5.7 ms otherwise -- single chunks do not predict the composition, the whole does, cf. launch_probe) and windows of consecutive
// chunks of the pool (neighbouring places, the analogue of whole-size candidates, but overlapping: many more of them fit).  The
// best composition stays mapped, the other chunks are released.  CLOUDSC2_PLACE_COMPOSE=greedy: the first form (measurements only).
int device_malloc_chunks(void** out, size_t bytes, PlaceStats& st) {
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  hipMemAllocationProp prop = {};
  prop.type = hipMemAllocationTypePinned;
  prop.location.type = hipMemLocationTypeDevice;
  prop.location.id = dev;
  hipMemAccessDesc acc = {};
  acc.location = prop.location;
  acc.flags = hipMemAccessFlagsProtReadWrite;
  DevAlloc a;
  a.chunk = env_gib("CLOUDSC2_PLACE_CHUNK_GB", 2) << 30;
  const size_t need = (bytes + a.chunk - 1) / a.chunk;
  a.bytes = need * a.chunk;
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  const size_t span = env_gib("CLOUDSC2_PLACE_SPAN_GB", 96) << 30;
  const size_t fit = (size_t)(0.85 * (double)free_b) / a.chunk;
  size_t cand = std::max(need, std::min(std::max(std::max(need + 8, (span + a.chunk - 1) / a.chunk), 3 * need), fit));  // >= 3x the need
  std::vector<hipMemGenericAllocationHandle_t> h;
  char* scratch = nullptr;
  const size_t scratch_bytes = cand * a.chunk;
  hipError_t e = hipMemAddressReserve((void**)&scratch, scratch_bytes, 1ull << 30, nullptr, 0);
  size_t mapped = 0;  // chunks mapped in `scratch`
  for (size_t k = 0; k < cand && e == hipSuccess; ++k) {
    hipMemGenericAllocationHandle_t x;
    e = hipMemCreate(&x, a.chunk, &prop, 0);
    if (e != hipSuccess) {
      if (k >= need) { e = hipSuccess; (void)hipGetLastError(); }  // fewer candidates than hoped for
      break;
    }
    h.push_back(x);
    e = hipMemMap(scratch + k * a.chunk, a.chunk, 0, x, 0);
    if (e == hipSuccess) ++mapped;
  }
  const size_t pool = h.size();
  if (e == hipSuccess && mapped >= need) e = hipMemSetAccess(scratch, mapped * a.chunk, &acc, 1);
  char* va = nullptr;
  size_t mapped2 = 0;  // chunks mapped in `va`
  auto bail = [&](hipError_t err) {
    (void)hipDeviceSynchronize();
    for (size_t k = 0; k < mapped2; ++k) (void)hipMemUnmap(va + k * a.chunk, a.chunk);
    for (size_t k = 0; k < mapped; ++k) (void)hipMemUnmap(scratch + k * a.chunk, a.chunk);
    for (auto x : h) (void)hipMemRelease(x);
    if (scratch) (void)hipMemAddressFree(scratch, scratch_bytes);
    if (va) (void)hipMemAddressFree(va, a.bytes);
    g_err = std::string("cloudsc2_device_malloc (composed): ") + hipGetErrorString(err);
    (void)hipGetLastError();
    return (int)err;
  };
  if (e != hipSuccess || mapped < need) return bail(e != hipSuccess ? e : hipErrorOutOfMemory);
  st.candidates = (int)pool;
  std::vector<std::vector<size_t>> comps;  // compositions, each in the chunks' order of creation
  if (pool > need) {
    std::vector<double> ms;
    e = probe_all(pool, a.chunk, kProbeWrite, [&](size_t k) { return (void*)(scratch + k * a.chunk); }, ms);
    if (e != hipSuccess) return bail(e);
    std::vector<size_t> order(pool);
    for (size_t k = 0; k < pool; ++k) order[k] = k;
    std::sort(order.begin(), order.end(), [&](size_t x, size_t y) { return ms[x] < ms[y]; });
    st.best_ms = ms[order[0]]; st.median_ms = ms[order[pool / 2]]; st.worst_ms = ms[order[pool - 1]];
    std::vector<size_t> greedy(order.begin(), order.begin() + need);
    std::sort(greedy.begin(), greedy.end());
    comps.push_back(greedy);
    static const char* how = getenv("CLOUDSC2_PLACE_COMPOSE");
    if (!(how && !strcmp(how, "greedy"))) {
      const size_t stride = std::max<size_t>(1, need / 5);
      for (size_t s0 = 0; s0 + need <= pool; s0 += stride) {
        std::vector<size_t> w(need);
        for (size_t j = 0; j < need; ++j) w[j] = s0 + j;
        comps.push_back(w);
      }
    }
  } else {
    std::vector<size_t> all(need);
    for (size_t j = 0; j < need; ++j) all[j] = j;
    comps.push_back(all);
  }
  if ((e = hipDeviceSynchronize()) != hipSuccess) return bail(e);
  for (size_t k = 0; k < mapped; ++k) (void)hipMemUnmap(scratch + k * a.chunk, a.chunk);
  mapped = 0;
  (void)hipMemAddressFree(scratch, scratch_bytes);
  scratch = nullptr;
  e = hipMemAddressReserve((void**)&va, a.bytes, 1ull << 30, nullptr, 0);
  if (e != hipSuccess) return bail(e);
  auto map_comp = [&](const std::vector<size_t>& c) {
    hipError_t r = hipSuccess;
    for (size_t j = 0; j < need && r == hipSuccess; ++j) {
      r = hipMemMap(va + j * a.chunk, a.chunk, 0, h[c[j]], 0);
      if (r == hipSuccess) ++mapped2;
    }
    if (r == hipSuccess) r = hipMemSetAccess(va, a.bytes, &acc, 1);
    return r;
  };
  auto unmap_comp = [&]() {
    (void)hipDeviceSynchronize();
    for (size_t j = 0; j < mapped2; ++j) (void)hipMemUnmap(va + j * a.chunk, a.chunk);
    mapped2 = 0;
  };
  size_t best = 0;
  if (comps.size() > 1) {
    std::vector<double> msm(comps.size(), 0.0), msw(comps.size(), 0.0);
    for (size_t c = 0; c < comps.size(); ++c) {
      if ((e = map_comp(comps[c])) != hipSuccess) return bail(e);
      std::vector<double> one;
      if (g_custom_probe) {  // the caller's sweep is the only judge; cleared first, so that all compositions run the same path
        (void)hipMemsetAsync(va, 0, a.bytes, nullptr);
        e = probe_all(1, a.bytes, kProbeCustom, [&](size_t) { return (void*)va; }, one);
        if (e != hipSuccess) return bail(e);
        msm[c] = msw[c] = one[0];
      } else {
        e = probe_all(1, a.bytes, kProbeMixed, [&](size_t) { return (void*)va; }, one);
        if (e == hipSuccess) { msm[c] = one[0]; e = probe_all(1, a.bytes, kProbeWrite, [&](size_t) { return (void*)va; }, one); }
        if (e != hipSuccess) return bail(e);
        msw[c] = one[0];
      }
      unmap_comp();
    }
    const double lom = *std::min_element(msm.begin(), msm.end()), low = *std::min_element(msw.begin(), msw.end());
    std::vector<double> score(comps.size());
    for (size_t c = 0; c < comps.size(); ++c) {
      score[c] = msm[c] / lom + msw[c] / low;
      if (score[c] < score[best]) best = c;
    }
    if (getenv("CLOUDSC2_PLACE_VERBOSE")) {
      fprintf(stderr, "cloudsc2_device_malloc (composed): %zu bytes = %zu chunks of a pool of %zu; compositions (first = fastest single chunks, then windows "
                      "of consecutive chunks), probe ms %s:", bytes, need, pool, g_custom_probe ? "of the caller's sweep (twice)" : "mixed/write");
      for (size_t c = 0; c < comps.size(); ++c) fprintf(stderr, " %s%.3f/%.3f", c == best ? "*" : "", msm[c], msw[c]);
      fprintf(stderr, "\n");
    }
  }
  if ((e = map_comp(comps[best])) != hipSuccess) return bail(e);
  std::vector<char> kept(pool, 0);
  for (size_t k : comps[best]) { kept[k] = 1; a.handles.push_back(h[k]); }
  for (size_t k = 0; k < pool; ++k) if (!kept[k]) (void)hipMemRelease(h[k]);
  if (getenv("CLOUDSC2_PLACE_VERBOSE") && comps.size() > 1) {  // does the choice still probe the same once the others are gone?
    double m = 0.0, w = 0.0;
    (void)cloudsc2_device_probe(va, a.bytes, kProbeMixed, 3, &m);
    (void)cloudsc2_device_probe(va, a.bytes, kProbeWrite, 3, &w);
    std::vector<double> one(1, 0.0);
    if (g_custom_probe) (void)probe_all(1, a.bytes, kProbeCustom, [&](size_t) { return (void*)va; }, one);
    fprintf(stderr, "cloudsc2_device_malloc (composed): the chosen composition mapped again, the other chunks released: mixed %.3f write %.3f caller's sweep %.3f ms\n", m, w, one[0]);
  }
  std::lock_guard<std::mutex> lock(g_alloc_mutex);
  g_allocs.emplace_back((void*)va, a);
  g_last_place = st;
  *out = va;
  return 0;
}

std::atomic<long long> g_searches{0}, g_plain_allocs{0};  // cloudsc2_device_malloc_counts (tests: who searched, who did not)

}  // namespace

namespace cloudsc2 {

// do other processes allocate on this device at the same time?  (more local ranks than visible devices, or said so; read once)
bool device_is_shared() {
  static const bool shared = [] {
    const char* sh = getenv("CLOUDSC2_PLACE_SHARED");
    if (sh) return atoi(sh) != 0;
    const char* comm = getenv("CLOUDSC2_COMM");
    if (comm && !strcmp(comm, "shm")) return true;  // rehearsal transport: more ranks than GPUs by construction
    const char* lws = getenv("LOCAL_WORLD_SIZE");
    int ndev = 0;
    if (lws && hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0) return atoi(lws) > ndev;
    return false;
  }();
  return shared;
}

// `policy`: kPlaceSearch = the search described above (resident states and what callers ask for through cloudsc2_device_malloc*);
// kPlaceOnRequest = one plain hipMalloc unless CLOUDSC2_PLACE=1 is set explicitly (the workspace of the host-array drivers, whose
// calls are PCIe-bound: 55-71 ms per call against a 0.1 ms difference of the kernel, and a host model's HBM is not ours to take
// transiently); kPlacePlain = never searched (staging buffers touched once per transfer).
int device_malloc_impl(void** out, size_t bytes, const ProbeFn* custom, PlacePolicy policy) {
  if (!out) return fail(CLOUDSC2_EINVAL, "cloudsc2_device_malloc: NULL result pointer");
  *out = nullptr;
  if (bytes == 0) return 0;
  std::lock_guard<std::mutex> place_lock(g_place_mutex);  // one placement search at a time (they time the device)
  static const bool allow_custom = !(getenv("CLOUDSC2_PLACE_PROBE") && strcmp(getenv("CLOUDSC2_PLACE_PROBE"), "kernel") != 0);
  struct Scope { Scope(const ProbeFn* f) { g_custom_probe = f; } ~Scope() { g_custom_probe = nullptr; } } scope(allow_custom ? custom : nullptr);
  if (int rc = require_device()) return rc;
  // an allocation is a synchronous moment: the device's dispatch rules are checked here (once per device and process), BEFORE the
  // placement search times the NL sweep -- which then runs with the nap the launches will run with
  (void)device_prepare();
  // how many candidates: see below, never more than fit 60 % of the free memory; requests below 256 MiB are not placed (their
  // share of any sweep's writes is small)
  static const bool place_env_off = getenv("CLOUDSC2_PLACE") && atoi(getenv("CLOUDSC2_PLACE")) == 0;
  static const bool place_env_on = getenv("CLOUDSC2_PLACE") && atoi(getenv("CLOUDSC2_PLACE")) != 0;
  const bool place = policy == kPlaceSearch ? !place_env_off : (policy == kPlaceOnRequest ? place_env_on : false);
  // Which search: whole-size hipMalloc candidates, always.  The composed form (CLOUDSC2_PLACE_MODE=chunks) was built for requests of
  // which only a few whole candidates fit (the 41 GB state of 1 M columns: 4) and is kept for measurements only: on memory mapped
  // from hipMemCreate chunks the NL kernel's time CHANGES when another kernel rewrites the buffer (5.04 -> 5.95 ms, 5.43 -> 4.88 ms
  // across the zero-fill of the state, profiles/r02_placement/s_composed_memory_is_unstable.txt), so no probe can predict it
  // (5.88 / 5.69 / 4.90 / 5.83 / 5.47 ms in fresh processes); on hipMalloc memory it does not change, and the NL sweep's time on a
  // candidate is the kernel's time on the state later to 0.5 % (4.99 / 5.13 / 4.92 / 5.01 / 5.08 ms, the best of 4 candidates each).
  static const char* mode = getenv("CLOUDSC2_PLACE_MODE");
  const bool chunks = mode && !strcmp(mode, "chunks");
  if (place && chunks && bytes >= (256u << 20)) {
    PlaceStats stc;
    return device_malloc_chunks(out, bytes, stc);
  }
  size_t ncand = 1, budget = 0;
  if (place && bytes >= (256u << 20) && !device_is_shared()) {
    // The classes come in runs of neighbouring allocations tens of GB long, and consecutive hipMallocs are neighbours: what
    // matters is how much memory the candidates span together, not how many they are.  Default: enough candidates to span
    // 96 GiB (at least 12, at most 64).
    const char* ec = getenv("CLOUDSC2_PLACE_CANDIDATES");
    const size_t span = env_gib("CLOUDSC2_PLACE_SPAN_GB", 96) << 30;
    const size_t want = (ec && atoi(ec) > 0) ? (size_t)atoi(ec) : std::min<size_t>(64, std::max<size_t>(12, (span + bytes - 1) / bytes));
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    // never more than the search's budget: 60 % of the free memory, 85 % for requests above 12 GiB, of which few fit anyway; less
    // where the host model says so (search_budget)
    budget = search_budget(bytes, free_b);
    ncand = std::max<size_t>(1, std::min(want, budget / bytes));
  }
  std::vector<void*> cand;
  auto grow = [&](size_t n) {  // n more candidates; fewer when the memory does not give them
    for (size_t k = 0; k < n; ++k) {
      void* p = nullptr;
      if (hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); break; }
      cand.push_back(p);
    }
  };
  grow(ncand);
  if (cand.empty()) {  // not even one: let pending frees land, then one plain request before giving up
    (void)hipDeviceSynchronize();
    grow(1);
  }
  if (cand.empty()) { g_err = "cloudsc2_device_malloc: hipMalloc: out of memory"; return (int)hipErrorOutOfMemory; }
  size_t best = 0;
  PlaceStats st;
  if (cand.size() > 1) {
    static const char* pk = getenv("CLOUDSC2_PLACE_PROBE");
    const bool generic = !g_custom_probe;
    const bool use_write = generic && (!pk || strcmp(pk, "mixed") != 0), use_mixed = generic && (!pk || strcmp(pk, "write") != 0);
    std::vector<double> msw, msm;
    hipError_t e = hipSuccess;
    // probes candidates [first, cand.size()) and appends their times
    auto probe_from = [&](size_t first) {
      const size_t n = cand.size() - first;
      auto base = [&](size_t k) { return cand[first + k]; };
      std::vector<double> m, w;
      if (!generic) {  // the caller's sweep is the only judge; every candidate cleared first, so that all run the same path
        for (size_t k = first; k < cand.size() && e == hipSuccess; ++k) e = hipMemsetAsync(cand[k], 0, bytes, nullptr);
        if (e == hipSuccess) e = probe_all(n, bytes, kProbeCustom, base, m);
      }
      if (use_mixed) e = probe_all(n, bytes, kProbeMixed, base, m);
      if (use_write && e == hipSuccess) e = probe_all(n, bytes, kProbeWrite, base, w);
      msm.insert(msm.end(), m.begin(), m.end());
      msw.insert(msw.end(), w.begin(), w.end());
    };
    probe_from(0);
    // No class difference among the candidates (all within 4 %): they are all fast -- or all slow (seen: AD's 11 GB arena on a box
    // whose first 135 GB had no fast place, 3.31 instead of 3.04 ms).  One more batch, with the first still allocated so that it
    // lands elsewhere, tells which; it costs ~50 ms on the many boxes where everything is fast.
    if (e == hipSuccess) {
      const std::vector<double>& v = msm.empty() ? msw : msm;
      const double lo = *std::min_element(v.begin(), v.end()), hi = *std::max_element(v.begin(), v.end());
      size_t free_b = 0, total_b = 0;
      if (hi < 1.04 * lo && hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
        const size_t first = cand.size();
        const size_t held = first * bytes, left = budget > held ? budget - held : 0;  // both batches share the search's budget
        grow(std::min(first, std::min((size_t)(0.7 * (double)free_b), left) / bytes));
        if (cand.size() > first) probe_from(first);
      }
    }
    if (e != hipSuccess) {
      for (auto p : cand) (void)hipFree(p);
      g_err = std::string("cloudsc2_device_malloc: placement probe: ") + hipGetErrorString(e);
      (void)hipGetLastError();
      return (int)e;
    }
    // score: the mixed stream's time relative to the best candidate's, plus a fifth of the same for the write stream -- the mixed
    // stream separates the classes by 15-20 % with < 1 % noise, the write stream by 5-8 % with 2-3 % noise, and with equal weights a
    // half-slow candidate (mixed 1.88 where clean ones had 1.78) once won on its write time (TL 1.84 ms instead of 1.65)
    std::vector<double> score(cand.size(), 0.0);
    for (auto* v : {&msw, &msm})
      if (!v->empty()) {
        const double lo = *std::min_element(v->begin(), v->end());
        const double weight = (v == &msw && !msm.empty()) ? 0.2 : 1.0;
        for (size_t k = 0; k < cand.size(); ++k) score[k] += weight * (*v)[k] / lo;
      }
    for (size_t k = 0; k < cand.size(); ++k)
      if (score[k] < score[best]) best = k;
    if (getenv("CLOUDSC2_PLACE_VERBOSE")) {
      fprintf(stderr, "cloudsc2_device_malloc: %zu bytes, %zu candidates, probe ms %s/write:", bytes, cand.size(), generic ? "mixed" : "of the caller's sweep");
      for (size_t k = 0; k < cand.size(); ++k)
        fprintf(stderr, " %s%.4f/%.4f", k == best ? "*" : "", msm.empty() ? 0.0 : msm[k], msw.empty() ? 0.0 : msw[k]);
      fprintf(stderr, "\n");
    }
    std::vector<double> s = msm.empty() ? msw : msm;  // reported: the mixed probe's times when it ran
    st.best_ms = s[best];
    std::sort(s.begin(), s.end());
    st.median_ms = s[s.size() / 2]; st.worst_ms = s.back();
    for (size_t k = 0; k < cand.size(); ++k)
      if (k != best) (void)hipFree(cand[k]);
    if (getenv("CLOUDSC2_PLACE_VERBOSE")) {  // does the choice still probe the same once the others are gone?
      std::vector<double> one(1, 0.0);
      if (!generic) (void)probe_all(1, bytes, kProbeCustom, [&](size_t) { return cand[best]; }, one);
      double m = 0.0, w = 0.0;
      (void)cloudsc2_device_probe(cand[best], bytes, kProbeMixed, 3, &m);
      (void)cloudsc2_device_probe(cand[best], bytes, kProbeWrite, 3, &w);
      fprintf(stderr, "cloudsc2_device_malloc: the chosen candidate after freeing the others: caller's sweep %.4f mixed %.4f write %.4f ms\n", one[0], m, w);
    }
  }
  st.candidates = (int)cand.size();
  (cand.size() > 1 ? g_searches : g_plain_allocs).fetch_add(1);
  if (getenv("CLOUDSC2_PLACE_VERBOSE") && cand.size() == 1)
    fprintf(stderr, "cloudsc2_device_malloc: %zu bytes, 1 candidate (plain hipMalloc%s)\n", bytes,
            policy == kPlaceSearch ? "" : policy == kPlaceOnRequest ? "; host-array driver workspace: searched only with CLOUDSC2_PLACE=1" : "; staging");
  DevAlloc a;
  a.bytes = bytes;
  std::lock_guard<std::mutex> lock(g_alloc_mutex);
  g_allocs.emplace_back(cand[best], a);
  g_last_place = st;
  *out = cand[best];
  return 0;
}

int device_free_impl(void* p) {
  if (!p) return 0;
  DevAlloc a;
  {
    std::lock_guard<std::mutex> lock(g_alloc_mutex);
    auto it = std::find_if(g_allocs.begin(), g_allocs.end(), [&](const std::pair<void*, DevAlloc>& x) { return x.first == p; });
    if (it == g_allocs.end()) return fail(CLOUDSC2_EINVAL, "cloudsc2_device_free: not a pointer returned by cloudsc2_device_malloc");
    a = it->second;
    g_allocs.erase(it);
  }
  if (a.chunk) {  // composed: unmap, release, give the range back
    HIP_TRY(hipDeviceSynchronize());
    for (size_t k = 0; k < a.handles.size(); ++k) (void)hipMemUnmap((char*)p + k * a.chunk, a.chunk);
    for (auto x : a.handles) (void)hipMemRelease(x);
    (void)hipMemAddressFree(p, a.bytes);
    return 0;
  }
  HIP_TRY(hipFree(p));
  return 0;
}

}  // namespace cloudsc2

extern "C" {
int cloudsc2_device_malloc(void** ptr, size_t bytes) { return device_malloc_impl(ptr, bytes); }
int cloudsc2_device_free(void* ptr) { return device_free_impl(ptr); }
int cloudsc2_device_probe(void* ptr, size_t bytes, int kind, int rounds, double* ms) {
  if (!ptr || !ms || rounds < 1 || rounds > 64 || (kind != 0 && kind != 1)) return fail(CLOUDSC2_EINVAL, "cloudsc2_device_probe: bad argument");
  if (int rc = require_device()) return rc;
  const long long nblocks = kind == 0 ? (long long)(bytes / (size_t)kProbeBlockBytes) : (long long)(bytes / (size_t)((kMixIn + kMixOut) * kMixBlockElems * 8));
  if (nblocks < 1 || nblocks > 0x7fffffffLL) return fail(CLOUDSC2_EINVAL, "cloudsc2_device_probe: buffer too small or too large");
  hipEvent_t ea = nullptr, eb = nullptr;
  hipError_t e = hipEventCreate(&ea);
  if (e == hipSuccess) e = hipEventCreate(&eb);
  std::vector<float> t;
  for (int r = 0; r <= rounds && e == hipSuccess; ++r) {  // launch 0 is a warm-up
    (void)hipEventRecord(ea, nullptr);
    launch_probe(ptr, bytes, kind);
    (void)hipEventRecord(eb, nullptr);
    e = hipEventSynchronize(eb);
    float f = 0;
    if (e == hipSuccess) e = hipEventElapsedTime(&f, ea, eb);
    if (r > 0) t.push_back(f);
  }
  if (ea) (void)hipEventDestroy(ea);
  if (eb) (void)hipEventDestroy(eb);
  if (e != hipSuccess) { g_err = std::string("cloudsc2_device_probe: ") + hipGetErrorString(e); (void)hipGetLastError(); return (int)e; }
  std::sort(t.begin(), t.end());
  *ms = t[t.size() / 2];
  return 0;
}
void cloudsc2_device_malloc_counts(long long* searched, long long* plain) {
  if (searched) *searched = g_searches.load();
  if (plain) *plain = g_plain_allocs.load();
}
void cloudsc2_device_malloc_info(int* candidates, double* best_ms, double* median_ms, double* worst_ms) {
  std::lock_guard<std::mutex> lock(g_alloc_mutex);
  if (candidates) *candidates = g_last_place.candidates;
  if (best_ms) *best_ms = g_last_place.best_ms;
  if (median_ms) *median_ms = g_last_place.median_ms;
  if (worst_ms) *worst_ms = g_last_place.worst_ms;
}
}
