// The tagged-granule exchange of the persistent kernels ("The tagged-granule exchange"): workgroups hand values
// to each other as 8-byte {step tag, payload} granules, written and polled with relaxed agent-scope atomics (sc1: they
// bypass the L2s; no fence, the data is its own flag - cdna guide G16 / R2), and every wait is bounded.  Granule format,
// poll cadence, bound and the LDS-only barrier are stated here once; the kernels keep their layouts, tags and orders.
#pragma once
#include "common.h"

typedef unsigned long long u64;

// Workgroup barrier that orders LDS only.  __syncthreads() also drains the vector-memory queue (s_waitcnt vmcnt(0)):
// inside the step loops that would wait, at every barrier, for whatever is in flight - the history prefetch from HBM,
// the write-through acknowledgement of a publish (1.3 us).  The waves of a workgroup talk through LDS only; what goes
// through global memory is either tag-polled (the exchanges) or read by later kernels.
__device__ __forceinline__ void ns_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// ---------------------------------------------------------------- cluster placement
// Which (cluster, member) the workgroup of grid index b is, in a launch of `clusters` independent clusters of `members`
// workgroups that exchange with each other.  The hardware deals consecutive grid indices to the 8 XCDs in turn (gemm.hip,
// xcd_work_item), so the linear map b / members, b % members spreads the members of a cluster over as many XCDs as
// there are; a hand-off inside one XCD is the shorter one (profiles/r05_ring_bench.txt, profiles/cluster_xcd.txt).  The
// placed map gives all members of a cluster one residue b % 8: XCD x holds clusters x, x + 8, .. in slots of `members`
// indices each.  clusters % 8 != 0 pads the grid: an index whose cluster does not exist is inactive and its workgroup
// returns before its first barrier, poll, LDS write or global write.  Index 0 is cluster 0, member 0 in both maps.
// Only which CU runs which role moves: work areas, exchange buffers and history are indexed by the logical ids.
constexpr int NS_XCDS = 8;
struct ns_cluster_slot { int cluster, member; bool active; };
__host__ __device__ __forceinline__ int ns_cluster_grid(int clusters, int members, bool placed = true) {
  return placed ? NS_XCDS * members * ((clusters + NS_XCDS - 1) / NS_XCDS) : clusters * members;
}
__host__ __device__ __forceinline__ ns_cluster_slot ns_cluster_place(int b, int clusters, int members, bool placed = true) {
  // (unsigned: a signed b / 8 costs the kernels sign fix-ups and, in one backward form, its register allocation)
  const unsigned ub = (unsigned)b, um = (unsigned)members;
  const int cluster = (int)(placed ? (ub & 7u) + 8u * ((ub >> 3) / um) : ub / um);
  const int member = (int)(placed ? (ub >> 3) % um : ub % um);
  return {cluster, member, cluster < clusters};
}
// Measured and not taken (profiles/cluster_xcd.txt): the fp32-state BiLSTM forward, whose H / 32 members all poll the whole
// chain's granules, is slower on one XCD ("bilstmf32" below stays linear by default), and so are lstm_wide's chip-wide
// row groups kept to 8 / (row groups) XCDs each.
// core.hip: whether the launches of `family` place their clusters - "bilstm" (lstm_cluster2_fwd, lstm_cluster2p_bwd and
// the single-role kernels), "bilstmf32" (lstm_cluster3_fwd), "attn", "gru", "taco1attn".  NS_CLUSTER_XCD, read per call:
// unset = the family's default, 0 = linear everywhere, 1 = placed everywhere, a comma list of family names = those stay
// linear and the others are placed.
bool ns_cluster_placed(const char* family);

// ---------------------------------------------------------------- the granule
// High word: the tag (the step that consumes it, so a buffer is never reset between steps); low word: 32 payload bits -
// one fp32, or two bf16 that the kernel packs itself.
__device__ __forceinline__ u64 ns_granule(unsigned tag, unsigned payload) { return ((u64)tag << 32) | (u64)payload; }
__device__ __forceinline__ u64 ns_granule(unsigned tag, float v) { return ns_granule(tag, __float_as_uint(v)); }
__device__ __forceinline__ unsigned ns_granule_tag(u64 g) { return (unsigned)(g >> 32); }
__device__ __forceinline__ unsigned ns_granule_payload(u64 g) { return (unsigned)g; }
__device__ __forceinline__ float ns_granule_value(u64 g) { return __uint_as_float((unsigned)g); }

// A pointer known to be global memory (pointers out of by-value argument structs are generic: flat_load / flat_store,
// which also count on lgkmcnt - a poll through them would hold up the LDS traffic of its wave).
#define NS_GLOBAL __attribute__((address_space(1)))
__device__ __forceinline__ void ns_put_granule(u64* p, u64 g) {
  __hip_atomic_store((NS_GLOBAL u64*)p, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void ns_put_granule(u64* p, unsigned tag, float v) { ns_put_granule(p, ns_granule(tag, v)); }
__device__ __forceinline__ u64 ns_ld_granule(const u64* p) {
  return __hip_atomic_load((const NS_GLOBAL u64*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------- bounded spins
// Every wait of a persistent kernel is bounded in WALL-CLOCK time, not in iterations: a workgroup that cannot be placed
// because a foreign kernel (a collective's channel kernel, a weight-gradient product on the second stream) holds its CU
// keeps its peers polling for as long as that kernel lives, and an iteration count says nothing about how long that is.
// The clock (s_memrealtime, 100 MHz) is read once per 1024 polls; 32 bits of it wrap after 42 s, far beyond the bound.
constexpr unsigned NS_SPIN_TICKS = 200000000u;      // 2 s
__device__ __forceinline__ bool ns_spin_timed_out(unsigned& t0, unsigned ticks = NS_SPIN_TICKS) {
  const unsigned now = (unsigned)wall_clock64() | 1u;
  if (t0 == 0u) { t0 = now; return false; }
  return now - t0 > ticks;
}

// The give-up rule of a spin, called after a pass that failed.  It counts the pass; every PERIOD passes it reads the
// status word - a peer has given up: so does the caller - and then the clock: past the bound it raises the status word
// to `code` first.  Between those passes it costs one add and one compare: no thread reads the status word from memory
// on a step's critical path.  The caller owns the object (the kernels that trace their polling read `spins`) and tells
// its own workgroup through LDS.
struct ns_spin {
  unsigned spins = 0, clk0 = 0;
  template <unsigned PERIOD = 1024>
  __device__ __forceinline__ bool give_up(int* status, int code, unsigned ticks = NS_SPIN_TICKS) {
    static_assert((PERIOD & (PERIOD - 1)) == 0, "cadence");
    bool gone = false;
    if ((++spins & (PERIOD - 1)) == 0) {
      if (__hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) gone = true;
      else if (ns_spin_timed_out(clk0, ticks)) { atomicExch(status, code); gone = true; }
    }
    return gone;
  }
};

// Polls N granules until every one carries `tag`.  A pass issues all N loads through ld(j) before any compare, so that
// it stays one memory round trip; ld does the load itself (ns_ld_granule) and returns ns_granule(tag, 0u) for an item
// that does not exist.  Returns false when it gave up (v is then whatever the last pass read).
template <unsigned PERIOD = 1024, int N, class Ld>
__device__ __forceinline__ bool ns_poll_granules(u64 (&v)[N], unsigned tag, ns_spin& sp, int* status, int code, Ld ld,
                                                 unsigned ticks = NS_SPIN_TICKS) {
  for (;;) {
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = ld(j);
    bool ok = true;
#pragma unroll
    for (int j = 0; j < N; ++j) ok = ok && ns_granule_tag(v[j]) == tag;
    if (ok) return true;
    if (sp.give_up<PERIOD>(status, code, ticks)) return false;
  }
}

// Every thread of a CT-thread workgroup waits for its own fp32 granules (PER per thread, stride CT) of src[0, total) and
// drops the values into dst (LDS).  Returns false when this thread gave up: the caller raises its workgroup's LDS abort
// word then.
template <int PER, int CT>
__device__ __forceinline__ bool ns_gather_granules(const u64* src, int total, unsigned tag, float* dst, int tid,
                                                   int* status, int code) {
  u64 v[PER];
  ns_spin sp;
  const bool good = ns_poll_granules(v, tag, sp, status, code, [&](int j) {
    const int i = tid + j * CT;
    return i < total ? ns_ld_granule(src + i) : ns_granule(tag, 0u);
  });
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int i = tid + j * CT;
    if (i < total) dst[i] = ns_granule_value(v[j]);
  }
  return good;
}

// The mapped form: at(i, src, dst) names the granule and the LDS word of item i = tid + j * CT.
template <int PER, int CT, class At>
__device__ __forceinline__ bool ns_gather_mapped(int total, unsigned tag, int tid, int* status, int code, At at) {
  const u64* src[PER];
  float* dst[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int i = tid + j * CT;
    src[j] = nullptr; dst[j] = nullptr;
    if (i < total) at(i, src[j], dst[j]);
  }
  u64 v[PER];
  ns_spin sp;
  const bool good = ns_poll_granules(v, tag, sp, status, code, [&](int j) {
    return src[j] ? ns_ld_granule(src[j]) : ns_granule(tag, 0u);
  });
#pragma unroll
  for (int j = 0; j < PER; ++j) if (dst[j]) *dst[j] = ns_granule_value(v[j]);
  return good;
}
