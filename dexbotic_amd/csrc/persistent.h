// Persistent kernels (dit_fused.hip, decode_fused.hip): one grid of co-resident workgroups walks phases separated by a device-wide
// barrier.  The protocol, as the code below implements it:
//  - Activations that cross workgroups are agent-scope (sc1) buffer accesses: stores write through to memory, loads miss in the
//    XCD-private L2s, whose contents are not coherent with each other.  The barrier therefore issues no fence and no cache
//    write-back or invalidate, and the weights stay cached.
//  - grid_sync: every wave waits until its own stores are acknowledged (s_waitcnt vmcnt(0)), the workgroup meets at __syncthreads,
//    and thread 0 adds 1 to arrival counter blockIdx.x % NCTR (relaxed, agent scope).  Lanes 0 .. NCTR-1 of wave 0 poll one counter
//    each with relaxed agent-scope loads and s_sleep in between, until every counter shows `epoch` arrivals of its workgroups.
//  - The spin is bounded (SPIN_LIMIT polls).  The launch is a plain one sized by the occupancy query (a cooperative launch adds
//    15-19 us per forward and enforces nothing more, MI355X_MICROARCH.md "coop-launch"), so co-residency holds only while nothing
//    else occupies CUs for long.  A workgroup that gives up raises the sticky abort word; every later barrier of every workgroup
//    falls through (the word is read every 16th poll), the launch drains in microseconds with a garbage result, and sync_status()
//    reports it to the host, which re-runs the request on the unfused path.
//  - grid_exit: the last workgroup out re-zeroes the counters, so each launch on a stream finds its sync block zeroed.
#pragma once
#include "common.h"

// Buffer-instruction cache policy: agent scope (gfx94x / gfx95x)
constexpr int SC1 = 16;

// Round 4: SIXTEEN arrival counters, 4 KiB apart.  The single counter + flag of rounds 1-3 cost 1.0 us + 10 ns per WORKGROUP (2.97 us
// at 192, 1.06 us at 8: `profiles/r04_barrier_vs_grid.txt`) — device-scope atomics on one address are applied one after the other at
// the memory side, and the flag hop is a second dependent round trip behind them; spread over 16 lines in 16 places the same arrivals
// take 1.27 us and nobody waits for a publisher (`scripts/probes/sync_probe.hip` modes 4 / 16: `profiles/r04_barrier_split.txt`).
constexpr unsigned NCTR = 16;
constexpr unsigned SPIN_LIMIT = 1u << 21;      // ~2 s

// Sync block layout in 32-bit words: the first KiB holds the exit counter, the abort word and the DiT kernels' two per-tile counter
// arrays (H / 16 <= 64 entries each); the NCTR arrival counters follow, one per 4 KiB.  68 KiB per (device, stream) and user.
constexpr unsigned SYNC_EXIT = 48;
constexpr unsigned SYNC_ABORT = 56;
constexpr unsigned SYNC_TILES_PROJ = 64;
constexpr unsigned SYNC_TILES_FC2 = 128;
constexpr int SYNC_NTILE = 64;
constexpr unsigned SYNC_CTR_WORDS = 1024;
constexpr size_t SYNC_BYTES = 4 * SYNC_CTR_WORDS * (NCTR + 1);
__host__ __device__ constexpr unsigned sync_ctr(unsigned g) { return SYNC_CTR_WORDS * (g + 1u); }   // arrival counter g

struct NoHook {
  __device__ void operator()() const {}
};

// `arrived` runs once the workgroup has met (the DiT stamp build times the store acknowledgement there).
template <typename Hook = NoHook>
__device__ __forceinline__ void grid_sync(unsigned* bar, unsigned nblk, unsigned& epoch, Hook arrived = {}) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // this wave's write-through stores have been acknowledged
  __syncthreads();
  arrived();
  epoch += 1;                                                // every thread keeps the count (wave 0's lanes need it)
  if (threadIdx.x < 64) {
    unsigned* abortw = bar + SYNC_ABORT;
    if (threadIdx.x == 0)
      (void)__hip_atomic_fetch_add(bar + sync_ctr(blockIdx.x % NCTR), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned g = threadIdx.x % NCTR;
    const unsigned target = epoch * ((nblk + NCTR - 1u - g) / NCTR);      // workgroups b < nblk with b % NCTR == g, `epoch` times
    const unsigned* mine = bar + sync_ctr(g);
    unsigned spins = 0;
    while (true) {
      const unsigned v = threadIdx.x < NCTR ? __hip_atomic_load(mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : target;
      if (__builtin_amdgcn_ballot_w64(v < target) == 0ull) break;
      __builtin_amdgcn_s_sleep(1);
      if ((++spins & 15u) == 0u) {            // the abort word: every 16th poll (a launch that was aborted drains in milliseconds)
        if (spins >= SPIN_LIMIT && threadIdx.x == 0) __hip_atomic_store(abortw, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (__hip_atomic_load(abortw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) || spins >= SPIN_LIMIT) break;
      }
    }
  }
  __syncthreads();
}

// Leave the counters zeroed for the next launch on this stream: every workgroup has passed the last barrier when it gets here, so
// the LAST one out may clear them, `clear_more` (counters of the caller's own) first.  Agent-scope atomic stores, not a host-side
// memset: under HIP-graph replay a memset node's zeros were not reliably what the next kernel's atomics saw (the sampler hung);
// atomics are performed at the memory side and always are.
template <typename Hook = NoHook>
__device__ __forceinline__ void grid_exit(unsigned* bar, unsigned nblk, Hook clear_more = {}) {
  if (threadIdx.x == 0) {
    unsigned* exit_cnt = bar + SYNC_EXIT;
    const unsigned out = __hip_atomic_fetch_add(exit_cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u;
    if (out == nblk) {
      clear_more();
      for (unsigned g = 0; g < NCTR; ++g) __hip_atomic_store(bar + sync_ctr(g), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(exit_cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// ---- host side

// The sync block of this stream in `blocks` (one StreamBlock of SYNC_BYTES per kernel family); `who` names the entry point.
inline int sync_block(StreamBlock& blocks, hipStream_t st, unsigned** out, const char* who) {
  if (int rc = blocks.get(st, out)) return rc;
  DXA_CHECK_ARG(*out != nullptr, "%s: first use on a stream allocates its sync block and cannot happen under stream capture: "
                "run the request once eagerly on this stream first", who);
  return DXA_OK;
}

// 1 in *timed_out if a launch on this stream gave up at a device-wide barrier since the last call (its result is garbage); the sync
// block is re-armed.  Synchronises the stream: call it where the host waits for the result anyway.
inline int sync_status(StreamBlock& blocks, dxa_stream_t stream, int* timed_out, const char* who) {
  DXA_CHECK_ARG(timed_out != nullptr, "%s: null output", who);
  hipStream_t st = (hipStream_t)stream;
  unsigned* blk = nullptr;
  if (int rc = sync_block(blocks, st, &blk, who)) return rc;
  unsigned word = 0;
  DXA_CHECK_HIP(hipMemcpyAsync(&word, blk + SYNC_ABORT, sizeof(word), hipMemcpyDeviceToHost, st));
  DXA_CHECK_HIP(hipStreamSynchronize(st));
  *timed_out = word != 0;
  if (word != 0) {
    DXA_CHECK_HIP(hipMemsetAsync(blk, 0, SYNC_BYTES, st));
    DXA_CHECK_HIP(hipStreamSynchronize(st));
  }
  return DXA_OK;
}

// How many 512-thread workgroups of `kernel` (with `lds` bytes of dynamic LDS) fit on one CU of the current device, and how many
// CUs it has: every workgroup of a persistent launch must be resident at once.  Cached per (device, kernel).
struct Residency {
  int per_cu, cus;
};
inline int residency(const void* kernel, size_t lds, Residency* out) {
  static std::mutex mu;
  static std::map<std::pair<int, const void*>, Residency> tab;
  int dev = 0;
  DXA_CHECK_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(mu);
  auto it = tab.find({dev, kernel});
  if (it == tab.end()) {
    Residency r;
    DXA_CHECK_HIP(hipDeviceGetAttribute(&r.cus, hipDeviceAttributeMultiprocessorCount, dev));
    DXA_CHECK_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&r.per_cu, kernel, 512, lds));
    it = tab.emplace(std::make_pair(dev, kernel), r).first;
  }
  *out = it->second;
  return DXA_OK;
}
