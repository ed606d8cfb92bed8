// Device-side pieces of the MemVLA memory path (dexbotic/model/memvla/memvla_arch.py:82-127, 195-411)
// that used to run as torch glue (rand / compare / cast / divide per dropout mask; cosine_similarity + .item() per merge):
//   dxa_dropout_mask       one launch draws a whole dropout mask (entries 0 | 1/(1-p)) from a counter-based generator
//   dxa_bank_consolidate   the token-merge consolidation of one memory bank ENTIRELY on the device: cosine similarity of
//                          every neighbouring pair of entries, arg-max, merge of that pair, compaction of entries and
//                          timesteps — no host read-back, the bank's length evolves deterministically (host bookkeeping)
//   dxa_bank_stage_fwd/bwd, dxa_bank_append, dxa_bank_consolidate_batched
//                          'parallel_stream' (memvla_arch.py:340-361): batch slot b is its own episode, so the B banks of a role lie
//                          side by side and staging what the retrieval reads, the append and the consolidation are one launch
//                          (two for the token merge) over all B slots, lengths read from a device array of counts
//   dxa_bank_stage_fwd_at, dxa_bank_append_at, dxa_bank_consolidate_batched_at
//                          the same kernels on a chosen subset of the S slots of a bank, in any order: row r of the call works on
//                          slot slot_ids[r] (served episodes tick at different rates, join and leave); the other slots are not touched
#include "common.h"

namespace {

constexpr int TPB = 256;

// Philox4x32-10 (Salmon et al., SC'11): counter (c0..c3) x key (k0, k1) -> 4 x 32 random bits
__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
  const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
  const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0, hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
  c[0] = hi1 ^ c[1] ^ k0; c[1] = lo1; c[2] = hi0 ^ c[3] ^ k1; c[3] = lo0;
}
__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c, k0, k1);
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}

// mask[i] = u_i >= p ? 1 / (1 - p) : 0 with u_i uniform in [0, 1): nn.Dropout / SDPA dropout_p semantics (keep probability
// 1 - p, survivors scaled); thread t draws elements 4 t .. 4 t + 3 from counter (t, offset)
template <typename T>
__global__ __launch_bounds__(TPB) void dropout_mask_k(T* __restrict__ out, int64_t n, float p, float keep_scale, uint32_t seed_lo,
                                                      uint32_t seed_hi, uint32_t off_lo, uint32_t off_hi) {
  const int64_t quads = (n + 3) / 4;
  for (int64_t t = (int64_t)blockIdx.x * TPB + threadIdx.x; t < quads; t += (int64_t)gridDim.x * TPB) {
    uint32_t c[4] = {(uint32_t)t, (uint32_t)(t >> 32), off_lo, off_hi};
    philox4x32_10(c, seed_lo, seed_hi);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int64_t i = 4 * t + e;
      if (i < n) {
        const float u = (float)(c[e] >> 8) * (1.0f / 16777216.0f);      // 24 random bits: exactly representable, < 1
        stf<T>(out + i, u >= p ? keep_scale : 0.f);
      }
    }
  }
}

// sims[i] = mean over the N tokens of cos(feat[i, n, :], feat[i + 1, n, :]), i < len - 1 (F.cosine_similarity, eps 1e-8 on each
// norm, memvla_arch.py:263-275).  One workgroup per pair; a wave owns tokens wave, wave + 4, ...; fixed fold order.
template <typename T>
__device__ __forceinline__ void bank_pair_sim(const T* __restrict__ a, const T* __restrict__ b, float* __restrict__ out, int64_t N,
                                              int64_t D) {
  __shared__ float red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float acc = 0.f;
  for (int64_t n = wave; n < N; n += 4) {
    float dot = 0.f, na = 0.f, nb = 0.f;
    for (int64_t d = lane; d < D; d += 64) {
      const float x = ldf<T>(a + n * D + d), y = ldf<T>(b + n * D + d);
      dot += x * y; na += x * x; nb += y * y;
    }
    dot = wave_sum(dot); na = wave_sum(na); nb = wave_sum(nb);
    acc += dot / (fmaxf(sqrtf(na), 1e-8f) * fmaxf(sqrtf(nb), 1e-8f));
  }
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) *out = ((red[0] + red[1]) + (red[2] + red[3])) / (float)N;
}
template <typename T>
__global__ __launch_bounds__(TPB) void bank_sims_k(const T* __restrict__ feat, float* __restrict__ sims, int64_t N, int64_t D) {
  const T* a = feat + (int64_t)blockIdx.x * N * D;
  bank_pair_sim<T>(a, a + N * D, sims + blockIdx.x, N, D);
}

// j = first arg-max of sims[0 .. len - 2] (numpy.argmax); entry j <- 0.5 (entry j + entry j + 1), entries j + 2 .. move down by
// one, same for the timesteps (memvla_arch.py:276-287).  Element e of every entry is handled by ONE thread walking the
// entries in ascending order (reads entry i + 1 before it writes entry i): in place, no barrier needed.
// fifo = 1: the oldest entry is dropped instead (memvla_arch.py:300-303): every entry moves down by one, sims is not read.
template <typename T>
__device__ __forceinline__ void bank_merge_slot(T* __restrict__ feat, float* __restrict__ ts, const float* __restrict__ sims, int len,
                                                int64_t E, int fifo) {
  int j = -1;
  if (!fifo) {
    j = 0;
    float best = sims[0];
    for (int i = 1; i < len - 1; ++i) {
      const float s = sims[i];
      if (s > best) { best = s; j = i; }
    }
  }
  for (int64_t e = (int64_t)blockIdx.x * TPB + threadIdx.x; e < E; e += (int64_t)gridDim.x * TPB) {
    // the merged value rounded through the storage type, as 0.5 * (f_j + f_j+1) is stored by the reference
    if (j >= 0)
      stf<T>(feat + (int64_t)j * E + e, 0.5f * ldf<T>(feat + (int64_t)j * E + e) + 0.5f * ldf<T>(feat + (int64_t)(j + 1) * E + e));
    for (int i = j + 1; i < len - 1; ++i) feat[(int64_t)i * E + e] = feat[(int64_t)(i + 1) * E + e];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (j >= 0) ts[j] = 0.5f * (ts[j] + ts[j + 1]);
    for (int i = j + 1; i < len - 1; ++i) ts[i] = ts[i + 1];
  }
}
template <typename T>
__global__ __launch_bounds__(TPB) void bank_merge_k(T* __restrict__ feat, float* __restrict__ ts, const float* __restrict__ sims,
                                                    int len, int64_t E, int fifo) {
  bank_merge_slot<T>(feat, ts, sims, len, E, fifo);
}

// ---- B banks side by side ('parallel_stream': batch slot b is its own running episode): feat [B, cap, N, D], ts [B, cap],
// counts [B] int32 on the device.  blockIdx.y = slot.  A count read from the device is clamped to [0, cap] before it indexes.
__device__ __forceinline__ int bank_count(const int32_t* __restrict__ counts, int b, int add, int cap) {
  const int n = counts[b] + add;
  return n < 0 ? 0 : (n > cap ? cap : n);
}
// the slot row r of a launch works on: r itself ('parallel_stream', slot_ids = null: all B slots in slot order) or slot_ids[r] of a
// bank of S slots (the _at entry points); an id read from the device that is outside [0, S) gives -1: the row touches no slot
__device__ __forceinline__ int bank_slot(const int32_t* __restrict__ slot_ids, int r, int S) {
  if (!slot_ids) return r;
  const int s = slot_ids[r];
  return (s < 0 || s >= S) ? -1 : s;
}

// what the retrieval of one step reads: mem [B, cap, E] = the slot's entries oldest first (no history: entry 0 = the slot's own
// tokens, the frame retrieving from itself), zeros behind them; ts_eff [B, cap] the matching timesteps; kv_len [B] keys in use
template <typename T>
__global__ __launch_bounds__(TPB) void bank_stage_k(const T* __restrict__ feat, const float* __restrict__ ts,
                                                    const int32_t* __restrict__ counts, const T* __restrict__ tokens,
                                                    const float* __restrict__ timesteps, T* __restrict__ mem,
                                                    float* __restrict__ ts_eff, int32_t* __restrict__ kv_len, int cap, int64_t N,
                                                    int64_t E, const int32_t* __restrict__ slot_ids, int S) {
  const int b = blockIdx.y, s = bank_slot(slot_ids, b, S);
  const int n = s < 0 ? 0 : bank_count(counts, b, 0, cap);         // a row without a slot is staged as a slot without history
  const int64_t total = (int64_t)cap * E, live = (int64_t)(n > 0 ? n : 1) * E;
  const T* src = n > 0 ? feat + (int64_t)s * total : tokens + (int64_t)b * E;
  T* dst = mem + (int64_t)b * total;
  for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < total; i += (int64_t)gridDim.x * TPB)
    dst[i] = i < live ? src[i] : (T)0.f;
  if (blockIdx.x == 0) {
    for (int i = threadIdx.x; i < cap; i += TPB)
      ts_eff[(int64_t)b * cap + i] = n > 0 ? (i < n ? ts[(int64_t)s * cap + i] : 0.f) : (i == 0 ? timesteps[b] : 0.f);
    if (threadIdx.x == 0) kv_len[b] = (int32_t)((n > 0 ? n : 1) * N);
  }
}

// dtokens[b] = dmem[b, 0] for a slot without history (its tokens were entry 0), 0 for the others (history is detached)
template <typename T>
__global__ __launch_bounds__(TPB) void bank_stage_bwd_k(const T* __restrict__ dmem, const int32_t* __restrict__ counts,
                                                        T* __restrict__ dtokens, int cap, int64_t E) {
  const int b = blockIdx.y;
  const bool own = bank_count(counts, b, 0, cap) == 0;
  const T* src = dmem + (int64_t)b * cap * E;
  T* dst = dtokens + (int64_t)b * E;
  for (int64_t e = (int64_t)blockIdx.x * TPB + threadIdx.x; e < E; e += (int64_t)gridDim.x * TPB) dst[e] = own ? src[e] : (T)0.f;
}

// feat[b, counts[b]] = src[b], ts[b, counts[b]] = timesteps[b]; a slot whose count says it is full (>= cap) is left alone
template <typename T>
__global__ __launch_bounds__(TPB) void bank_append_k(T* __restrict__ feat, float* __restrict__ ts, const int32_t* __restrict__ counts,
                                                     const T* __restrict__ src, const float* __restrict__ timesteps, int cap,
                                                     int64_t E, const int32_t* __restrict__ slot_ids, int S) {
  const int b = blockIdx.y, slot = bank_slot(slot_ids, b, S);
  const int n = bank_count(counts, b, 0, cap);
  if (slot < 0 || n >= cap) return;
  T* dst = feat + ((int64_t)slot * cap + n) * E;
  const T* s = src + (int64_t)b * E;
  for (int64_t e = (int64_t)blockIdx.x * TPB + threadIdx.x; e < E; e += (int64_t)gridDim.x * TPB) dst[e] = s[e];
  if (blockIdx.x == 0 && threadIdx.x == 0) ts[(int64_t)slot * cap + n] = timesteps[b];
}

// bank_sims_k / bank_merge_k over (pair, slot) / (elements, slot) for the slots whose length counts[b] + add exceeds mem_length
// (counts and the sims scratch are indexed by the launch's row b, the bank by the row's slot);
// the other slots' blocks return at once (the test is uniform over a block, so the barrier inside bank_pair_sim is safe)
template <typename T>
__global__ __launch_bounds__(TPB) void bank_sims_batched_k(const T* __restrict__ feat, const int32_t* __restrict__ counts, int add,
                                                           int mem_length, float* __restrict__ sims, int cap, int64_t N, int64_t D,
                                                           const int32_t* __restrict__ slot_ids, int S) {
  const int b = blockIdx.y, i = blockIdx.x, slot = bank_slot(slot_ids, b, S);
  const int len = bank_count(counts, b, add, cap);
  if (slot < 0 || len <= mem_length || i >= len - 1) return;
  const T* a = feat + ((int64_t)slot * cap + i) * N * D;
  bank_pair_sim<T>(a, a + N * D, sims + (int64_t)b * (cap - 1) + i, N, D);
}
template <typename T>
__global__ __launch_bounds__(TPB) void bank_merge_batched_k(T* __restrict__ feat, float* __restrict__ ts,
                                                            const int32_t* __restrict__ counts, int add, int mem_length,
                                                            const float* __restrict__ sims, int cap, int64_t E, int fifo,
                                                            const int32_t* __restrict__ slot_ids, int S) {
  const int b = blockIdx.y, slot = bank_slot(slot_ids, b, S);
  const int len = bank_count(counts, b, add, cap);
  if (slot < 0 || len <= mem_length || len < 2) return;
  bank_merge_slot<T>(feat + (int64_t)slot * cap * E, ts + (int64_t)slot * cap, sims + (int64_t)b * (cap - 1), len, E, fifo);
}

// out[r, n, c] = (x ? x[r, n, c] : 0) + alpha * g[r, c]: the timestep positional embedding added to every token of a bank entry
// (memvla_arch.py:352-360), and the broadcast of a per-entry row over the tokens (x = null: backward of the token mean)
template <typename T>
__global__ __launch_bounds__(TPB) void add_rows_k(const T* __restrict__ x, const T* __restrict__ g, T* __restrict__ o, int64_t R,
                                                  int64_t Nn, int64_t C, float alpha) {
  const int64_t total = R * Nn * C;
  for (int64_t it = (int64_t)blockIdx.x * TPB + threadIdx.x; it < total; it += (int64_t)gridDim.x * TPB) {
    const int64_t c = it % C, r = it / (Nn * C);
    stf<T>(o + it, (x ? ldf<T>(x + it) : 0.f) + alpha * ldf<T>(g + r * C + c));
  }
}
// out[r, c] = scale * sum_n x[r, n, c] (fp32 accumulation in token order: deterministic); grid (column tiles, R)
template <typename T>
__global__ __launch_bounds__(TPB) void token_sum_k(const T* __restrict__ x, T* __restrict__ o, int64_t Nn, int64_t C, float scale) {
  const int64_t c = (int64_t)blockIdx.x * TPB + threadIdx.x, r = blockIdx.y;
  if (c >= C) return;
  const T* p = x + r * Nn * C + c;
  float s = 0.f;
  for (int64_t n = 0; n < Nn; ++n) s += ldf<T>(p + n * C);
  stf<T>(o + r * C + c, s * scale);
}

}  // namespace

extern "C" int dxa_add_rows(const void* x, const void* g, void* out, int64_t R, int64_t Nn, int64_t C, float alpha, int dtype,
                            dxa_stream_t stream) {
  DXA_CHECK_ARG(g && out && R >= 0 && Nn >= 0 && C > 0 && (dtype == DXA_F32 || dtype == DXA_BF16), "dxa_add_rows: bad args");
  if (R * Nn == 0) return DXA_OK;
  const dim3 grid(dxa_grid1d(R * Nn * C, TPB));
  if (dtype == DXA_BF16)
    hipLaunchKernelGGL((add_rows_k<bf16_t>), grid, dim3(TPB), 0, (hipStream_t)stream, (const bf16_t*)x, (const bf16_t*)g, (bf16_t*)out, R, Nn, C, alpha);
  else
    hipLaunchKernelGGL((add_rows_k<float>), grid, dim3(TPB), 0, (hipStream_t)stream, (const float*)x, (const float*)g, (float*)out, R, Nn, C, alpha);
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}

extern "C" int dxa_token_sum(const void* x, void* out, int64_t R, int64_t Nn, int64_t C, float scale, int dtype, dxa_stream_t stream) {
  DXA_CHECK_ARG(x && out && R >= 0 && Nn >= 0 && C > 0 && R <= 65535 && (dtype == DXA_F32 || dtype == DXA_BF16), "dxa_token_sum: bad args");
  if (R == 0) return DXA_OK;
  const dim3 grid((unsigned)((C + TPB - 1) / TPB), (unsigned)R);
  if (dtype == DXA_BF16)
    hipLaunchKernelGGL((token_sum_k<bf16_t>), grid, dim3(TPB), 0, (hipStream_t)stream, (const bf16_t*)x, (bf16_t*)out, Nn, C, scale);
  else
    hipLaunchKernelGGL((token_sum_k<float>), grid, dim3(TPB), 0, (hipStream_t)stream, (const float*)x, (float*)out, Nn, C, scale);
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}

extern "C" int dxa_dropout_mask(void* out, int64_t n, float p, uint64_t seed, uint64_t offset, int dtype, dxa_stream_t stream) {
  DXA_CHECK_ARG(out && n >= 0 && p >= 0.f && p < 1.f && (dtype == DXA_F32 || dtype == DXA_BF16), "dxa_dropout_mask: bad args");
  if (n == 0) return DXA_OK;
  const float ks = 1.f / (1.f - p);
  const dim3 g(dxa_grid1d((n + 3) / 4, TPB));
  hipStream_t st = (hipStream_t)stream;
  if (dtype == DXA_BF16)
    hipLaunchKernelGGL((dropout_mask_k<bf16_t>), g, dim3(TPB), 0, st, (bf16_t*)out, n, p, ks, (uint32_t)seed, (uint32_t)(seed >> 32),
                       (uint32_t)offset, (uint32_t)(offset >> 32));
  else
    hipLaunchKernelGGL((dropout_mask_k<float>), g, dim3(TPB), 0, st, (float*)out, n, p, ks, (uint32_t)seed, (uint32_t)(seed >> 32),
                       (uint32_t)offset, (uint32_t)(offset >> 32));
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}

extern "C" int dxa_bank_consolidate(void* feat, float* ts, int len, int64_t N, int64_t D, int dtype, int fifo, float* sims,
                                    dxa_stream_t stream) {
  DXA_CHECK_ARG(feat && ts && (sims || fifo) && len >= 2 && N > 0 && D > 0 && (dtype == DXA_F32 || dtype == DXA_BF16),
                "dxa_bank_consolidate: bad args");
  hipStream_t st = (hipStream_t)stream;
  const int64_t E = N * D;
  if (dtype == DXA_BF16) {
    if (!fifo) hipLaunchKernelGGL((bank_sims_k<bf16_t>), dim3(len - 1), dim3(TPB), 0, st, (const bf16_t*)feat, sims, N, D);
    hipLaunchKernelGGL((bank_merge_k<bf16_t>), dim3(dxa_grid1d(E, TPB, 256)), dim3(TPB), 0, st, (bf16_t*)feat, ts, sims, len, E, fifo);
  } else {
    if (!fifo) hipLaunchKernelGGL((bank_sims_k<float>), dim3(len - 1), dim3(TPB), 0, st, (const float*)feat, sims, N, D);
    hipLaunchKernelGGL((bank_merge_k<float>), dim3(dxa_grid1d(E, TPB, 256)), dim3(TPB), 0, st, (float*)feat, ts, sims, len, E, fifo);
  }
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}

// ---- 'parallel_stream': B banks per launch -----------------------------------------------------------------------------------
#define DXA_BANK_CHECK(name, ptrs)                                                                                       \
  do {                                                                                                                   \
    DXA_CHECK_ARG(ptrs, name ": null pointer");                                                                          \
    DXA_CHECK_ARG(B > 0 && N > 0 && D > 0 && cap > 0, name ": B, N, D and cap must be positive");                        \
    DXA_CHECK_ARG(cap >= 2, name ": cap must be at least 2 (mem_length + 1)");                                           \
    DXA_CHECK_ARG(B <= 65535 && cap <= 65536, name ": at most 65535 slots of 65536 entries");                            \
    DXA_CHECK_ARG(dtype == DXA_F32 || dtype == DXA_BF16, name ": dtype must be fp32 or bf16");                           \
  } while (0)

static int bank_stage_launch(const void* feat, const float* ts, const int32_t* slot_ids, const int32_t* counts,
                             const void* tokens, const float* timesteps, void* mem, float* ts_eff, int32_t* kv_len, int64_t B,
                             int64_t S, int64_t cap, int64_t N, int64_t D, int dtype, dxa_stream_t stream) {
  const int64_t E = N * D;
  const dim3 grid(dxa_grid1d(cap * E, TPB, 1024), (unsigned)B);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == DXA_BF16)
    hipLaunchKernelGGL((bank_stage_k<bf16_t>), grid, dim3(TPB), 0, st, (const bf16_t*)feat, ts, counts, (const bf16_t*)tokens,
                       timesteps, (bf16_t*)mem, ts_eff, kv_len, (int)cap, N, E, slot_ids, (int)S);
  else
    hipLaunchKernelGGL((bank_stage_k<float>), grid, dim3(TPB), 0, st, (const float*)feat, ts, counts, (const float*)tokens,
                       timesteps, (float*)mem, ts_eff, kv_len, (int)cap, N, E, slot_ids, (int)S);
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}

extern "C" int dxa_bank_stage_fwd(const void* feat, const float* ts, const int32_t* counts, const void* tokens,
                                  const float* timesteps, void* mem, float* ts_eff, int32_t* kv_len, int64_t B, int64_t cap,
                                  int64_t N, int64_t D, int dtype, dxa_stream_t stream) {
  DXA_BANK_CHECK("dxa_bank_stage_fwd", feat && ts && counts && tokens && timesteps && mem && ts_eff && kv_len);
  DXA_CHECK_ARG(cap * N <= INT32_MAX, "dxa_bank_stage_fwd: cap * N keys do not fit kv_len");
  return bank_stage_launch(feat, ts, nullptr, counts, tokens, timesteps, mem, ts_eff, kv_len, B, B, cap, N, D,
                           dtype, stream);
}

extern "C" int dxa_bank_stage_bwd(const void* dmem, const int32_t* counts, void* dtokens, int64_t B, int64_t cap, int64_t N,
                                  int64_t D, int dtype, dxa_stream_t stream) {
  DXA_BANK_CHECK("dxa_bank_stage_bwd", dmem && counts && dtokens);
  const int64_t E = N * D;
  const dim3 grid(dxa_grid1d(E, TPB, 256), (unsigned)B);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == DXA_BF16)
    hipLaunchKernelGGL((bank_stage_bwd_k<bf16_t>), grid, dim3(TPB), 0, st, (const bf16_t*)dmem, counts, (bf16_t*)dtokens, (int)cap, E);
  else
    hipLaunchKernelGGL((bank_stage_bwd_k<float>), grid, dim3(TPB), 0, st, (const float*)dmem, counts, (float*)dtokens, (int)cap, E);
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}

static int bank_append_launch(void* feat, float* ts, const int32_t* slot_ids, const int32_t* counts, const void* src,
                              const float* timesteps, int64_t B, int64_t S, int64_t cap, int64_t N, int64_t D, int dtype,
                              dxa_stream_t stream) {
  const int64_t E = N * D;
  const dim3 grid(dxa_grid1d(E, TPB, 256), (unsigned)B);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == DXA_BF16)
    hipLaunchKernelGGL((bank_append_k<bf16_t>), grid, dim3(TPB), 0, st, (bf16_t*)feat, ts, counts, (const bf16_t*)src, timesteps,
                       (int)cap, E, slot_ids, (int)S);
  else
    hipLaunchKernelGGL((bank_append_k<float>), grid, dim3(TPB), 0, st, (float*)feat, ts, counts, (const float*)src, timesteps,
                       (int)cap, E, slot_ids, (int)S);
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}

extern "C" int dxa_bank_append(void* feat, float* ts, const int32_t* counts, const void* src, const float* timesteps, int64_t B,
                               int64_t cap, int64_t N, int64_t D, int dtype, dxa_stream_t stream) {
  DXA_BANK_CHECK("dxa_bank_append", feat && ts && counts && src && timesteps);
  return bank_append_launch(feat, ts, nullptr, counts, src, timesteps, B, B, cap, N, D, dtype, stream);
}

static int bank_consolidate_launch(void* feat, float* ts, const int32_t* slot_ids, const int32_t* counts, int count_add,
                                   int mem_length, int fifo, float* sims, int64_t B, int64_t S, int64_t cap, int64_t N, int64_t D,
                                   int dtype, dxa_stream_t stream) {
  const int64_t E = N * D;
  const dim3 gs((unsigned)(cap - 1), (unsigned)B), gm(dxa_grid1d(E, TPB, 256), (unsigned)B);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == DXA_BF16) {
    if (!fifo)
      hipLaunchKernelGGL((bank_sims_batched_k<bf16_t>), gs, dim3(TPB), 0, st, (const bf16_t*)feat, counts, count_add, mem_length, sims,
                         (int)cap, N, D, slot_ids, (int)S);
    hipLaunchKernelGGL((bank_merge_batched_k<bf16_t>), gm, dim3(TPB), 0, st, (bf16_t*)feat, ts, counts, count_add, mem_length, sims,
                       (int)cap, E, fifo, slot_ids, (int)S);
  } else {
    if (!fifo)
      hipLaunchKernelGGL((bank_sims_batched_k<float>), gs, dim3(TPB), 0, st, (const float*)feat, counts, count_add, mem_length, sims,
                         (int)cap, N, D, slot_ids, (int)S);
    hipLaunchKernelGGL((bank_merge_batched_k<float>), gm, dim3(TPB), 0, st, (float*)feat, ts, counts, count_add, mem_length, sims,
                       (int)cap, E, fifo, slot_ids, (int)S);
  }
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}

extern "C" int dxa_bank_consolidate_batched(void* feat, float* ts, const int32_t* counts, int count_add, int mem_length, int fifo,
                                            float* sims, int64_t B, int64_t cap, int64_t N, int64_t D, int dtype,
                                            dxa_stream_t stream) {
  DXA_BANK_CHECK("dxa_bank_consolidate_batched", feat && ts && counts && (sims || fifo));
  DXA_CHECK_ARG(mem_length >= 1 && mem_length < cap, "dxa_bank_consolidate_batched: mem_length must be in [1, cap)");
  DXA_CHECK_ARG(count_add >= 0 && count_add <= cap, "dxa_bank_consolidate_batched: count_add must be in [0, cap]");
  return bank_consolidate_launch(feat, ts, nullptr, counts, count_add, mem_length, fifo, sims, B, B, cap, N, D, dtype, stream);
}

// ---- the same three on rows slot_ids[0 .. R) of a bank of S slots (served episodes) --------------------------------------------
// B of the shared checks is the number of rows R; the slot count S is checked here
#define DXA_BANK_AT_CHECK(name)                                                                                          \
  do {                                                                                                                   \
    const int64_t B = R;                                                                                                 \
    DXA_BANK_CHECK(name, true);                                                                                          \
    DXA_CHECK_ARG(S > 0 && S <= INT32_MAX && R <= S, name ": R rows need 0 < R <= S slots");                             \
  } while (0)

extern "C" int dxa_bank_stage_fwd_at(const void* feat, const float* ts, const int32_t* slot_ids, const int32_t* counts,
                                     const void* tokens, const float* timesteps, void* mem, float* ts_eff, int32_t* kv_len,
                                     int64_t R, int64_t S, int64_t cap, int64_t N, int64_t D, int dtype, dxa_stream_t stream) {
  DXA_CHECK_ARG(feat && ts && slot_ids && counts && tokens && timesteps && mem && ts_eff && kv_len,
                "dxa_bank_stage_fwd_at: null pointer");
  DXA_BANK_AT_CHECK("dxa_bank_stage_fwd_at");
  DXA_CHECK_ARG(cap * N <= INT32_MAX, "dxa_bank_stage_fwd_at: cap * N keys do not fit kv_len");
  return bank_stage_launch(feat, ts, slot_ids, counts, tokens, timesteps, mem, ts_eff, kv_len, R, S, cap, N,
                           D, dtype, stream);
}

extern "C" int dxa_bank_append_at(void* feat, float* ts, const int32_t* slot_ids, const int32_t* counts, const void* src,
                                  const float* timesteps, int64_t R, int64_t S, int64_t cap, int64_t N, int64_t D, int dtype,
                                  dxa_stream_t stream) {
  DXA_CHECK_ARG(feat && ts && slot_ids && counts && src && timesteps, "dxa_bank_append_at: null pointer");
  DXA_BANK_AT_CHECK("dxa_bank_append_at");
  return bank_append_launch(feat, ts, slot_ids, counts, src, timesteps, R, S, cap, N, D, dtype, stream);
}

extern "C" int dxa_bank_consolidate_batched_at(void* feat, float* ts, const int32_t* slot_ids, const int32_t* counts, int count_add,
                                               int mem_length, int fifo, float* sims, int64_t R, int64_t S, int64_t cap, int64_t N,
                                               int64_t D, int dtype, dxa_stream_t stream) {
  DXA_CHECK_ARG(feat && ts && slot_ids && counts && (sims || fifo), "dxa_bank_consolidate_batched_at: null pointer");
  DXA_BANK_AT_CHECK("dxa_bank_consolidate_batched_at");
  DXA_CHECK_ARG(mem_length >= 1 && mem_length < cap, "dxa_bank_consolidate_batched_at: mem_length must be in [1, cap)");
  DXA_CHECK_ARG(count_add >= 0 && count_add <= cap, "dxa_bank_consolidate_batched_at: count_add must be in [0, cap]");
  return bank_consolidate_launch(feat, ts, slot_ids, counts, count_add, mem_length, fifo, sims, R, S, cap, N, D, dtype, stream);
}
