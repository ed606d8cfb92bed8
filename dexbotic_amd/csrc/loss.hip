// LM-head loss and greedy decode primitives for gfx950 (see include/dexbotic_amd.h).
//   dxa_cross_entropy_fwd/bwd : HF ForCausalLMLoss (transformers/loss/loss_utils.py) as called from
//                               dexbotic/model/dexbotic_arch.py:488 — logits upcast to fp32, mean over the
//                               non-ignored (already shifted) labels.
//   dxa_argmax_rows           : torch.argmax over the vocabulary (first index among equal maxima, a NaN the maximum), the greedy
//                               choice of GenerationMixin.generate(do_sample=False) (discrete_vla_arch.py:33-41).
//   dxa_cross_entropy_rows_bwd, dxa_ce_sample_reduce, dxa_expectile_loss : MuVLA's per-sample normalised, reward-weighted loss and its
//                               reward head's expectile regression (dexbotic/model/muvla/muvla_arch.py:559-592).
//   dxa_sample_rows           : the sampled choice of generate(do_sample=True): temperature, top-k, top-p, softmax and the draw in
//                               one launch (its own section at the end of this file).
// The cross-entropy and argmax kernels are one 256-thread workgroup per row streaming the row once (HBM-bound: 152 k logits = 304 KB bf16):
// online (max, sum-exp) pairs per thread folded across the block — no second pass for the maximum.
#include "common.h"

namespace {

template <typename T, int VEC>
__global__ __launch_bounds__(256) void argmax_rows_k(const T* __restrict__ xin, int64_t ld, int64_t* __restrict__ out,
                                                     int64_t cols) {
  __shared__ float red_v[4];
  __shared__ int64_t red_i[4];
  __shared__ int red_n[4];
  const T* x = xin + (int64_t)blockIdx.x * ld;
  float best = -INFINITY;
  int64_t idx = INT64_MAX;
  bool saw_nan = false;
  for (int64_t i = (int64_t)threadIdx.x * VEC; i < cols; i += 256 * VEC) {
    float v[VEC];
    Vec<T, VEC>::ld(v, x + i);
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      saw_nan |= (v[e] != v[e]);
      if (v[e] > best) { best = v[e]; idx = i + e; }    // a thread meets its columns in ascending order: an equal later one never wins
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float v2 = __shfl_xor(best, o, 64);
    const int64_t i2 = __shfl_xor(idx, o, 64);
    if (v2 > best || (v2 == best && i2 < idx)) { best = v2; idx = i2; }
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const bool wave_nan = __ballot(saw_nan) != 0;
  if (lane == 0) { red_v[w] = best; red_i[w] = idx; red_n[w] = wave_nan; }
  __syncthreads();
  if (red_n[0] | red_n[1] | red_n[2] | red_n[3]) {      // rare, uniform over the workgroup: NaN is the maximum, the FIRST one wins (torch)
    int64_t first = INT64_MAX;
    for (int64_t i = (int64_t)threadIdx.x * VEC; i < cols; i += 256 * VEC) {
      float v[VEC];
      Vec<T, VEC>::ld(v, x + i);
#pragma unroll
      for (int e = 0; e < VEC; ++e)
        if (v[e] != v[e] && i + e < first) first = i + e;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const int64_t i2 = __shfl_xor(first, o, 64);
      if (i2 < first) first = i2;
    }
    if (lane == 0) red_i[w] = first;                    // (no wave reads red_i on this path before the barrier below)
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int i = 1; i < 4; ++i)
        if (red_i[i] < first) first = red_i[i];
      out[blockIdx.x] = first;
    }
    return;
  }
  if (threadIdx.x == 0) {
    for (int i = 1; i < 4; ++i)
      if (red_v[i] > best || (red_v[i] == best && red_i[i] < idx)) { best = red_v[i]; idx = red_i[i]; }
    out[blockIdx.x] = idx == INT64_MAX ? 0 : idx;       // all -inf row: index 0 like torch
  }
}

// A handful of rows over a vocabulary (the greedy decode step: ONE row of 152,064 logits): argmax_rows_k walks the row with 256
// threads, 148 dependent iterations of 64-bit compares — 67 us of the 4.5 ms token (profiles/r05_decode_per_token_kernel_stats.txt).
// 1024 threads, 16-byte loads, two loads in flight, 32-bit indices (cols < 2^31), the same (value, then LOWEST index) order.
__global__ __launch_bounds__(1024) void argmax_rows_wide_k(const bf16_t* __restrict__ xin, int64_t ld, int64_t* __restrict__ out,
                                                           int cols) {
  __shared__ float red_v[16];
  __shared__ int red_i[16];
  __shared__ int red_n[16];
  const bf16_t* x = xin + (int64_t)blockIdx.x * ld;
  float best = -INFINITY;
  int idx = INT_MAX;
  bool saw_nan = false;
  auto take = [&](const float (&v)[8], int i) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      saw_nan |= (v[e] != v[e]);
      if (v[e] > best) { best = v[e]; idx = i + e; }    // a thread meets its columns in ascending order: an equal later one never wins
    }
  };
  int i = (int)threadIdx.x * 8;
  for (; i + 1024 * 8 < cols; i += 2 * 1024 * 8) {             // cols % 8 == 0: a thread's 8 columns are all inside or all outside
    float v0[8], v1[8];
    Vec<bf16_t, 8>::ld(v0, x + i);
    Vec<bf16_t, 8>::ld(v1, x + i + 1024 * 8);
    take(v0, i);
    take(v1, i + 1024 * 8);
  }
  if (i < cols) {
    float v0[8];
    Vec<bf16_t, 8>::ld(v0, x + i);
    take(v0, i);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float v2 = __shfl_xor(best, o, 64);
    const int i2 = __shfl_xor(idx, o, 64);
    if (v2 > best || (v2 == best && i2 < idx)) { best = v2; idx = i2; }
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const bool wave_nan = __ballot(saw_nan) != 0;
  if (lane == 0) { red_v[w] = best; red_i[w] = idx; red_n[w] = wave_nan; }
  __syncthreads();
  int any_nan = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) any_nan |= red_n[k];
  if (any_nan) {                                        // rare, uniform over the workgroup: NaN is the maximum, the FIRST one wins (torch)
    int first = INT_MAX;
    for (int j = (int)threadIdx.x * 8; j < cols; j += 1024 * 8) {
      float v[8];
      Vec<bf16_t, 8>::ld(v, x + j);
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (v[e] != v[e] && j + e < first) first = j + e;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o, 64));
    if (lane == 0) red_i[w] = first;                    // (no wave reads red_i on this path before the barrier below)
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int k = 1; k < 16; ++k) first = min(first, red_i[k]);
      out[blockIdx.x] = first;
    }
    return;
  }
  if (threadIdx.x == 0) {
    for (int k = 1; k < 16; ++k)
      if (red_v[k] > best || (red_v[k] == best && red_i[k] < idx)) { best = red_v[k]; idx = red_i[k]; }
    out[blockIdx.x] = idx == INT_MAX ? 0 : idx;         // all -inf row: index 0 like torch
  }
}

inline bool al(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int dxa_argmax_rows(const void* x, int64_t ld, int64_t* out, int64_t rows, int64_t cols, int dtype,
                               dxa_stream_t stream) {
  DXA_CHECK_ARG(x && out && rows >= 0 && cols > 0 && ld >= cols && (dtype == DXA_F32 || dtype == DXA_BF16),
                "dxa_argmax_rows: bad args");
  if (rows == 0) return DXA_OK;
  const size_t es = dtype == DXA_BF16 ? 2 : 4;
  const bool vec = cols % 4 == 0 && ld % 4 == 0 && al(x, 4 * es);
  dim3 grid((unsigned)rows);
  if (dtype == DXA_BF16 && rows <= 64 && cols >= 16384 && cols < (1ll << 31) && cols % 8 == 0 && ld % 8 == 0 && al(x, 16)) {
    hipLaunchKernelGGL(argmax_rows_wide_k, grid, dim3(1024), 0, ST, (const bf16_t*)x, ld, out, (int)cols);
    DXA_CHECK_LAUNCH();
    return DXA_OK;
  }
  if (dtype == DXA_BF16) {
    if (vec) hipLaunchKernelGGL((argmax_rows_k<bf16_t, 4>), grid, dim3(256), 0, ST, (const bf16_t*)x, ld, out, cols);
    else hipLaunchKernelGGL((argmax_rows_k<bf16_t, 1>), grid, dim3(256), 0, ST, (const bf16_t*)x, ld, out, cols);
  } else {
    if (vec) hipLaunchKernelGGL((argmax_rows_k<float, 4>), grid, dim3(256), 0, ST, (const float*)x, ld, out, cols);
    else hipLaunchKernelGGL((argmax_rows_k<float, 1>), grid, dim3(256), 0, ST, (const float*)x, ld, out, cols);
  }
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}

// ------------------------------------------------------------------------- cross-entropy, hard and soft targets
// One kernel pair serves dxa_cross_entropy_* and dxa_soft_cross_entropy_*.  dexbotic/model/navila/loss.py soft_cross_entropy: a row
// whose label is one of the K soft ("time") token ids is scored against a Gaussian over those ids centred on the label; every other
// row is the plain cross-entropy.  dxa_cross_entropy_* launches the pair with K = 0 (no soft ids: every row is a plain one).
namespace {

constexpr int SOFT_CE_MAX_K = 64;

// index of `lab` among the soft ids or -1
__device__ __forceinline__ int soft_find(const int64_t* __restrict__ ids, int K, int64_t lab) {
  for (int k = 0; k < K; ++k)
    if (ids[k] == lab) return k;
  return -1;
}
// un-normalised Gaussian weight of soft id `s` for label `lab`: fp32 from the integer difference
__device__ __forceinline__ float soft_weight(int64_t lab, int64_t s, float inv2s2) {
  const float d = (float)(lab - s);
  return expf(-(d * d) * inv2s2);
}

template <typename T, int VEC>
__global__ __launch_bounds__(256) void soft_ce_fwd_k(const T* __restrict__ logits, int64_t ld, const int64_t* __restrict__ labels,
                                                     float* __restrict__ row_loss, float* __restrict__ lse_out, int64_t V,
                                                     int64_t ignore_index, const int64_t* __restrict__ soft_ids, int K,
                                                     float inv2s2) {
  __shared__ float red_m[4], red_s[4];
  const int64_t r = blockIdx.x;
  const T* x = logits + r * ld;
  float m = -INFINITY, s = 0.f;
  for (int64_t i = (int64_t)threadIdx.x * VEC; i < V; i += 256 * VEC) {
    float v[VEC];
    Vec<T, VEC>::ld(v, x + i);
    float vm = v[0];
#pragma unroll
    for (int e = 1; e < VEC; ++e) vm = fmaxf(vm, v[e]);
    const float mn = fmaxf(m, vm);
    const float sh = fmaxf(mn, -3.4028235e38f);  // (-FLT_MAX) nothing but -inf seen yet: a finite shift, so every term is exp(-inf) = 0, not exp(NaN)
    float acc = s * expf(m - sh);          // m = -inf on the first visit: s = 0, exp(-inf) = 0
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc += expf(v[e] - sh);    // a NaN entry (fmaxf passes it by) makes s NaN for good
    m = mn; s = acc;
  }
  // fold (m, s) pairs: wave shuffle, then the 4 waves through LDS
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
    const float mn = fmaxf(m, m2);
    const float sh = (mn == -INFINITY) ? 0.f : mn;        // as in the loop above: 0 + 0, and a NaN sum stays NaN
    s = s * expf(m - sh) + s2 * expf(m2 - sh);
    m = mn;
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) { red_m[w] = m; red_s[w] = s; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float M = red_m[0], S = red_s[0];
    for (int i = 1; i < 4; ++i) {
      const float mn = fmaxf(M, red_m[i]);
      const float sh = (mn == -INFINITY) ? 0.f : mn;
      S = S * expf(M - sh) + red_s[i] * expf(red_m[i] - sh);
      M = mn;
    }
    const float lse = M + logf(S);
    lse_out[r] = lse;
    const int64_t lab = labels[r];
    const bool ign = (lab == ignore_index || lab < 0 || lab >= V);
    if (ign || soft_find(soft_ids, K, lab) < 0) {
      row_loss[r] = ign ? 0.f : lse - ldf<T>(x + lab);
    } else {
      float den = 0.f, dot = 0.f;
      for (int k = 0; k < K; ++k) {                        // K <= 64 ids, in the order given
        const int64_t sk = soft_ids[k];
        if (sk < 0 || sk >= V) continue;                   // (refused on the host; never read out of the row)
        const float e = soft_weight(lab, sk, inv2s2);
        den += e;
        dot += e * ldf<T>(x + sk);
      }
      row_loss[r] = lse - dot / den;
    }
  }
}

// dlogits = (softmax(x) - onehot(label)) * g ; g = gscale[0] * scale ; ignored rows -> 0.  May run in place.
// A soft row first keeps z[s_k] of its K soft ids (dlogits may alias logits), writes softmax * g everywhere, and then
// the K soft columns once more as (softmax - p_k) * g: one rounding per element, no search per element.  SOFT = false (launched
// for K = 0) compiles the soft rows' LDS and branches away: with them the K = 0 launch measured 2 - 6 us over 120 - 126 us at
// [512, 152064] bf16 (profiles/ce_merge.txt).  ROWW (dxa_cross_entropy_rows_bwd with a row_w): one more factor of g per row, read
// once per workgroup; a compile-time flag for the same reason, so the other entry points launch the code they always did.
template <typename T, int VEC, bool SOFT, bool ROWW>
__global__ __launch_bounds__(256) void soft_ce_bwd_k(const T* logits, int64_t ld, const int64_t* __restrict__ labels,
                                                     const float* __restrict__ lse, const float* __restrict__ gscale, float scale,
                                                     T* dlogits, int64_t ldd, int64_t V, int64_t ignore_index,
                                                     const int64_t* __restrict__ soft_ids, int K, float inv2s2,
                                                     const float* __restrict__ row_w) {
  __shared__ float sz[SOFT_CE_MAX_K], se[SOFT_CE_MAX_K];
  const int64_t r = blockIdx.x;
  const T* x = logits + r * ld;
  T* d = dlogits + r * ldd;
  int64_t lab = labels[r];
  const bool ign = (lab == ignore_index || lab < 0 || lab >= V);
  float g = ign ? 0.f : (gscale ? gscale[0] : 1.f) * scale;
  if constexpr (ROWW) {
    if (!ign) g *= row_w[r];
  }
  const float l = lse[r];
  const bool soft = SOFT && !ign && soft_find(soft_ids, K, lab) >= 0;  // uniform over the workgroup
  if (soft) {
    if ((int)threadIdx.x < K) {
      const int64_t sk = soft_ids[threadIdx.x];
      const bool in = sk >= 0 && sk < V;
      sz[threadIdx.x] = in ? ldf<T>(x + sk) : 0.f;
      se[threadIdx.x] = in ? soft_weight(lab, sk, inv2s2) : 0.f;
    }
    __syncthreads();
  }
  const int64_t hot = soft ? -1 : lab;
  for (int64_t i = (int64_t)threadIdx.x * VEC; i < V; i += 256 * VEC) {
    float v[VEC];
    Vec<T, VEC>::ld(v, x + i);
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const float p = ign ? 0.f : expf(v[e] - l);
      v[e] = (p - ((i + e) == hot ? 1.f : 0.f)) * g;
    }
    Vec<T, VEC>::st(d + i, v);
  }
  if (soft) {
    __syncthreads();                                       // the row is written: now the K soft columns, one thread each
    if ((int)threadIdx.x < K) {
      const int64_t sk = soft_ids[threadIdx.x];
      if (sk >= 0 && sk < V) {
        float den = 0.f;
        for (int k = 0; k < K; ++k) den += se[k];          // the forward's order of additions
        stf<T>(d + sk, (expf(sz[threadIdx.x] - l) - se[threadIdx.x] / den) * g);
      }
    }
  }
}

int check_soft_ids(const char* who, const int64_t* soft_ids, const int64_t* host, int K, int64_t V) {
  DXA_CHECK_ARG(K >= 0 && K <= SOFT_CE_MAX_K, "%s: K = %d soft ids (0 .. %d supported)", who, K, SOFT_CE_MAX_K);
  if (K == 0) return DXA_OK;
  DXA_CHECK_ARG(soft_ids && host, "%s: soft_ids and soft_ids_host are required when K > 0", who);
  for (int k = 0; k < K; ++k) {
    DXA_CHECK_ARG(host[k] >= 0 && host[k] < V, "%s: soft id %lld (index %d) outside the vocabulary [0, %lld)", who,
                  (long long)host[k], k, (long long)V);
    for (int j = 0; j < k; ++j)
      DXA_CHECK_ARG(host[j] != host[k], "%s: duplicate soft id %lld", who, (long long)host[k]);
  }
  return DXA_OK;
}

// argument checks and launch of both forward entry points; `who` names the caller in the error text
int ce_fwd_launch(const char* who, const void* logits, int64_t ld, const int64_t* labels, float* row_loss, float* lse, int64_t rows,
                  int64_t V, int64_t ignore_index, const int64_t* soft_ids, const int64_t* soft_ids_host, int K, float inv2s2,
                  int dtype, dxa_stream_t stream) {
  DXA_CHECK_ARG(logits && labels && row_loss && lse && rows >= 0 && V > 0 && ld >= V &&
                (dtype == DXA_F32 || dtype == DXA_BF16), "%s: bad args", who);
  if (int rc = check_soft_ids(who, soft_ids, soft_ids_host, K, V)) return rc;
  if (rows == 0) return DXA_OK;
  const size_t es = dtype == DXA_BF16 ? 2 : 4;
  const bool vec = V % 4 == 0 && ld % 4 == 0 && al(logits, 4 * es);
  dim3 grid((unsigned)rows);
#define CE_FWD(T_, V_) hipLaunchKernelGGL((soft_ce_fwd_k<T_, V_>), grid, dim3(256), 0, ST, (const T_*)logits, ld, labels, row_loss, lse, V, ignore_index, soft_ids, K, inv2s2)
  if (dtype == DXA_BF16) { if (vec) CE_FWD(bf16_t, 4); else CE_FWD(bf16_t, 1); }
  else { if (vec) CE_FWD(float, 4); else CE_FWD(float, 1); }
#undef CE_FWD
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}

int ce_bwd_launch(const char* who, const void* logits, int64_t ld, const int64_t* labels, const float* lse, const float* gscale,
                  float scale, void* dlogits, int64_t ldd, int64_t rows, int64_t V, int64_t ignore_index, const int64_t* soft_ids,
                  const int64_t* soft_ids_host, int K, float inv2s2, const float* row_w, int dtype, dxa_stream_t stream) {
  DXA_CHECK_ARG(logits && labels && lse && dlogits && rows >= 0 && V > 0 && ld >= V && ldd >= V &&
                (dtype == DXA_F32 || dtype == DXA_BF16), "%s: bad args", who);
  if (int rc = check_soft_ids(who, soft_ids, soft_ids_host, K, V)) return rc;
  if (rows == 0) return DXA_OK;
  const size_t es = dtype == DXA_BF16 ? 2 : 4;
  const bool vec = V % 4 == 0 && ld % 4 == 0 && ldd % 4 == 0 && al(logits, 4 * es) && al(dlogits, 4 * es);
  dim3 grid((unsigned)rows);
#define CE_BWD_S(T_, V_, S_, W_) hipLaunchKernelGGL((soft_ce_bwd_k<T_, V_, S_, W_>), grid, dim3(256), 0, ST, (const T_*)logits, ld, labels, lse, gscale, scale, (T_*)dlogits, ldd, V, ignore_index, soft_ids, K, inv2s2, row_w)
#define CE_BWD(T_, V_) do { if (K > 0) CE_BWD_S(T_, V_, true, false); else if (row_w) CE_BWD_S(T_, V_, false, true); /* (no entry point passes row_w with soft ids) */ else CE_BWD_S(T_, V_, false, false); } while (0)
  if (dtype == DXA_BF16) { if (vec) CE_BWD(bf16_t, 4); else CE_BWD(bf16_t, 1); }
  else { if (vec) CE_BWD(float, 4); else CE_BWD(float, 1); }
#undef CE_BWD
#undef CE_BWD_S
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}

}  // namespace

extern "C" int dxa_cross_entropy_fwd(const void* logits, int64_t ld, const int64_t* labels, float* row_loss, float* lse,
                                     int64_t rows, int64_t V, int64_t ignore_index, int dtype, dxa_stream_t stream) {
  return ce_fwd_launch("dxa_cross_entropy_fwd", logits, ld, labels, row_loss, lse, rows, V, ignore_index, nullptr, nullptr, 0, 0.f,
                       dtype, stream);
}

extern "C" int dxa_cross_entropy_bwd(const void* logits, int64_t ld, const int64_t* labels, const float* lse,
                                     const float* gscale, float scale, void* dlogits, int64_t ldd, int64_t rows, int64_t V,
                                     int64_t ignore_index, int dtype, dxa_stream_t stream) {
  return ce_bwd_launch("dxa_cross_entropy_bwd", logits, ld, labels, lse, gscale, scale, dlogits, ldd, rows, V, ignore_index, nullptr,
                       nullptr, 0, 0.f, nullptr, dtype, stream);
}

extern "C" int dxa_cross_entropy_rows_bwd(const void* logits, int64_t ld, const int64_t* labels, const float* lse,
                                          const float* gscale, float scale, const float* row_w, void* dlogits, int64_t ldd,
                                          int64_t rows, int64_t V, int64_t ignore_index, int dtype, dxa_stream_t stream) {
  return ce_bwd_launch("dxa_cross_entropy_rows_bwd", logits, ld, labels, lse, gscale, scale, dlogits, ldd, rows, V, ignore_index,
                       nullptr, nullptr, 0, 0.f, row_w, dtype, stream);
}

extern "C" int dxa_soft_cross_entropy_fwd(const void* logits, int64_t ld, const int64_t* labels, float* row_loss, float* lse,
                                          int64_t rows, int64_t V, int64_t ignore_index, const int64_t* soft_ids,
                                          const int64_t* soft_ids_host, int K, float inv2s2, int dtype, dxa_stream_t stream) {
  return ce_fwd_launch("dxa_soft_cross_entropy_fwd", logits, ld, labels, row_loss, lse, rows, V, ignore_index, soft_ids, soft_ids_host,
                       K, inv2s2, dtype, stream);
}

extern "C" int dxa_soft_cross_entropy_bwd(const void* logits, int64_t ld, const int64_t* labels, const float* lse,
                                          const float* gscale, float scale, void* dlogits, int64_t ldd, int64_t rows, int64_t V,
                                          int64_t ignore_index, const int64_t* soft_ids, const int64_t* soft_ids_host, int K,
                                          float inv2s2, int dtype, dxa_stream_t stream) {
  return ce_bwd_launch("dxa_soft_cross_entropy_bwd", logits, ld, labels, lse, gscale, scale, dlogits, ldd, rows, V, ignore_index,
                       soft_ids, soft_ids_host, K, inv2s2, nullptr, dtype, stream);
}

// ------------------------------------------------------------------- per-sample reduction and expectile loss (MuVLA)
// dexbotic/model/muvla/muvla_arch.py:559-592.  The language loss is the mean over the samples of w_b * (sum of the sample's row
// losses) / max(n_b, 1), w_b = 1 + sigmoid(reward_b); the reward head is trained with an expectile-weighted squared error.
namespace {

// one workgroup, sample after sample in order; a sample's rows are summed in double through a fixed LDS tree (sum_f32_k's)
__global__ __launch_bounds__(1024) void ce_sample_reduce_k(const float* __restrict__ row_loss, const int64_t* __restrict__ labels,
                                                           const float* __restrict__ reward, float* __restrict__ row_w,
                                                           float* __restrict__ loss, int64_t B, int64_t L, int64_t V,
                                                           int64_t ignore_index) {
  __shared__ double red_s[1024];
  __shared__ int red_n[1024];
  double total = 0.0;                                      // thread 0's only
  for (int64_t b = 0; b < B; ++b) {
    double s = 0.0;
    int n = 0;
    for (int64_t t = threadIdx.x; t < L; t += 1024) {
      const int64_t lab = labels[b * L + t];
      if (!(lab == ignore_index || lab < 0 || lab >= V)) { s += (double)row_loss[b * L + t]; ++n; }   // the forward's own rule
    }
    red_s[threadIdx.x] = s;
    red_n[threadIdx.x] = n;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
      if ((int)threadIdx.x < o) { red_s[threadIdx.x] += red_s[threadIdx.x + o]; red_n[threadIdx.x] += red_n[threadIdx.x + o]; }
      __syncthreads();
    }
    const double w = reward ? 1.0 + (double)(1.f / (1.f + expf(-reward[b]))) : 1.0;
    const double den = (double)(red_n[0] > 1 ? red_n[0] : 1) * (double)B;
    const float rw = (float)(w / den);
    for (int64_t t = threadIdx.x; t < L; t += 1024) row_w[b * L + t] = rw;
    if (threadIdx.x == 0) total += w * red_s[0] / den;
    __syncthreads();                                       // red_* are rewritten by the next sample
  }
  if (threadIdx.x == 0) loss[0] = (float)total;
}

__global__ __launch_bounds__(1024) void expectile_loss_k(const float* __restrict__ pred, const float* __restrict__ target,
                                                         float* __restrict__ loss, float* __restrict__ dpred, int64_t n, float tau,
                                                         float gscale) {
  __shared__ float red[16];
  float s = 0.f;
  const float k = 2.f / (float)n * gscale;
  for (int64_t i = threadIdx.x; i < n; i += 1024) {
    const float d = pred[i] - target[i];
    const float w = d < 0.f ? tau : 1.f - tau;
    s += w * d * d;
    if (dpred) dpred[i] = k * w * d;
  }
  const float tot = block_sum(s, red);
  if (threadIdx.x == 0) loss[0] = tot / (float)n;
}

}  // namespace

extern "C" int dxa_ce_sample_reduce(const float* row_loss, const int64_t* labels, const float* reward, float* row_w, float* loss,
                                    int64_t B, int64_t L, int64_t V, int64_t ignore_index, dxa_stream_t stream) {
  DXA_CHECK_ARG(row_loss && labels && row_w && loss, "dxa_ce_sample_reduce: null pointer (row_loss, labels, row_w and loss are required)");
  DXA_CHECK_ARG(B > 0 && L > 0 && V > 0, "dxa_ce_sample_reduce: bad sizes (B %lld, L %lld, V %lld: all must be positive)",
                (long long)B, (long long)L, (long long)V);
  hipLaunchKernelGGL(ce_sample_reduce_k, dim3(1), dim3(1024), 0, ST, row_loss, labels, reward, row_w, loss, B, L, V, ignore_index);
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}

extern "C" int dxa_expectile_loss(const float* pred, const float* target, float* loss, float* dpred, int64_t n, float tau,
                                  float gscale, dxa_stream_t stream) {
  DXA_CHECK_ARG(pred && target && loss, "dxa_expectile_loss: null pointer (pred, target and loss are required)");
  DXA_CHECK_ARG(n > 0, "dxa_expectile_loss: n = %lld (must be positive)", (long long)n);
  DXA_CHECK_ARG(tau > 0.f && tau < 1.f, "dxa_expectile_loss: tau %g outside (0, 1)", (double)tau);
  hipLaunchKernelGGL(expectile_loss_k, dim3(1), dim3(1024), 0, ST, pred, target, loss, dpred, n, tau, gscale);
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}

// ------------------------------------------------------------------------------------ sampled token choice
// dxa_sample_rows: GenerationMixin.generate(do_sample=True) on one [rows, V] logits matrix — temperature, top-k, top-p, softmax and
// the draw (semantics, tie rule and argument checks: include/dexbotic_amd.h).  One 1024-thread workgroup per row; the row (304 KB of
// bf16 at V = 152,064) is read several times, from L2 after the first:
//   1. extremes       largest / smallest key and number of the row's valid entries (neither NaN nor -inf)
//   2. top-k          radix select, 8 bits per pass from the top of the order-preserving integer key of x (bf16: 2 passes, fp32: 4),
//                     counting entries per digit.  For top_k <= 1024 the top_k-th largest of the 1024 per-thread maxima, found the
//                     same way from registers, is a lower bound of the threshold: only the few entries at or above it are counted.
//   3. top-p          one pass for the mass of the top-k set, then the same select with an entry's mass e as its weight
//   4. draw           wave w sums the kept mass of the w-th sixteenth of the index range; the sixteenth that holds u * Z is cut into
//                     sixteen again until it fits one element group per thread, which a workgroup-wide scan resolves
// Mass is kept in fixed point: q = (uint64) (e * 2^40), e = exp(z - max z) in [0, 1].  Sums of integers do not depend on their order,
// so every threshold and the draw are the same bits on every run although the digit histograms are filled with LDS atomics, and the
// partial sums of the draw agree exactly between its steps.  An entry with e < 2^-40 weighs nothing (it is never drawn); the sum of
// what the truncation drops is below V * 2^-40 of the largest entry's weight.
namespace {

typedef unsigned long long u64;

constexpr int SMP_THREADS = 1024;
constexpr int SMP_COPIES = 16;                       // copies of a digit's counter, one per lane & 15: a wave's adds spread over the banks
constexpr float SMP_ONE = 1099511627776.f;           // 2^40

// order-preserving key of a float: a > b <=> key(a) > key(b); -0 = +0; NaN -> 0, below -inf
__device__ __forceinline__ uint32_t f32_key(float x) {
  uint32_t b = __float_as_uint(x);
  if ((b & 0x7fffffffu) > 0x7f800000u) return 0u;
  if (b == 0x80000000u) b = 0u;
  return (b >> 31) ? ~b : (b | 0x80000000u);
}
template <typename T> struct SampleKey;
template <> struct SampleKey<float> { static constexpr int BITS = 32; };
template <> struct SampleKey<bf16_t> { static constexpr int BITS = 16; };   // the low 16 bits of a bf16's fp32 key depend on its sign only
template <typename T> __device__ __forceinline__ uint32_t sample_key(float x) { return f32_key(x) >> (32 - SampleKey<T>::BITS); }
template <typename T> __device__ __forceinline__ float sample_unkey(uint32_t k) {
  k <<= (32 - SampleKey<T>::BITS);
  const uint32_t b = (k >> 31) ? (k & 0x7fffffffu) : ~k;
  return __uint_as_float(b & ~((1u << (32 - SampleKey<T>::BITS)) - 1u));
}

struct SampleShared {
  u64 hist[256 * SMP_COPIES];
  u64 suffix[256];
  u64 wsum[16];
  uint32_t wa[16], wb[16], wc[16], wd[16];
};

__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// inclusive prefix sum over the lanes of a wave
__device__ __forceinline__ u64 wave_scan_u64(u64 v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u64 t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

template <typename T, int VEC>
__global__ __launch_bounds__(SMP_THREADS) void sample_rows_k(const T* __restrict__ logits, int64_t ld, int64_t V, float inv_t,
                                                             int64_t top_k, float top_p, const float* __restrict__ u,
                                                             int64_t* __restrict__ token, int32_t* __restrict__ kept_out,
                                                             float* __restrict__ thresh_out, float* __restrict__ prob_out) {
  __shared__ SampleShared sh;
  constexpr int BITS = SampleKey<T>::BITS;
  constexpr uint32_t KEY_NINF = 0x007fffffu >> (32 - BITS);          // key of -inf: a valid entry's key is larger
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t r = blockIdx.x;
  const T* x = logits + r * ld;

  // every element of the row once, a wave reading consecutive addresses: f(key, value)
  auto sweep = [&](auto&& f) {
    for (int64_t i = (int64_t)tid * VEC; i < V; i += (int64_t)SMP_THREADS * VEC) {      // VEC > 1: V % VEC == 0
      float v[VEC];
      Vec<T, VEC>::ld(v, x + i);
#pragma unroll
      for (int e = 0; e < VEC; ++e) f(sample_key<T>(v[e]), v[e]);
    }
  };
  auto block_sum_u64 = [&](u64 v) -> u64 {
    v = wave_sum_u64(v);
    if (lane == 0) sh.wsum[w] = v;
    __syncthreads();
    u64 t = 0;
    for (int i = 0; i < 16; ++i) t += sh.wsum[i];
    __syncthreads();
    return t;
  };

  // 1. extremes of the valid entries
  uint32_t kmax = 0u, kmin = 0xffffffffu, cnt = 0u;
  sweep([&](uint32_t k, float) {
    if (k > KEY_NINF) { kmax = max(kmax, k); kmin = min(kmin, k); ++cnt; }
  });
  const uint32_t own_max = kmax;                                    // of this thread's entries, 0 without a valid one
  uint32_t nthr = cnt ? 1u : 0u;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    kmax = max(kmax, (uint32_t)__shfl_xor(kmax, o, 64));
    kmin = min(kmin, (uint32_t)__shfl_xor(kmin, o, 64));
    cnt += __shfl_xor(cnt, o, 64);
    nthr += __shfl_xor(nthr, o, 64);
  }
  if (lane == 0) { sh.wa[w] = kmax; sh.wb[w] = kmin; sh.wc[w] = cnt; sh.wd[w] = nthr; }
  __syncthreads();
  kmax = 0u; kmin = 0xffffffffu; cnt = 0u; nthr = 0u;
  for (int i = 0; i < 16; ++i) { kmax = max(kmax, sh.wa[i]); kmin = min(kmin, sh.wb[i]); cnt += sh.wc[i]; nthr += sh.wd[i]; }
  __syncthreads();
  if (cnt == 0u) {                                                  // no finite logit: index 0, as dxa_argmax_rows
    if (tid == 0) {
      token[r] = 0;
      if (kept_out) kept_out[r] = 0;
      if (thresh_out) thresh_out[r] = INFINITY;
      if (prob_out) prob_out[r] = 0.f;
    }
    return;
  }

  const float zmax = sample_unkey<T>(kmax) * inv_t;
  auto weight = [&](float v) -> u64 {                               // e = exp(z - max z) in fixed point; the maximum weighs exactly 2^40
    const float z = v * inv_t;
    const float e = (z == zmax) ? 1.f : expf(z - zmax);
    return (u64)(e * SMP_ONE);
  };

  // Radix select over the entries `sw` visits whose key is >= floor: the largest key t with weight{key >= t} >= target, weight = 1
  // (count) or the entry's mass.  The caller guarantees 1 <= target <= weight{key >= floor}.
  auto select = [&](auto&& sw, uint32_t floor, bool mass, u64 target) -> uint32_t {
    uint32_t prefix = 0u;
    u64 above = 0;                                                  // weight of the keys whose leading digits are larger than prefix
    for (int lvl = 0; lvl < BITS / 8; ++lvl) {
      const int shift = BITS - 8 * (lvl + 1);
      for (int i = tid; i < 256 * SMP_COPIES; i += SMP_THREADS) sh.hist[i] = 0;
      __syncthreads();
      sw([&](uint32_t k, float v) {
        if (k >= floor && (lvl == 0 || (k >> (shift + 8)) == prefix))
          atomicAdd(&sh.hist[((k >> shift) & 255u) * SMP_COPIES + (lane & (SMP_COPIES - 1))], mass ? weight(v) : (u64)1);
      });
      __syncthreads();
      u64 s = 0;
      if (tid < 256) {                                              // thread t owns digit 255 - t: a prefix sum over t is a suffix sum over digits
        const int d = 255 - tid;
        for (int c = 0; c < SMP_COPIES; ++c) s += sh.hist[d * SMP_COPIES + ((c + tid) & (SMP_COPIES - 1))];
        s = wave_scan_u64(s, lane);
        if (lane == 63) sh.wsum[w] = s;
      }
      __syncthreads();
      if (tid < 256) {
        for (int i = 0; i < w; ++i) s += sh.wsum[i];
        sh.suffix[tid] = s;                                         // weight of the digits >= 255 - t
        const u64 short_of = __ballot(above + s < target);
        if (lane == 0) sh.wa[w] = (uint32_t)__popcll(short_of);
      }
      __syncthreads();
      int t = (int)(sh.wa[0] + sh.wa[1] + sh.wa[2] + sh.wa[3]);     // digits 255 .. 256 - t together stay short of the target
      if (t > 255) t = 255;
      if (t > 0) above += sh.suffix[t - 1];
      prefix = (prefix << 8) | (uint32_t)(255 - t);
      __syncthreads();
    }
    return prefix;
  };

  uint32_t tkey = kmin;                                             // smallest kept key

  // 2. top-k: the top_k-th largest key, ties with it kept
  if (top_k > 0 && top_k < V && (u64)top_k < (u64)cnt) {
    uint32_t floor = KEY_NINF + 1u;
    if ((u64)top_k <= (u64)nthr)
      floor = select([&](auto&& f) { if (own_max > KEY_NINF) f(own_max, 0.f); }, floor, false, (u64)top_k);
    tkey = select(sweep, floor, false, (u64)top_k);
  }

  // 3. top-p over what top-k kept: an entry stays iff the mass of the strictly larger entries is < top_p * Z
  if (top_p < 1.f) {
    u64 z = 0;
    sweep([&](uint32_t k, float v) { if (k >= tkey) z += weight(v); });
    z = block_sum_u64(z);
    const double want = ceil((double)top_p * (double)z);
    u64 target = want >= (double)z ? z : (u64)want;
    if (target < 1) target = 1;
    tkey = select(sweep, tkey, true, target);
  }

  // 4. draw: first index, in ascending order, whose running kept mass exceeds u * Z
  int64_t lo = 0, hi = V;
  u64 target = 0, zq = 0;
  uint32_t kept = 0u;
  for (bool first = true;; first = false) {
    const int64_t len = hi - lo;
    if (!first && len <= (int64_t)SMP_THREADS * VEC) break;
    const int64_t span = ((len + 15) / 16 + 64 * VEC - 1) / (64 * VEC) * (64 * VEC);   // of one wave
    const int64_t a = lo + (int64_t)w * span, b = min(hi, a + span);
    u64 s = 0;
    uint32_t c = 0u;
    for (int64_t i = a + (int64_t)lane * VEC; i < b; i += 64 * VEC) {
      float v[VEC];
      Vec<T, VEC>::ld(v, x + i);
#pragma unroll
      for (int e = 0; e < VEC; ++e)
        if (sample_key<T>(v[e]) >= tkey) { s += weight(v[e]); ++c; }
    }
    s = wave_sum_u64(s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane == 0) { sh.wsum[w] = s; sh.wa[w] = c; }
    __syncthreads();
    if (first) {
      for (int i = 0; i < 16; ++i) { zq += sh.wsum[i]; kept += sh.wa[i]; }
      double t = (double)u[r] * (double)zq;
      if (!(t >= 0.0)) t = 0.0;
      target = t >= (double)zq ? zq - 1 : (u64)t;                   // u >= 1 or rounding: the last kept entry that weighs something
    }
    int ws = 0;
    u64 before = 0;
    for (; ws < 15; ++ws) {
      if (before + sh.wsum[ws] > target) break;
      before += sh.wsum[ws];
    }
    target -= before;
    lo += (int64_t)ws * span;
    hi = min(hi, lo + span);
    __syncthreads();
  }
  {
    const int64_t i = lo + (int64_t)tid * VEC;
    u64 q[VEC];
    u64 s = 0;
#pragma unroll
    for (int e = 0; e < VEC; ++e) q[e] = 0;
    if (i < hi) {
      float v[VEC];
      Vec<T, VEC>::ld(v, x + i);
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        if (sample_key<T>(v[e]) >= tkey) q[e] = weight(v[e]);
        s += q[e];
      }
    }
    u64 inc = wave_scan_u64(s, lane);
    if (lane == 63) sh.wsum[w] = inc;
    __syncthreads();
    for (int k = 0; k < w; ++k) inc += sh.wsum[k];
    u64 run = inc - s;
    if (run <= target && target < inc) {                            // exactly one thread: target < the mass of [lo, hi)
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const bool was_short = run <= target;
        run += q[e];
        if (was_short && run > target) {
          token[r] = i + e;
          if (prob_out) prob_out[r] = (float)q[e] / (float)zq;
        }
      }
    }
    if (tid == 0) {
      if (kept_out) kept_out[r] = (int32_t)kept;
      if (thresh_out) thresh_out[r] = sample_unkey<T>(tkey);
    }
  }
}

}  // namespace

extern "C" int dxa_sample_rows(const void* logits, int64_t ld, int64_t rows, int64_t V, int dtype, float temperature,
                               int64_t top_k, float top_p, const float* u, int64_t* token, int32_t* kept, float* thresh,
                               float* prob, dxa_stream_t stream) {
  DXA_CHECK_ARG(logits && u && token, "dxa_sample_rows: null pointer (logits, u and token are required)");
  DXA_CHECK_ARG(dtype == DXA_F32 || dtype == DXA_BF16, "dxa_sample_rows: dtype %d (DXA_F32 or DXA_BF16)", dtype);
  DXA_CHECK_ARG(rows >= 0 && rows <= INT_MAX && V > 0 && V < (1ll << 31) && ld >= V,
                "dxa_sample_rows: bad shape (rows %lld, V %lld, ld %lld: rows >= 0, 0 < V < 2^31, ld >= V)", (long long)rows,
                (long long)V, (long long)ld);
  DXA_CHECK_ARG(temperature > 0.f && temperature < INFINITY, "dxa_sample_rows: temperature %g (must be positive and finite)",
                (double)temperature);
  DXA_CHECK_ARG(top_p > 0.f && top_p <= 1.f, "dxa_sample_rows: top_p %g outside (0, 1]", (double)top_p);
  if (rows == 0) return DXA_OK;
  const bool vec = V % 8 == 0 && ld % 8 == 0 && al(logits, 16);     // every row starts on a 16-byte boundary
  const float inv_t = 1.f / temperature;
  dim3 grid((unsigned)rows);
#define SAMPLE(T_, V_) hipLaunchKernelGGL((sample_rows_k<T_, V_>), grid, dim3(SMP_THREADS), 0, ST, (const T_*)logits, ld, V, inv_t, top_k, top_p, u, token, kept, thresh, prob)
  if (dtype == DXA_BF16) { if (vec) SAMPLE(bf16_t, 8); else SAMPLE(bf16_t, 1); }
  else { if (vec) SAMPLE(float, 4); else SAMPLE(float, 1); }
#undef SAMPLE
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}
