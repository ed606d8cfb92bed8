// GRPO policy update of the OFT-discrete policy for gfx950 (see include/dexbotic_amd.h): the learning side of the reference's
// SimpleVLA-RL post-training (dexbotic/exp/rl/rl_trainer.py).
//   dxa_bin_logprob_fwd : logprobs_from_logits_naive + entropy_from_logits (rl_trainer.py:46-55) on the num_bins - 1 bin logits of
//                         every action row, after `logits.div(temperature)` (rl_trainer.py:354-359, 392-396)
//   dxa_ppo_clip_fwd    : _compute_policy_loss (rl_trainer.py:488-506) as four masked sums, and d loss / d log_prob per token
//   dxa_bin_logprob_bwd : d loss / d logits from the per-row coefficient
// The bin kernels are one wave per row, four rows per 256-thread workgroup: a row is num_bins - 1 = 255 logits (four per lane), the
// whole operand of an update chunk 448 x 255 elements.  Rows are read with scalar loads: 255 elements are no multiple of a vector, a
// row starts at any element, and the operand is a fraction of a megabyte — these launches are bound by their latency, not by bytes.
// Every reduction is a fixed xor butterfly (bin kernels) or block_sum (the clip kernel, one workgroup): no atomics, the same bits on
// every run.
#include "common.h"

namespace {

constexpr int BLP_ROWS = 4;                            // rows (= waves) per workgroup

template <typename T>
__global__ __launch_bounds__(256) void bin_logprob_fwd_k(const T* __restrict__ logits, int64_t ld, const int64_t* __restrict__ bins,
                                                         float inv_t, float* __restrict__ logp, float* __restrict__ entropy,
                                                         float* __restrict__ lse_out, int64_t rows, int NB) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * BLP_ROWS + (threadIdx.x >> 6);
  if (r >= rows) return;                               // wave-uniform; no workgroup barrier below
  const T* x = logits + r * ld;
  float m = -INFINITY;
  for (int j = lane; j < NB; j += 64) m = fmaxf(m, ldf<T>(x + j) * inv_t);
  m = wave_max(m);
  float s = 0.f, t = 0.f;
  for (int j = lane; j < NB; j += 64) {
    const float z = ldf<T>(x + j) * inv_t;
    const float e = expf(z - m);
    s += e;
    t += e * z;
  }
  s = wave_sum(s);
  t = wave_sum(t);
  if (lane == 0) {
    const float lse = m + logf(s);
    const int64_t b = bins[r];
    lse_out[r] = lse;
    entropy[r] = lse - t / s;
    logp[r] = (b >= 0 && b < NB) ? ldf<T>(x + b) * inv_t - lse : NAN;
  }
}

// dlogits may alias logits: a lane writes only the elements it has read itself
template <typename T>
__global__ __launch_bounds__(256) void bin_logprob_bwd_k(const T* logits, int64_t ld, const int64_t* __restrict__ bins,
                                                         const float* __restrict__ lse, const float* __restrict__ coef,
                                                         const float* __restrict__ gscale, float inv_t, T* dlogits, int64_t rows,
                                                         int NB) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * BLP_ROWS + (threadIdx.x >> 6);
  if (r >= rows) return;
  const T* x = logits + r * ld;
  T* d = dlogits + r * ld;
  const float c = coef[r];
  if (c == 0.f) {                                      // a masked token: zeros, whatever its logits hold
    for (int j = lane; j < NB; j += 64) stf<T>(d + j, 0.f);
    return;
  }
  const float g = c * (gscale ? gscale[0] : 1.f) * inv_t;
  const float l = lse[r];
  const int64_t b = bins[r];
  for (int j = lane; j < NB; j += 64) {
    const float p = expf(ldf<T>(x + j) * inv_t - l);
    stf<T>(d + j, g * (((int64_t)j == b ? 1.f : 0.f) - p));
  }
}

// One workgroup, like l1_loss_k.  A masked token contributes exactly 0 to every sum and gets coef 0, also where its values are not
// finite.  inv_denom > 0: the caller's normaliser; otherwise 1 / sum(mask) (masked_mean), 0 for an empty mask.
template <typename M>
__global__ __launch_bounds__(1024) void ppo_clip_fwd_k(const float* __restrict__ logp, const float* __restrict__ old_logp,
                                                       const float* __restrict__ adv, const M* __restrict__ mask, int64_t n,
                                                       float clip_low, float clip_high, float inv_denom, float* __restrict__ sums,
                                                       float* __restrict__ loss, float* __restrict__ coef) {
  __shared__ float red[16];
  const float lo = 1.f - clip_low, hi = 1.f + clip_high;
  float s_loss = 0.f, s_clip = 0.f, s_kl = 0.f, s_cnt = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += 1024) {
    float c = 0.f;
    if (mask[i] != (M)0) {
      const float lp = logp[i], ol = old_logp[i], a = adv[i];
      const float ratio = expf(lp - ol);
      const float pg1 = -a * ratio;
      const float pg2 = -a * fminf(fmaxf(ratio, lo), hi);
      s_loss += fmaxf(pg1, pg2);
      s_clip += pg2 > pg1 ? 1.f : 0.f;
      s_kl += ol - lp;
      s_cnt += 1.f;
      c = pg1 >= pg2 ? pg1 : 0.f;                      // torch.maximum / clamp autograd, ties included (include/dexbotic_amd.h)
    }
    coef[i] = inv_denom > 0.f ? c * inv_denom : c;
  }
  const float t_loss = block_sum(s_loss, red);
  const float t_clip = block_sum(s_clip, red);
  const float t_kl = block_sum(s_kl, red);
  const float t_cnt = block_sum(s_cnt, red);
  const float inv = inv_denom > 0.f ? inv_denom : (t_cnt > 0.f ? 1.f / t_cnt : 0.f);
  if (!(inv_denom > 0.f))
    for (int64_t i = threadIdx.x; i < n; i += 1024) coef[i] *= inv;      // the elements this thread wrote itself
  if (threadIdx.x == 0) {
    sums[0] = t_loss; sums[1] = t_clip; sums[2] = t_kl; sums[3] = t_cnt;
    if (loss) loss[0] = t_loss * inv;
  }
}

int bin_args(const char* who, int64_t ld, int64_t rows, int64_t NB, int dtype) {
  DXA_CHECK_ARG(dtype == DXA_F32 || dtype == DXA_BF16, "%s: dtype %d (DXA_F32 or DXA_BF16)", who, dtype);
  DXA_CHECK_ARG(NB >= 1 && NB <= (1 << 16), "%s: NB = %lld outside [1, 65536]", who, (long long)NB);
  DXA_CHECK_ARG(ld >= NB, "%s: ld = %lld below NB = %lld", who, (long long)ld, (long long)NB);
  DXA_CHECK_ARG(rows >= 0 && rows <= (1ll << 30), "%s: rows = %lld outside [0, 2^30]", who, (long long)rows);
  return DXA_OK;
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int dxa_bin_logprob_fwd(const void* logits, int64_t ld, const int64_t* bins, float inv_temperature, float* logp,
                                   float* entropy, float* lse, int64_t rows, int64_t NB, int dtype, dxa_stream_t stream) {
  DXA_CHECK_ARG(logits && bins && logp && entropy && lse, "dxa_bin_logprob_fwd: null pointer (logits, bins, logp, entropy and lse are required)");
  if (int rc = bin_args("dxa_bin_logprob_fwd", ld, rows, NB, dtype)) return rc;
  DXA_CHECK_ARG(inv_temperature > 0.f && inv_temperature < INFINITY, "dxa_bin_logprob_fwd: inv_temperature %g (must be positive and finite)",
                (double)inv_temperature);
  if (rows == 0) return DXA_OK;
  dim3 grid((unsigned)((rows + BLP_ROWS - 1) / BLP_ROWS));
  if (dtype == DXA_BF16)
    hipLaunchKernelGGL((bin_logprob_fwd_k<bf16_t>), grid, dim3(256), 0, ST, (const bf16_t*)logits, ld, bins, inv_temperature, logp,
                       entropy, lse, rows, (int)NB);
  else
    hipLaunchKernelGGL((bin_logprob_fwd_k<float>), grid, dim3(256), 0, ST, (const float*)logits, ld, bins, inv_temperature, logp,
                       entropy, lse, rows, (int)NB);
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}

extern "C" int dxa_bin_logprob_bwd(const void* logits, int64_t ld, const int64_t* bins, const float* lse, const float* coef,
                                   const float* gscale, float inv_temperature, void* dlogits, int64_t rows, int64_t NB, int dtype,
                                   dxa_stream_t stream) {
  DXA_CHECK_ARG(logits && bins && lse && coef && dlogits, "dxa_bin_logprob_bwd: null pointer (logits, bins, lse, coef and dlogits are required)");
  if (int rc = bin_args("dxa_bin_logprob_bwd", ld, rows, NB, dtype)) return rc;
  DXA_CHECK_ARG(inv_temperature > 0.f && inv_temperature < INFINITY, "dxa_bin_logprob_bwd: inv_temperature %g (must be positive and finite)",
                (double)inv_temperature);
  if (rows == 0) return DXA_OK;
  dim3 grid((unsigned)((rows + BLP_ROWS - 1) / BLP_ROWS));
  if (dtype == DXA_BF16)
    hipLaunchKernelGGL((bin_logprob_bwd_k<bf16_t>), grid, dim3(256), 0, ST, (const bf16_t*)logits, ld, bins, lse, coef, gscale,
                       inv_temperature, (bf16_t*)dlogits, rows, (int)NB);
  else
    hipLaunchKernelGGL((bin_logprob_bwd_k<float>), grid, dim3(256), 0, ST, (const float*)logits, ld, bins, lse, coef, gscale,
                       inv_temperature, (float*)dlogits, rows, (int)NB);
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}

extern "C" int dxa_ppo_clip_fwd(const float* logp, const float* old_logp, const float* adv, const void* mask, int mask_u8, int64_t n,
                                float clip_low, float clip_high, float inv_denom, float* sums, float* loss, float* coef,
                                dxa_stream_t stream) {
  DXA_CHECK_ARG(logp && old_logp && adv && mask && sums && coef,
                "dxa_ppo_clip_fwd: null pointer (logp, old_logp, adv, mask, sums and coef are required)");
  DXA_CHECK_ARG(n > 0 && n <= (1ll << 30), "dxa_ppo_clip_fwd: n = %lld outside [1, 2^30]", (long long)n);
  DXA_CHECK_ARG(mask_u8 == 0 || mask_u8 == 1, "dxa_ppo_clip_fwd: mask_u8 = %d (0: fp32 mask, 1: uint8 mask)", mask_u8);
  DXA_CHECK_ARG(clip_low >= 0.f && clip_low < 1.f && clip_high >= 0.f && clip_high < INFINITY,
                "dxa_ppo_clip_fwd: clip range (%g, %g): clip_low in [0, 1) and a finite clip_high >= 0", (double)clip_low, (double)clip_high);
  DXA_CHECK_ARG(inv_denom == inv_denom && inv_denom < INFINITY, "dxa_ppo_clip_fwd: inv_denom %g is not finite", (double)inv_denom);
  if (mask_u8)
    hipLaunchKernelGGL((ppo_clip_fwd_k<uint8_t>), dim3(1), dim3(1024), 0, ST, logp, old_logp, adv, (const uint8_t*)mask, n, clip_low,
                       clip_high, inv_denom, sums, loss, coef);
  else
    hipLaunchKernelGGL((ppo_clip_fwd_k<float>), dim3(1), dim3(1024), 0, ST, logp, old_logp, adv, (const float*)mask, n, clip_low,
                       clip_high, inv_denom, sums, loss, coef);
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}
