// OFT diffusion head kernels (dexbotic/model/oft/oft_arch.py:106-116,147-154,224-250, oft/action_model/model.py:33-55,197-271): the
// first half of the noisy-action projector (a Linear(1, d) and its GELU in one pass, with its fixed-order weight gradients), the
// reserved rows of the spliced sequence written in place (state row, time row, projected noisy-action rows), and the two ends of one
// DDIM step of the cached-prefix sampler.  fp32 arithmetic, 16-byte accesses, fixed summation orders, no atomics.
#include "common.h"

namespace {

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// VEC floats from / to VEC elements of T: 16 bytes per access for (bf16, 8) and (fp32, 4); (fp32, 8) is two 16-byte accesses
template <typename T, int VEC>
__device__ __forceinline__ void ldv(float (&o)[VEC], const T* p) {
  if constexpr (VEC == 8 && sizeof(T) == 4) {
    float a[4], b[4];
    Vec<float, 4>::ld(a, reinterpret_cast<const float*>(p));
    Vec<float, 4>::ld(b, reinterpret_cast<const float*>(p) + 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) { o[i] = a[i]; o[4 + i] = b[i]; }
  } else {
    Vec<T, VEC>::ld(o, p);
  }
}
template <typename T, int VEC>
__device__ __forceinline__ void stv(T* p, const float (&v)[VEC]) {
  if constexpr (VEC == 8 && sizeof(T) == 4) {
    const float a[4] = {v[0], v[1], v[2], v[3]}, b[4] = {v[4], v[5], v[6], v[7]};
    Vec<float, 4>::st(reinterpret_cast<float*>(p), a);
    Vec<float, 4>::st(reinterpret_cast<float*>(p) + 4, b);
  } else {
    Vec<T, VEC>::st(p, v);
  }
}

// first row of sample b's block of `n` rows, or -1 when the block does not lie inside [0, Sq): such a sample is left alone
__device__ __forceinline__ int64_t block_start(const int64_t* __restrict__ off, int64_t b, int64_t n, int64_t Sq) {
  const int64_t o = off[b];
  return (o >= 0 && o + n <= Sq) ? o : -1;
}

// fc1 of the projector on one scalar: the pre-activation as the next op of the compute dtype sees it
template <typename T>
__device__ __forceinline__ float embed_pre(float a, float w, float b) { return rnd<T>(a * w + b); }

// ------------------------------------------------------------------------------------------------ noisy_embed
// one workgroup per noisy-action scalar: h[r, c] = gelu_erf(rnd(a[r]) * w1[c] + b1[c])
template <typename T, typename TW, int VEC>
__global__ __launch_bounds__(256) void noisy_embed_fwd_k(const float* __restrict__ a, const TW* __restrict__ w1,
                                                         const TW* __restrict__ b1, T* __restrict__ h, int64_t d) {
  const int64_t r = blockIdx.x;
  const float ar = rnd<T>(a[r]);
  T* hr = h + r * d;
  for (int64_t c = (int64_t)threadIdx.x * VEC; c < d; c += 256 * VEC) {
    float w[VEC], b[VEC], o[VEC];
    ldv<TW, VEC>(w, w1 + c);
    ldv<TW, VEC>(b, b1 + c);
#pragma unroll
    for (int i = 0; i < VEC; ++i) o[i] = act_fwd(DXA_ACT_GELU_ERF, embed_pre<T>(ar, w[i], b[i]));
    stv<T, VEC>(hr + c, o);
  }
}

constexpr int EMBED_CHUNK = 16;      // rows summed by one workgroup of the first stage

// stage 1, grid (column blocks, chunks): workgroup (x, g) sums dpre = dh * gelu'(pre) (pre recomputed from a, w1, b1) over the rows
// g*16 ... g*16 + 15 in ascending order: partial[g, c] = sum dpre * rnd(a[r]), partial[g, d + c] = sum dpre
template <typename T, typename TW, int VEC>
__global__ __launch_bounds__(256) void noisy_embed_bwd_part_k(const T* __restrict__ dh, const float* __restrict__ a,
                                                              const TW* __restrict__ w1, const TW* __restrict__ b1,
                                                              float* __restrict__ partial, int64_t R, int64_t d) {
  const int64_t c = ((int64_t)blockIdx.x * 256 + threadIdx.x) * VEC;
  if (c >= d) return;
  const int64_t g = blockIdx.y;
  float w[VEC], b[VEC], sw[VEC], sb[VEC];
  ldv<TW, VEC>(w, w1 + c);
  ldv<TW, VEC>(b, b1 + c);
#pragma unroll
  for (int i = 0; i < VEC; ++i) sw[i] = sb[i] = 0.f;
  const int64_t r1 = (g + 1) * EMBED_CHUNK < R ? (g + 1) * EMBED_CHUNK : R;
  for (int64_t r = g * EMBED_CHUNK; r < r1; ++r) {
    const float ar = rnd<T>(a[r]);
    float gv[VEC];
    ldv<T, VEC>(gv, dh + r * d + c);
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      const float dpre = gv[i] * act_grad(DXA_ACT_GELU_ERF, embed_pre<T>(ar, w[i], b[i]));
      sw[i] += dpre * ar;
      sb[i] += dpre;
    }
  }
  stv<float, VEC>(partial + g * 2 * d + c, sw);
  stv<float, VEC>(partial + g * 2 * d + d + c, sb);
}

// stage 2 over the 2 d columns of dw1 | db1: (+)= the chunks' partial rows in ascending order
__global__ __launch_bounds__(256) void noisy_embed_bwd_fold_k(const float* __restrict__ partial, float* __restrict__ dw1,
                                                              float* __restrict__ db1, int64_t d, int64_t chunks, int accumulate) {
  const int64_t c = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (c >= 2 * d) return;
  float s[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) s[i] = 0.f;
  for (int64_t g = 0; g < chunks; ++g) {
    float v[4];
    ldv<float, 4>(v, partial + g * 2 * d + c);
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] += v[i];
  }
  float* out = c < d ? dw1 + c : db1 + (c - d);          // (d % 4 == 0: a group of four lies on one side)
  if (accumulate) {
    float old[4];
    ldv<float, 4>(old, out);
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] = old[i] + s[i];
  }
  stv<float, 4>(out, s);
}

// ------------------------------------------------------------------------------------------------ diffusion_put
// one workgroup per (sample, block row): [state row, with `skip`] [time row] [R projected rows]
template <typename T, int VEC>
__global__ __launch_bounds__(256) void diffusion_put_fwd_k(T* __restrict__ x, const T* __restrict__ proj, const T* __restrict__ time,
                                                           const T* __restrict__ state, const int64_t* __restrict__ off, int64_t Sq,
                                                           int64_t d, int64_t R, int skip) {
  const int64_t Q = R + 1 + skip;
  const int64_t b = blockIdx.x / Q, j = blockIdx.x - b * Q;
  const int64_t o = block_start(off, b, Q, Sq);
  if (o < 0) return;
  const T* src = (skip && j == 0) ? state + b * d : (j == skip ? time + b * d : proj + (b * R + (j - skip - 1)) * d);
  T* xr = x + ((b * Sq + o + j) * d);
  for (int64_t c = (int64_t)threadIdx.x * VEC; c < d; c += 256 * VEC) {
    float v[VEC];
    ldv<T, VEC>(v, src + c);
    stv<T, VEC>(xr + c, v);
  }
}

// workgroups [0, B R): dproj row (b, j) = dx[b, off[b] + skip + 1 + j]; workgroups [B R, B R + B) (with dstate): the state row's
// gradient.  Zeros for a sample whose block is out of range.  The time row has no gradient.
template <typename T, int VEC>
__global__ __launch_bounds__(256) void diffusion_put_bwd_k(const T* __restrict__ dx, const int64_t* __restrict__ off,
                                                           T* __restrict__ dproj, T* __restrict__ dstate, int64_t B, int64_t Sq,
                                                           int64_t d, int64_t R, int skip) {
  const int64_t Q = R + 1 + skip;
  int64_t b, row;
  T* dst;
  if ((int64_t)blockIdx.x < B * R) {
    b = blockIdx.x / R;
    row = skip + 1 + ((int64_t)blockIdx.x - b * R);
    dst = dproj + (int64_t)blockIdx.x * d;
  } else {
    b = (int64_t)blockIdx.x - B * R;
    row = 0;
    dst = dstate + b * d;
  }
  const int64_t o = block_start(off, b, Q, Sq);
  const T* src = dx + ((b * Sq + (o < 0 ? 0 : o + row)) * d);
  for (int64_t c = (int64_t)threadIdx.x * VEC; c < d; c += 256 * VEC) {
    float v[VEC];
    if (o >= 0) {
      ldv<T, VEC>(v, src + c);
    } else {
#pragma unroll
      for (int i = 0; i < VEC; ++i) v[i] = 0.f;
    }
    stv<T, VEC>(dst + c, v);
  }
}

// ------------------------------------------------------------------------------------------------ ddim_step_embed
// workgroup j < n: the DDIM update of x[j] (with eps) and row j of the projector's fc2 operand; workgroup n: the time row
template <typename T, typename TW, int VEC>
__global__ __launch_bounds__(256) void ddim_step_embed_k(const T* __restrict__ eps, float* __restrict__ x, float c0, float c1, float c2,
                                                         float c3, float clip, const T* __restrict__ time_row,
                                                         const TW* __restrict__ w1, const TW* __restrict__ b1, T* __restrict__ suffix,
                                                         T* __restrict__ h, int64_t n, int64_t d) {
  const int64_t j = blockIdx.x;
  if (j == n) {
    for (int64_t c = (int64_t)threadIdx.x * VEC; c < d; c += 256 * VEC) {
      float v[VEC];
      ldv<T, VEC>(v, time_row + c);
      stv<T, VEC>(suffix + c, v);
    }
    return;
  }
  float xv = x[j];
  if (eps) {
    const float e = ldf<T>(eps + j);
    float x0 = c0 * xv - c1 * e;
    if (clip > 0.f) x0 = x0 < -clip ? -clip : (x0 > clip ? clip : x0);       // (a NaN stays a NaN, as in torch.clamp)
    xv = c2 * x0 + c3 * e;
    __syncthreads();                                     // every thread has read x[j]
    if (threadIdx.x == 0) x[j] = xv;
  }
  const float ar = rnd<T>(xv);
  T* hr = h + j * d;
  for (int64_t c = (int64_t)threadIdx.x * VEC; c < d; c += 256 * VEC) {
    float w[VEC], b[VEC], o[VEC];
    ldv<TW, VEC>(w, w1 + c);
    ldv<TW, VEC>(b, b1 + c);
#pragma unroll
    for (int i = 0; i < VEC; ++i) o[i] = act_fwd(DXA_ACT_GELU_ERF, embed_pre<T>(ar, w[i], b[i]));
    stv<T, VEC>(hr + c, o);
  }
}

int check_dtypes(const char* who, int dtype, int w_dtype) {
  if (!(dtype == DXA_F32 || dtype == DXA_BF16) || !(w_dtype == DXA_F32 || w_dtype == DXA_BF16) ||
      (dtype == DXA_F32 && w_dtype == DXA_BF16)) {
    dxa_set_error("%s: unsupported dtype combination (%d,%d)", who, dtype, w_dtype);
    return DXA_ERR_UNSUPPORTED;
  }
  return DXA_OK;
}

// a row of d elements is read and written 16 bytes at a time, in either dtype
int check_width(const char* who, int64_t d) {
  DXA_CHECK_ARG(d >= 8 && d % 8 == 0 && d <= (1 << 20), "%s: d = %lld must be a multiple of 8 in [8, 2^20] (rows are accessed 16 bytes at a time)",
                who, (long long)d);
  return DXA_OK;
}

int check_block(const char* who, int64_t B, int64_t Sq, int64_t R, int skip) {
  DXA_CHECK_ARG(B >= 0 && Sq > 0 && R > 0 && (skip == 0 || skip == 1), "%s: bad sizes B=%lld Sq=%lld R=%lld skip=%d", who, (long long)B,
                (long long)Sq, (long long)R, skip);
  DXA_CHECK_ARG(B <= (1 << 20) && Sq <= (1 << 24) && R + 1 + skip <= Sq && B * (R + 2) <= (1ll << 30),
                "%s: sizes out of range B=%lld Sq=%lld R=%lld (the block of skip + 1 + R rows must fit into Sq)", who, (long long)B,
                (long long)Sq, (long long)R);
  return DXA_OK;
}

}  // namespace

extern "C" int dxa_noisy_embed_fwd(const float* a, const void* w1, const void* b1, void* h, int64_t R, int64_t d, int dtype, int w_dtype,
                                   dxa_stream_t stream) {
  if (int rc = check_dtypes("dxa_noisy_embed_fwd", dtype, w_dtype)) return rc;
  DXA_CHECK_ARG(a && w1 && b1 && h, "dxa_noisy_embed_fwd: null a / w1 / b1 / h");
  DXA_CHECK_ARG(R >= 0 && R <= (1ll << 30), "dxa_noisy_embed_fwd: R = %lld outside [0, 2^30]", (long long)R);
  if (int rc = check_width("dxa_noisy_embed_fwd", d)) return rc;
  DXA_CHECK_ARG(al16(w1) && al16(b1) && al16(h), "dxa_noisy_embed_fwd: w1 / b1 / h must be 16-byte aligned");
  if (R == 0) return DXA_OK;
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((unsigned)R);
#define EMB(T_, TW_, V_) hipLaunchKernelGGL((noisy_embed_fwd_k<T_, TW_, V_>), grid, dim3(256), 0, st, a, (const TW_*)w1, (const TW_*)b1, (T_*)h, d)
  if (dtype == DXA_BF16 && w_dtype == DXA_BF16) EMB(bf16_t, bf16_t, 8);
  else if (dtype == DXA_BF16) EMB(bf16_t, float, 8);
  else EMB(float, float, 4);
#undef EMB
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}

extern "C" int dxa_noisy_embed_bwd_blocks(int64_t R) {
  if (R < 1) R = 1;
  return (int)((R + EMBED_CHUNK - 1) / EMBED_CHUNK);
}

extern "C" int dxa_noisy_embed_bwd(const void* dh, const float* a, const void* w1, const void* b1, float* dw1, float* db1, float* partial,
                                   int64_t R, int64_t d, int accumulate, int dtype, int w_dtype, dxa_stream_t stream) {
  if (int rc = check_dtypes("dxa_noisy_embed_bwd", dtype, w_dtype)) return rc;
  DXA_CHECK_ARG(dh && a && w1 && b1 && dw1 && db1 && partial, "dxa_noisy_embed_bwd: null dh / a / w1 / b1 / dw1 / db1 / partial");
  DXA_CHECK_ARG(R >= 1 && R <= (1ll << 19), "dxa_noisy_embed_bwd: R = %lld outside [1, 2^19] (the chunks run along grid y)", (long long)R);
  if (int rc = check_width("dxa_noisy_embed_bwd", d)) return rc;
  DXA_CHECK_ARG(al16(dh) && al16(w1) && al16(b1) && al16(dw1) && al16(db1) && al16(partial),
                "dxa_noisy_embed_bwd: dh / w1 / b1 / dw1 / db1 / partial must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int64_t chunks = dxa_noisy_embed_bwd_blocks(R);
  const int vec = dtype == DXA_BF16 ? 8 : 4;
  dim3 grid((unsigned)dxa_cdiv(d, 256 * vec), (unsigned)chunks);
#define EMBB(T_, TW_, V_) hipLaunchKernelGGL((noisy_embed_bwd_part_k<T_, TW_, V_>), grid, dim3(256), 0, st, (const T_*)dh, a, (const TW_*)w1, (const TW_*)b1, partial, R, d)
  if (dtype == DXA_BF16 && w_dtype == DXA_BF16) EMBB(bf16_t, bf16_t, 8);
  else if (dtype == DXA_BF16) EMBB(bf16_t, float, 8);
  else EMBB(float, float, 4);
#undef EMBB
  DXA_CHECK_LAUNCH();
  hipLaunchKernelGGL(noisy_embed_bwd_fold_k, dim3((unsigned)dxa_cdiv(2 * d, 1024)), dim3(256), 0, st, partial, dw1, db1, d, chunks, accumulate);
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}

extern "C" int dxa_diffusion_put_fwd(void* x, const void* proj, const void* time, const void* state, const int64_t* off, int64_t B,
                                     int64_t Sq, int64_t d, int64_t n_rows, int dtype, dxa_stream_t stream) {
  if (int rc = check_dtypes("dxa_diffusion_put_fwd", dtype, dtype)) return rc;
  DXA_CHECK_ARG(x && proj && time && off, "dxa_diffusion_put_fwd: null x / proj / time / off");
  const int skip = state ? 1 : 0;
  if (int rc = check_block("dxa_diffusion_put_fwd", B, Sq, n_rows, skip)) return rc;
  if (int rc = check_width("dxa_diffusion_put_fwd", d)) return rc;
  DXA_CHECK_ARG(al16(x) && al16(proj) && al16(time) && al16(state), "dxa_diffusion_put_fwd: x / proj / time / state must be 16-byte aligned");
  if (B == 0) return DXA_OK;
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((unsigned)(B * (n_rows + 1 + skip)));
#define DPUT(T_, V_) hipLaunchKernelGGL((diffusion_put_fwd_k<T_, V_>), grid, dim3(256), 0, st, (T_*)x, (const T_*)proj, (const T_*)time, (const T_*)state, off, Sq, d, n_rows, skip)
  if (dtype == DXA_BF16) DPUT(bf16_t, 8); else DPUT(float, 4);
#undef DPUT
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}

extern "C" int dxa_diffusion_put_bwd(const void* dx, const int64_t* off, void* dproj, void* dstate, int64_t B, int64_t Sq, int64_t d,
                                     int64_t n_rows, int skip, int dtype, dxa_stream_t stream) {
  if (int rc = check_dtypes("dxa_diffusion_put_bwd", dtype, dtype)) return rc;
  DXA_CHECK_ARG(dx && off && dproj, "dxa_diffusion_put_bwd: null dx / off / dproj");
  DXA_CHECK_ARG(!dstate || skip == 1, "dxa_diffusion_put_bwd: dstate without a state row (skip = 0)");
  if (int rc = check_block("dxa_diffusion_put_bwd", B, Sq, n_rows, skip)) return rc;
  if (int rc = check_width("dxa_diffusion_put_bwd", d)) return rc;
  DXA_CHECK_ARG(al16(dx) && al16(dproj) && al16(dstate), "dxa_diffusion_put_bwd: dx / dproj / dstate must be 16-byte aligned");
  if (B == 0) return DXA_OK;
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((unsigned)(B * n_rows + (dstate ? B : 0)));
#define DPUTB(T_, V_) hipLaunchKernelGGL((diffusion_put_bwd_k<T_, V_>), grid, dim3(256), 0, st, (const T_*)dx, off, (T_*)dproj, (T_*)dstate, B, Sq, d, n_rows, skip)
  if (dtype == DXA_BF16) DPUTB(bf16_t, 8); else DPUTB(float, 4);
#undef DPUTB
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}

extern "C" int dxa_ddim_step_embed(const void* eps, float* x, float c0, float c1, float c2, float c3, float clip, const void* time_row,
                                   const void* w1, const void* b1, void* suffix, void* h, int64_t n, int64_t d, int dtype, int w_dtype,
                                   dxa_stream_t stream) {
  if (int rc = check_dtypes("dxa_ddim_step_embed", dtype, w_dtype)) return rc;
  DXA_CHECK_ARG(x && time_row && w1 && b1 && suffix && h, "dxa_ddim_step_embed: null x / time_row / w1 / b1 / suffix / h");
  DXA_CHECK_ARG(n >= 1 && n <= (1 << 20), "dxa_ddim_step_embed: n = %lld outside [1, 2^20]", (long long)n);
  if (int rc = check_width("dxa_ddim_step_embed", d)) return rc;
  DXA_CHECK_ARG(al16(time_row) && al16(w1) && al16(b1) && al16(suffix) && al16(h),
                "dxa_ddim_step_embed: time_row / w1 / b1 / suffix / h must be 16-byte aligned");
  DXA_CHECK_ARG(clip == clip, "dxa_ddim_step_embed: clip is NaN (<= 0 switches the clamp off)");
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((unsigned)(n + 1));
#define STEP(T_, TW_, V_) hipLaunchKernelGGL((ddim_step_embed_k<T_, TW_, V_>), grid, dim3(256), 0, st, (const T_*)eps, x, c0, c1, c2, c3, clip, (const T_*)time_row, (const TW_*)w1, (const TW_*)b1, (T_*)suffix, (T_*)h, n, d)
  if (dtype == DXA_BF16 && w_dtype == DXA_BF16) STEP(bf16_t, bf16_t, 8);
  else if (dtype == DXA_BF16) STEP(bf16_t, float, 8);
  else STEP(float, float, 4);
#undef STEP
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}
