// OFT policy kernels (dexbotic/model/oft/oft_arch.py, oft/action_model/model.py): the learned action-query rows written into the
// spliced sequence at per-sample offsets, the LayerNorm of the MLP-ResNet head over the A*d wide rows read straight out of the decoder
// output at those offsets, and the L1 loss.  fp32 statistics, fixed summation orders, no atomics.
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

// ------------------------------------------------------------------------------------------------ action_put
// one workgroup per (sample, block row): row 0 of a block with `skip` is the sample's state row, the rest the shared query rows
// (`qstride` = d), or one shared row for all of them (action_fill: `qstride` = 0)
template <typename T, typename TQ, int VEC>
__global__ __launch_bounds__(256) void action_put_fwd_k(T* __restrict__ x, const TQ* __restrict__ query, const T* __restrict__ state,
                                                        const int64_t* __restrict__ off, int64_t Sq, int64_t d, int64_t nq, int skip,
                                                        int64_t qstride) {
  const int64_t Q = nq + skip;
  const int64_t b = blockIdx.x / Q, j = blockIdx.x - b * Q;
  const int64_t o = block_start(off, b, Q, Sq);
  if (o < 0) return;
  T* xr = x + ((b * Sq + o + j) * d);
  if (skip && j == 0) {
    const T* sr = state + b * d;
    for (int64_t c = (int64_t)threadIdx.x * VEC; c < d; c += 256 * VEC) {
      float v[VEC];
      ldv<T, VEC>(v, sr + c);
      stv<T, VEC>(xr + c, v);
    }
    return;
  }
  const TQ* qr = query + (j - skip) * qstride;
  for (int64_t c = (int64_t)threadIdx.x * VEC; c < d; c += 256 * VEC) {
    float v[VEC];
    ldv<TQ, VEC>(v, qr + c);
    stv<T, VEC>(xr + c, v);
  }
}

// workgroups [0, nq): dquery row j = sum over the samples in ascending order (fp32), replacing or added to what the slot holds;
// workgroups [nq, nq + B) (with dstate): the state row's gradient of sample b
template <typename T, int VEC>
__global__ __launch_bounds__(256) void action_put_bwd_k(const T* __restrict__ dx, const int64_t* __restrict__ off,
                                                        float* __restrict__ dquery, T* __restrict__ dstate, int64_t B, int64_t Sq,
                                                        int64_t d, int64_t nq, int skip, int accumulate) {
  const int64_t Q = nq + skip;
  if ((int64_t)blockIdx.x >= nq) {
    const int64_t b = (int64_t)blockIdx.x - nq;
    const int64_t o = block_start(off, b, Q, Sq);
    for (int64_t c = (int64_t)threadIdx.x * VEC; c < d; c += 256 * VEC) {
      float v[VEC];
      if (o >= 0) {
        ldv<T, VEC>(v, dx + ((b * Sq + o) * d + c));
      } else {
#pragma unroll
        for (int i = 0; i < VEC; ++i) v[i] = 0.f;
      }
      stv<T, VEC>(dstate + b * d + c, v);
    }
    return;
  }
  const int64_t j = blockIdx.x;
  for (int64_t c = (int64_t)threadIdx.x * VEC; c < d; c += 256 * VEC) {
    float s[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) s[i] = 0.f;
    for (int64_t b = 0; b < B; ++b) {
      const int64_t o = block_start(off, b, Q, Sq);
      if (o < 0) continue;
      float v[VEC];
      ldv<T, VEC>(v, dx + ((b * Sq + o + skip + j) * d + c));
#pragma unroll
      for (int i = 0; i < VEC; ++i) s[i] += v[i];
    }
    float* out = dquery + j * d + c;
    if (accumulate) {
      float old[VEC];
      ldv<float, VEC>(old, out);
#pragma unroll
      for (int i = 0; i < VEC; ++i) s[i] = old[i] + s[i];
    }
    stv<float, VEC>(out, s);
  }
}

// ------------------------------------------------------------------------------------------------ action_layernorm
// Row (b, t) of the head's input: the A*d contiguous elements from h[b, off[b] + skip + t*A, 0].
__device__ __forceinline__ int64_t action_row(const int64_t* __restrict__ off, int64_t row, int64_t T, int64_t A, int64_t Sq,
                                              int64_t d, int skip) {
  const int64_t b = row / T, t = row - b * T;
  const int64_t o = block_start(off, b, skip + T * A, Sq);
  return o < 0 ? -1 : (b * Sq + o + skip + t * A) * d;
}

// rows of up to 4096 columns: one wave per row, the loops and the summation order of layernorm_fwd_k (norm.hip), so that the result
// has the bits of dxa_layernorm_fwd on the gathered rows
template <typename T, typename TW, int VEC>
__global__ __launch_bounds__(256) void action_ln_fwd_wave_k(const T* __restrict__ h, const int64_t* __restrict__ off,
                                                            const TW* __restrict__ w, const TW* __restrict__ b, T* __restrict__ y,
                                                            float* __restrict__ mean_out, float* __restrict__ rstd_out, int64_t rows,
                                                            int64_t T_, int64_t A, int64_t Sq, int64_t d, int skip, float eps) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int64_t start = action_row(off, row, T_, A, Sq, d, skip);
  if (start < 0) return;
  const int64_t cols = A * d;
  const T* xr = h + start;
  float s = 0.f;
  for (int64_t c = (int64_t)lane * VEC; c < cols; c += 64 * VEC) {
    float v[VEC];
    Vec<T, VEC>::ld(v, xr + c);
#pragma unroll
    for (int i = 0; i < VEC; ++i) s += v[i];
  }
  const float mean = wave_sum(s) / (float)cols;
  float ss = 0.f;
  for (int64_t c = (int64_t)lane * VEC; c < cols; c += 64 * VEC) {
    float v[VEC];
    Vec<T, VEC>::ld(v, xr + c);
#pragma unroll
    for (int i = 0; i < VEC; ++i) { const float dv = v[i] - mean; ss += dv * dv; }
  }
  const float rstd = rsqrtf(wave_sum(ss) / (float)cols + eps);
  if (lane == 0) {
    if (mean_out) mean_out[row] = mean;
    if (rstd_out) rstd_out[row] = rstd;
  }
  T* yr = y + row * cols;
  for (int64_t c = (int64_t)lane * VEC; c < cols; c += 64 * VEC) {
    float v[VEC], g[VEC], bb[VEC];
    Vec<T, VEC>::ld(v, xr + c);
    if (w) Vec<TW, VEC>::ld(g, w + c);
    if (b) Vec<TW, VEC>::ld(bb, b + c);
#pragma unroll
    for (int i = 0; i < VEC; ++i) v[i] = (v[i] - mean) * rstd * (w ? g[i] : 1.f) + (b ? bb[i] : 0.f);
    Vec<T, VEC>::st(yr + c, v);
  }
}

// wider rows: a workgroup of 256 threads per row, thread t owns the chunks k*256 + t of VEC elements.  NCH > 0: the row (up to
// NCH * 256 * VEC columns) is read ONCE and stays in registers between the two statistics passes and the write; NCH = 0: rows wider
// than that, and the scalar path, read the row again for each pass.  Mean first, then the sum of squared distances from it.
template <typename T, typename TW, int VEC, int NCH>
__global__ __launch_bounds__(256) void action_ln_fwd_wg_k(const T* __restrict__ h, const int64_t* __restrict__ off,
                                                          const TW* __restrict__ w, const TW* __restrict__ b, T* __restrict__ y,
                                                          float* __restrict__ mean_out, float* __restrict__ rstd_out, int64_t T_,
                                                          int64_t A, int64_t Sq, int64_t d, int skip, float eps) {
  __shared__ float red[16];
  const int64_t row = blockIdx.x;
  const int64_t start = action_row(off, row, T_, A, Sq, d, skip);
  if (start < 0) return;
  const int64_t cols = A * d;
  const T* xr = h + start;
  T* yr = y + row * cols;
  constexpr int NR = NCH > 0 ? NCH : 1;
  float v[NR][VEC];
  float s = 0.f;
  if constexpr (NCH > 0) {
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const int64_t c = ((int64_t)k * 256 + threadIdx.x) * VEC;
      if (c < cols) {
        ldv<T, VEC>(v[k], xr + c);
      } else {
#pragma unroll
        for (int i = 0; i < VEC; ++i) v[k][i] = 0.f;
      }
    }
#pragma unroll
    for (int k = 0; k < NCH; ++k)
#pragma unroll
      for (int i = 0; i < VEC; ++i) s += v[k][i];
  } else {
    for (int64_t c = (int64_t)threadIdx.x * VEC; c < cols; c += 256 * VEC) {
      ldv<T, VEC>(v[0], xr + c);
#pragma unroll
      for (int i = 0; i < VEC; ++i) s += v[0][i];
    }
  }
  const float mean = block_sum(s, red) / (float)cols;
  float ss = 0.f;
  if constexpr (NCH > 0) {
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const int64_t c = ((int64_t)k * 256 + threadIdx.x) * VEC;
      if (c < cols) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) { const float dv = v[k][i] - mean; ss += dv * dv; }
      }
    }
  } else {
    for (int64_t c = (int64_t)threadIdx.x * VEC; c < cols; c += 256 * VEC) {
      ldv<T, VEC>(v[0], xr + c);
#pragma unroll
      for (int i = 0; i < VEC; ++i) { const float dv = v[0][i] - mean; ss += dv * dv; }
    }
  }
  const float rstd = rsqrtf(block_sum(ss, red) / (float)cols + eps);
  if (threadIdx.x == 0) {
    if (mean_out) mean_out[row] = mean;
    if (rstd_out) rstd_out[row] = rstd;
  }
  if constexpr (NCH > 0) {
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const int64_t c = ((int64_t)k * 256 + threadIdx.x) * VEC;
      if (c < cols) {
        float g[VEC], bb[VEC], o[VEC];
        if (w) ldv<TW, VEC>(g, w + c);
        if (b) ldv<TW, VEC>(bb, b + c);
#pragma unroll
        for (int i = 0; i < VEC; ++i) o[i] = (v[k][i] - mean) * rstd * (w ? g[i] : 1.f) + (b ? bb[i] : 0.f);
        stv<T, VEC>(yr + c, o);
      }
    }
  } else {
    for (int64_t c = (int64_t)threadIdx.x * VEC; c < cols; c += 256 * VEC) {
      float g[VEC], bb[VEC], o[VEC];
      ldv<T, VEC>(v[0], xr + c);
      if (w) ldv<TW, VEC>(g, w + c);
      if (b) ldv<TW, VEC>(bb, b + c);
#pragma unroll
      for (int i = 0; i < VEC; ++i) o[i] = (v[0][i] - mean) * rstd * (w ? g[i] : 1.f) + (b ? bb[i] : 0.f);
      stv<T, VEC>(yr + c, o);
    }
  }
}

// Backward.  Workgroup g takes the rows g, g + gridDim.x, ... in that order; thread t owns the same columns in every row, so its
// share of dw | db is a private running sum: in registers (NCH > 0, rows of up to NCH * 256 * VEC columns) or in the workgroup's
// slab of `partial` (NCH = 0), written / left there as [gridDim.x, 2 * cols] for dxa_colsum.  Per row: one pass over dy, x, w for the
// two row sums (and the dw | db terms), a workgroup reduction, a second pass (the row is L2 resident) that writes dx into dh.
// Afterwards the workgroups zero every row of dh that is no action row: dh leaves the launch completely written.
template <typename T, typename TW, int VEC, int NCH>
__global__ __launch_bounds__(256) void action_ln_bwd_k(const T* __restrict__ dy, const T* __restrict__ h,
                                                       const int64_t* __restrict__ off, const TW* __restrict__ w,
                                                       const float* __restrict__ mean, const float* __restrict__ rstd,
                                                       T* __restrict__ dh, float* __restrict__ partial, int64_t B, int64_t T_,
                                                       int64_t A, int64_t Sq, int64_t d, int skip) {
  __shared__ float red[16];
  const int64_t cols = A * d, rows = B * T_;
  constexpr int NR = NCH > 0 ? NCH : 1;
  float aw[NR][VEC], ab[NR][VEC];
  float* slab = partial ? partial + (int64_t)blockIdx.x * 2 * cols : nullptr;
  if constexpr (NCH > 0) {
#pragma unroll
    for (int k = 0; k < NCH; ++k)
#pragma unroll
      for (int i = 0; i < VEC; ++i) aw[k][i] = ab[k][i] = 0.f;
  } else if (slab) {
    for (int64_t c = (int64_t)threadIdx.x * VEC; c < cols; c += 256 * VEC)
#pragma unroll
      for (int i = 0; i < VEC; ++i) slab[c + i] = slab[cols + c + i] = 0.f;       // the columns this thread alone ever touches
  }
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const int64_t start = action_row(off, row, T_, A, Sq, d, skip);
    if (start < 0) continue;                                 // (uniform over the workgroup)
    const float mu = mean[row], rs = rstd[row];
    const T* xr = h + start;
    const T* gr = dy + row * cols;
    float s1 = 0.f, s2 = 0.f;
    auto pass1 = [&](int64_t c, float (&paw)[VEC], float (&pab)[VEC]) {
      float xv[VEC], gv[VEC], wv[VEC];
      ldv<T, VEC>(xv, xr + c);
      ldv<T, VEC>(gv, gr + c);
      if (w) ldv<TW, VEC>(wv, w + c);
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        const float xh = (xv[i] - mu) * rs;
        const float g = gv[i] * (w ? wv[i] : 1.f);
        s1 += g;
        s2 += g * xh;
        paw[i] += gv[i] * xh;
        pab[i] += gv[i];
      }
    };
    if constexpr (NCH > 0) {
#pragma unroll
      for (int k = 0; k < NCH; ++k) {
        const int64_t c = ((int64_t)k * 256 + threadIdx.x) * VEC;
        if (c < cols) pass1(c, aw[k], ab[k]);
      }
    } else {
      for (int64_t c = (int64_t)threadIdx.x * VEC; c < cols; c += 256 * VEC) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) { aw[0][i] = slab ? slab[c + i] : 0.f; ab[0][i] = slab ? slab[cols + c + i] : 0.f; }
        pass1(c, aw[0], ab[0]);
        if (slab) {
#pragma unroll
          for (int i = 0; i < VEC; ++i) { slab[c + i] = aw[0][i]; slab[cols + c + i] = ab[0][i]; }
        }
      }
    }
    const float c1 = block_sum(s1, red) / (float)cols;
    const float c2 = block_sum(s2, red) / (float)cols;
    T* dxr = dh + start;
    for (int64_t c = (int64_t)threadIdx.x * VEC; c < cols; c += 256 * VEC) {
      float xv[VEC], gv[VEC], wv[VEC], o[VEC];
      ldv<T, VEC>(xv, xr + c);
      ldv<T, VEC>(gv, gr + c);
      if (w) ldv<TW, VEC>(wv, w + c);
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        const float g = gv[i] * (w ? wv[i] : 1.f);
        o[i] = rs * (g - c1 - (xv[i] - mu) * rs * c2);
      }
      stv<T, VEC>(dxr + c, o);
    }
  }
  if constexpr (NCH > 0) {
    if (slab) {
#pragma unroll
      for (int k = 0; k < NCH; ++k) {
        const int64_t c = ((int64_t)k * 256 + threadIdx.x) * VEC;
        if (c < cols) {
          stv<float, VEC>(slab + c, aw[k]);
          stv<float, VEC>(slab + cols + c, ab[k]);
        }
      }
    }
  }
  // every other row of dh: zero
  float z[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) z[i] = 0.f;
  const int64_t n_act = T_ * A;
  for (int64_t r = blockIdx.x; r < B * Sq; r += gridDim.x) {
    const int64_t b = r / Sq, p = r - b * Sq;
    const int64_t o = block_start(off, b, skip + n_act, Sq);
    if (o >= 0 && p >= o + skip && p < o + skip + n_act) continue;
    T* zr = dh + r * d;
    for (int64_t c = (int64_t)threadIdx.x * VEC; c < d; c += 256 * VEC) stv<T, VEC>(zr + c, z);
  }
}

constexpr int64_t ACTION_LN_WAVE_MAX_COLS = 4096;      // one wave per row up to here (the order of dxa_layernorm_fwd)
constexpr int ACTION_LN_REG_CHUNKS_16B = 13;           // 13 chunks x 256 threads x 8 bf16 = 26624 columns in registers (7 x 3584 = 25088)
constexpr int64_t ACTION_LN_REG_MAX_COLS = 26624;      // fp32: 26 chunks of 4
constexpr int ACTION_LN_BWD_MAX_BLOCKS = 64;

int check_action_dtypes(const char* who, int dtype, int w_dtype) {
  if (!(dtype == DXA_F32 || dtype == DXA_BF16) || !(w_dtype == DXA_F32 || w_dtype == DXA_BF16) ||
      (dtype == DXA_F32 && w_dtype == DXA_BF16)) {
    dxa_set_error("%s: unsupported dtype combination (%d,%d)", who, dtype, w_dtype);
    return DXA_ERR_UNSUPPORTED;
  }
  return DXA_OK;
}

int check_action_sizes(const char* who, int64_t B, int64_t Sq, int64_t d, int64_t T, int64_t A, int skip) {
  DXA_CHECK_ARG(B >= 0 && Sq > 0 && d > 0 && T > 0 && A > 0 && (skip == 0 || skip == 1), "%s: bad sizes B=%lld Sq=%lld d=%lld T=%lld A=%lld skip=%d",
                who, (long long)B, (long long)Sq, (long long)d, (long long)T, (long long)A, skip);
  DXA_CHECK_ARG(B <= (1 << 20) && Sq <= (1 << 24) && d <= (1 << 20) && T * A + skip <= Sq && A * d <= (1ll << 24) && B * T <= (1ll << 30),
                "%s: sizes out of range B=%lld Sq=%lld d=%lld T=%lld A=%lld (the block of T*A + skip rows must fit into Sq)", who,
                (long long)B, (long long)Sq, (long long)d, (long long)T, (long long)A);
  return DXA_OK;
}

}  // namespace

extern "C" int dxa_action_put_fwd(void* x, const void* query, const void* state, const int64_t* off, int64_t B, int64_t Sq, int64_t d,
                                  int64_t n_query, int dtype, int q_dtype, dxa_stream_t stream) {
  if (int rc = check_action_dtypes("dxa_action_put_fwd", dtype, q_dtype == DXA_F32 ? DXA_F32 : dtype)) return rc;
  DXA_CHECK_ARG(q_dtype == DXA_F32 || q_dtype == dtype, "dxa_action_put_fwd: the query is fp32 or in the dtype of x (%d,%d)", dtype, q_dtype);
  DXA_CHECK_ARG(x && query && off, "dxa_action_put_fwd: null x / query / off");
  const int skip = state ? 1 : 0;
  if (int rc = check_action_sizes("dxa_action_put_fwd", B, Sq, d, n_query, 1, skip)) return rc;
  if (B == 0) return DXA_OK;
  hipStream_t st = (hipStream_t)stream;
  const int vec = dtype == DXA_BF16 ? 8 : 4;
  const bool vec_ok = al16(x) && al16(query) && (!state || al16(state)) && d % vec == 0;
  dim3 grid((unsigned)(B * (n_query + skip)));
#define PUT(T_, TQ_, V_) hipLaunchKernelGGL((action_put_fwd_k<T_, TQ_, V_>), grid, dim3(256), 0, st, (T_*)x, (const TQ_*)query, (const T_*)state, off, Sq, d, n_query, skip, d)
  if (dtype == DXA_BF16 && q_dtype == DXA_BF16) { if (vec_ok) PUT(bf16_t, bf16_t, 8); else PUT(bf16_t, bf16_t, 1); }
  else if (dtype == DXA_BF16) { if (vec_ok) PUT(bf16_t, float, 8); else PUT(bf16_t, float, 1); }
  else { if (vec_ok) PUT(float, float, 4); else PUT(float, float, 1); }
#undef PUT
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}

extern "C" int dxa_action_put_bwd(const void* dx, const int64_t* off, float* dquery, void* dstate, int64_t B, int64_t Sq, int64_t d,
                                  int64_t n_query, int skip, int accumulate, int dtype, dxa_stream_t stream) {
  if (int rc = check_action_dtypes("dxa_action_put_bwd", dtype, dtype)) return rc;
  DXA_CHECK_ARG(dx && off && dquery, "dxa_action_put_bwd: null dx / off / dquery");
  DXA_CHECK_ARG(!dstate || skip == 1, "dxa_action_put_bwd: dstate without a state row (skip = 0)");
  if (int rc = check_action_sizes("dxa_action_put_bwd", B, Sq, d, n_query, 1, skip)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int vec = dtype == DXA_BF16 ? 8 : 4;
  const bool vec_ok = al16(dx) && al16(dquery) && (!dstate || al16(dstate)) && d % vec == 0;
  dim3 grid((unsigned)(n_query + (dstate ? B : 0)));
#define PUTB(T_, V_) hipLaunchKernelGGL((action_put_bwd_k<T_, V_>), grid, dim3(256), 0, st, (const T_*)dx, off, dquery, (T_*)dstate, B, Sq, d, n_query, skip, accumulate)
  if (dtype == DXA_BF16) { if (vec_ok) PUTB(bf16_t, 8); else PUTB(bf16_t, 1); }
  else { if (vec_ok) PUTB(float, 4); else PUTB(float, 1); }
#undef PUTB
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}

extern "C" int dxa_action_layernorm_fwd(const void* h, const int64_t* off, const void* w, const void* b, void* y, float* mean,
                                        float* rstd, int64_t B, int64_t Sq, int64_t d, int64_t T, int64_t A, int skip, float eps,
                                        int dtype, int w_dtype, dxa_stream_t stream) {
  if (int rc = check_action_dtypes("dxa_action_layernorm_fwd", dtype, w_dtype)) return rc;
  DXA_CHECK_ARG(h && off && y, "dxa_action_layernorm_fwd: null h / off / y");
  if (int rc = check_action_sizes("dxa_action_layernorm_fwd", B, Sq, d, T, A, skip)) return rc;
  const int64_t rows = B * T, cols = A * d;
  if (rows == 0) return DXA_OK;
  hipStream_t st = (hipStream_t)stream;
  const bool al = al16(h) && al16(y) && (!w || al16(w)) && (!b || al16(b));
  if (cols <= ACTION_LN_WAVE_MAX_COLS) {
    const bool v4 = al && d % 4 == 0;          // every row then starts on a multiple of 4 elements
    dim3 grid((unsigned)((rows + 3) / 4));
#define LNW(T_, TW_, V_) hipLaunchKernelGGL((action_ln_fwd_wave_k<T_, TW_, V_>), grid, dim3(256), 0, st, (const T_*)h, off, (const TW_*)w, (const TW_*)b, (T_*)y, mean, rstd, rows, T, A, Sq, d, skip, eps)
    if (dtype == DXA_BF16 && w_dtype == DXA_BF16) { if (v4) LNW(bf16_t, bf16_t, 4); else LNW(bf16_t, bf16_t, 1); }
    else if (dtype == DXA_BF16) { if (v4) LNW(bf16_t, float, 4); else LNW(bf16_t, float, 1); }
    else { if (v4) LNW(float, float, 4); else LNW(float, float, 1); }
#undef LNW
  } else {
    const int vec = dtype == DXA_BF16 ? 8 : 4;
    const bool vec_ok = al && d % vec == 0;
    const bool regs = vec_ok && cols <= ACTION_LN_REG_MAX_COLS;
    dim3 grid((unsigned)rows);
#define LNG(T_, TW_, V_, N_) hipLaunchKernelGGL((action_ln_fwd_wg_k<T_, TW_, V_, N_>), grid, dim3(256), 0, st, (const T_*)h, off, (const TW_*)w, (const TW_*)b, (T_*)y, mean, rstd, T, A, Sq, d, skip, eps)
    if (dtype == DXA_BF16 && w_dtype == DXA_BF16) {
      if (regs) LNG(bf16_t, bf16_t, 8, ACTION_LN_REG_CHUNKS_16B); else if (vec_ok) LNG(bf16_t, bf16_t, 8, 0); else LNG(bf16_t, bf16_t, 1, 0);
    } else if (dtype == DXA_BF16) {
      if (regs) LNG(bf16_t, float, 8, ACTION_LN_REG_CHUNKS_16B); else if (vec_ok) LNG(bf16_t, float, 8, 0); else LNG(bf16_t, float, 1, 0);
    } else {
      if (regs) LNG(float, float, 4, 2 * ACTION_LN_REG_CHUNKS_16B); else if (vec_ok) LNG(float, float, 4, 0); else LNG(float, float, 1, 0);
    }
#undef LNG
  }
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}

extern "C" int dxa_action_layernorm_bwd_blocks(int64_t rows) {
  if (rows < 1) rows = 1;
  return (int)(rows < ACTION_LN_BWD_MAX_BLOCKS ? rows : ACTION_LN_BWD_MAX_BLOCKS);
}

extern "C" int dxa_action_layernorm_bwd(const void* dy, const void* h, const int64_t* off, const void* w, const float* mean,
                                        const float* rstd, void* dh, float* partial_dwdb, int64_t B, int64_t Sq, int64_t d, int64_t T,
                                        int64_t A, int skip, int dtype, int w_dtype, dxa_stream_t stream) {
  if (int rc = check_action_dtypes("dxa_action_layernorm_bwd", dtype, w_dtype)) return rc;
  DXA_CHECK_ARG(dy && h && off && mean && rstd && dh, "dxa_action_layernorm_bwd: null dy / h / off / mean / rstd / dh");
  DXA_CHECK_ARG(!w || partial_dwdb, "dxa_action_layernorm_bwd: partial_dwdb required when w is given");
  if (int rc = check_action_sizes("dxa_action_layernorm_bwd", B, Sq, d, T, A, skip)) return rc;
  const int64_t rows = B * T, cols = A * d;
  if (rows == 0) return DXA_OK;
  hipStream_t st = (hipStream_t)stream;
  float* part = w ? partial_dwdb : nullptr;
  const int vec = dtype == DXA_BF16 ? 8 : 4;
  const bool vec_ok = al16(h) && al16(dy) && al16(dh) && (!w || al16(w)) && (!part || al16(part)) && d % vec == 0;
  dim3 grid((unsigned)dxa_action_layernorm_bwd_blocks(rows));
#define LNB(T_, TW_, V_, N_) hipLaunchKernelGGL((action_ln_bwd_k<T_, TW_, V_, N_>), grid, dim3(256), 0, st, (const T_*)dy, (const T_*)h, off, (const TW_*)w, mean, rstd, (T_*)dh, part, B, T, A, Sq, d, skip)
#define LNB_PICK(T_, TW_, V_)                                                                            \
  do {                                                                                                   \
    if (!vec_ok) LNB(T_, TW_, 1, 0);                                                                     \
    else if (cols <= ACTION_LN_WAVE_MAX_COLS) LNB(T_, TW_, V_, 16 / V_);                                 \
    else if (cols <= ACTION_LN_REG_MAX_COLS) LNB(T_, TW_, V_, ACTION_LN_REG_CHUNKS_16B * 8 / V_);        \
    else LNB(T_, TW_, V_, 0);                                                                            \
  } while (0)
  if (dtype == DXA_BF16 && w_dtype == DXA_BF16) LNB_PICK(bf16_t, bf16_t, 8);
  else if (dtype == DXA_BF16) LNB_PICK(bf16_t, float, 8);
  else LNB_PICK(float, float, 4);
#undef LNB_PICK
#undef LNB
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}

// ------------------------------------------------------------------------------------------------ L1 loss
namespace {
__global__ __launch_bounds__(1024) void l1_loss_k(const float* __restrict__ pred, const float* __restrict__ target,
                                                  float* __restrict__ loss, float* __restrict__ dpred, int64_t n, float gscale) {
  __shared__ float red[16];
  float s = 0.f;
  const float k = gscale / (float)n;
  for (int64_t i = threadIdx.x; i < n; i += 1024) {
    const float dv = pred[i] - target[i];
    s += fabsf(dv);
    if (dpred) dpred[i] = dv > 0.f ? k : (dv < 0.f ? -k : 0.f);
  }
  const float tot = block_sum(s, red);
  if (threadIdx.x == 0) loss[0] = tot / (float)n;
}
}  // namespace

extern "C" int dxa_l1_loss(const float* pred, const float* target, float* loss, float* dpred, int64_t n, float gscale,
                           dxa_stream_t stream) {
  DXA_CHECK_ARG(pred && target && loss && n > 0, "dxa_l1_loss: bad args (null pred / target / loss, or n <= 0)");
  hipLaunchKernelGGL(l1_loss_k, dim3(1), dim3(1024), 0, (hipStream_t)stream, pred, target, loss, dpred, n, gscale);
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}

// ================================================================================================ OFT-discrete
// (dexbotic/model/oft/oft_discrete_arch.py): the action rows as the dense operand of the lm_head product, the shared embedding row
// written into the reserved rows, and the inference head over the last num_bins - 1 rows of lm_head.weight.
namespace {

// ------------------------------------------------------------------------------------------------ action_rows
// one workgroup per action row: y[b*R + j] = h[b, off[b] + skip + j], zeros for a sample whose block is out of range
template <typename T, int VEC>
__global__ __launch_bounds__(256) void action_rows_fwd_k(const T* __restrict__ h, const int64_t* __restrict__ off, T* __restrict__ y,
                                                         int64_t Sq, int64_t d, int64_t R, int skip) {
  const int64_t b = blockIdx.x / R, j = blockIdx.x - b * R;
  const int64_t o = block_start(off, b, R + skip, Sq);
  const T* hr = h + ((b * Sq + (o < 0 ? 0 : o + skip + j)) * d);
  T* yr = y + (int64_t)blockIdx.x * d;
  for (int64_t c = (int64_t)threadIdx.x * VEC; c < d; c += 256 * VEC) {
    float v[VEC];
    if (o >= 0) {
      ldv<T, VEC>(v, hr + c);
    } else {
#pragma unroll
      for (int i = 0; i < VEC; ++i) v[i] = 0.f;
    }
    stv<T, VEC>(yr + c, v);
  }
}

// every row of dh, the workgroups striding over them: the dy row on an action row, zero elsewhere
template <typename T, int VEC>
__global__ __launch_bounds__(256) void action_rows_bwd_k(const T* __restrict__ dy, const int64_t* __restrict__ off, T* __restrict__ dh,
                                                         int64_t B, int64_t Sq, int64_t d, int64_t R, int skip) {
  for (int64_t r = blockIdx.x; r < B * Sq; r += gridDim.x) {
    const int64_t b = r / Sq, p = r - b * Sq;
    const int64_t o = block_start(off, b, R + skip, Sq);
    const bool act = o >= 0 && p >= o + skip && p < o + skip + R;          // (uniform over the workgroup)
    const T* src = dy + (act ? (b * R + (p - o - skip)) * d : 0);
    T* dst = dh + r * d;
    for (int64_t c = (int64_t)threadIdx.x * VEC; c < d; c += 256 * VEC) {
      float v[VEC];
      if (act) {
        ldv<T, VEC>(v, src + c);
      } else {
#pragma unroll
        for (int i = 0; i < VEC; ++i) v[i] = 0.f;
      }
      stv<T, VEC>(dst + c, v);
    }
  }
}

// ------------------------------------------------------------------------------------------------ action_fill (backward)
constexpr int FILL_CHUNK = 16;      // action rows summed by one workgroup of the first stage

// stage 1, grid (column blocks, chunks [+ B]): workgroup (x, g < chunks) sums the dx rows of the action rows g*16 ... g*16 + 15
// (numbered b*R + j, ascending; the rows of an out-of-range sample contribute nothing) into partial[g, its columns];
// workgroup (x, chunks + b): the state row's gradient of sample b
template <typename T, int VEC>
__global__ __launch_bounds__(256) void action_fill_bwd_part_k(const T* __restrict__ dx, const int64_t* __restrict__ off,
                                                              float* __restrict__ partial, T* __restrict__ dstate, int64_t B,
                                                              int64_t Sq, int64_t d, int64_t R, int skip, int64_t chunks) {
  const int64_t c = ((int64_t)blockIdx.x * 256 + threadIdx.x) * VEC;
  if (c >= d) return;
  const int64_t g = blockIdx.y;
  if (g >= chunks) {
    const int64_t b = g - chunks;
    const int64_t o = block_start(off, b, R + skip, Sq);
    float v[VEC];
    if (o >= 0) {
      ldv<T, VEC>(v, dx + ((b * Sq + o) * d + c));
    } else {
#pragma unroll
      for (int i = 0; i < VEC; ++i) v[i] = 0.f;
    }
    stv<T, VEC>(dstate + b * d + c, v);
    return;
  }
  float s[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) s[i] = 0.f;
  const int64_t r1 = (g + 1) * FILL_CHUNK < B * R ? (g + 1) * FILL_CHUNK : B * R;
  for (int64_t r = g * FILL_CHUNK; r < r1; ++r) {
    const int64_t b = r / R, j = r - b * R;
    const int64_t o = block_start(off, b, R + skip, Sq);
    if (o < 0) continue;
    float v[VEC];
    ldv<T, VEC>(v, dx + ((b * Sq + o + skip + j) * d + c));
#pragma unroll
    for (int i = 0; i < VEC; ++i) s[i] += v[i];
  }
  stv<float, VEC>(partial + g * d + c, s);
}

// stage 2: drow (+)= the chunks' partial rows in ascending order
template <int VEC>
__global__ __launch_bounds__(256) void action_fill_bwd_fold_k(const float* __restrict__ partial, float* __restrict__ drow, int64_t d,
                                                              int64_t chunks, int accumulate) {
  const int64_t c = ((int64_t)blockIdx.x * 256 + threadIdx.x) * VEC;
  if (c >= d) return;
  float s[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) s[i] = 0.f;
  for (int64_t g = 0; g < chunks; ++g) {
    float v[VEC];
    ldv<float, VEC>(v, partial + g * d + c);
#pragma unroll
    for (int i = 0; i < VEC; ++i) s[i] += v[i];
  }
  if (accumulate) {
    float old[VEC];
    ldv<float, VEC>(old, drow + c);
#pragma unroll
    for (int i = 0; i < VEC; ++i) s[i] = old[i] + s[i];
  }
  stv<float, VEC>(drow + c, s);
}

// ------------------------------------------------------------------------------------------------ action_bins
// Workgroup (row group rg, bin group bg) computes TM x TM tiles of 16 x 16: logits[(rg*TM + m)*16 .., (bg*TM + n)*16 ..] = H W^T with
// MFMA fragments loaded straight from global memory (no operand is shared between the waves: an LDS stage would be a round trip for
// nothing): lane (r = lane & 15, q = lane >> 4) holds k-group q of action row r of each row tile (A) and of bin row r of each bin
// tile (B).  bf16: 8 consecutive k per lane, one v_mfma_f32_16x16x32_bf16 per 32 k.  fp32: 4 consecutive k per lane, element i of
// both operands goes to the i-th of four v_mfma_f32_16x16x4_f32 (the k order inside a step is permuted the same way on both sides).
// The 4 waves take the k-steps w, w + 4, ... in ascending order; their partial tiles are added in the order ((0 + 1) + 2) + 3
// through LDS, rounded once and stored: an element's bits do not depend on TM.  TM = 1 spreads a single request's 112 rows over
// 7 x 16 workgroups; TM = 2 halves the operand bytes each workgroup pulls through its L1 per output, for the large batches.
// The bin groups of one row group then meet at a counter (agent-scope release by every workgroup, acquire by the one that draws
// the last ticket, which nobody waits for): that workgroup reads the finished logit rows back and writes bin and action.
template <typename T, int TM>
__global__ __launch_bounds__(256) void action_bins_k(const T* __restrict__ h, const int64_t* __restrict__ off, const T* __restrict__ w,
                                                     T* __restrict__ logits, int64_t* __restrict__ bin, float* __restrict__ action,
                                                     int* __restrict__ cnt, int64_t rows, int64_t Sq, int64_t d, int64_t R, int skip,
                                                     int NB, int nbg) {
  constexpr int KL = sizeof(T) == 2 ? 8 : 4;        // k per lane and step
  constexpr int KS = 4 * KL;                        // k per step
  constexpr int NT = TM * TM;                       // tiles per workgroup
  constexpr int FLAG = 4 * NT * 16 * 17;
  __shared__ float red[FLAG + 1];                   // per wave NT partial tiles of 16 x 16 (rows padded to 17), and the "last ticket" word
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int lr = lane & 15, lq = lane >> 4;
  const int64_t rg = blockIdx.x / nbg;
  const int bg = (int)(blockIdx.x - rg * nbg);
  // operand rows of this lane; a lane without one reads row 0 (always there) and its values are replaced by zeros
  const T* hp[TM];
  const T* wp[TM];
  bool a_ok[TM], b_ok[TM];
#pragma unroll
  for (int m = 0; m < TM; ++m) {
    const int64_t arow = (rg * TM + m) * 16 + lr;
    a_ok[m] = arow < rows;
    hp[m] = h;
    if (a_ok[m]) {
      const int64_t b = arow / R, j = arow - b * R;
      const int64_t o = block_start(off, b, R + skip, Sq);
      a_ok[m] = o >= 0;
      if (a_ok[m]) hp[m] = h + (b * Sq + o + skip + j) * d;
    }
    const int n_l = (bg * TM + m) * 16 + lr;
    b_ok[m] = n_l < NB;
    wp[m] = w + (b_ok[m] ? (int64_t)n_l * d : 0);
  }
  f32x4_t acc[TM][TM];
#pragma unroll
  for (int m = 0; m < TM; ++m)
#pragma unroll
    for (int n = 0; n < TM; ++n) acc[m][n] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  const uint4 z4 = make_uint4(0, 0, 0, 0);
  // 16 bytes of each operand at element k of the lane's rows (`ok` false: k is past the row, nothing is read there)
  auto load = [&](int64_t k, bool ok, uint4 (&a)[TM], uint4 (&bb)[TM]) {
#pragma unroll
    for (int m = 0; m < TM; ++m) {
      a[m] = *reinterpret_cast<const uint4*>(hp[m] + (ok ? k : 0));
      bb[m] = *reinterpret_cast<const uint4*>(wp[m] + (ok ? k : 0));
      if (!(a_ok[m] && ok)) a[m] = z4;
      if (!(b_ok[m] && ok)) bb[m] = z4;
    }
  };
  auto mma = [&](const uint4 (&a)[TM], const uint4 (&bb)[TM]) {
#pragma unroll
    for (int m = 0; m < TM; ++m)
#pragma unroll
      for (int n = 0; n < TM; ++n) {
        if constexpr (sizeof(T) == 2) {
          acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a[m]), __builtin_bit_cast(bf16x8_t, bb[n]),
                                                              acc[m][n], 0, 0, 0);
        } else {
          acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a[m].x), __uint_as_float(bb[n].x), acc[m][n], 0, 0, 0);
          acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a[m].y), __uint_as_float(bb[n].y), acc[m][n], 0, 0, 0);
          acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a[m].z), __uint_as_float(bb[n].z), acc[m][n], 0, 0, 0);
          acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a[m].w), __uint_as_float(bb[n].w), acc[m][n], 0, 0, 0);
        }
      }
  };
  const int64_t d_full = d / KS * KS;
  int64_t k0 = (int64_t)wv * KS;
  constexpr int U = 4;                              // steps whose loads are issued together
  for (; k0 + (U - 1) * 4 * KS < d_full; k0 += U * 4 * KS) {
    uint4 a[U][TM], bb[U][TM];
#pragma unroll
    for (int u = 0; u < U; ++u) load(k0 + u * 4 * KS + lq * KL, true, a[u], bb[u]);
#pragma unroll
    for (int u = 0; u < U; ++u) mma(a[u], bb[u]);
  }
  for (; k0 < d_full; k0 += 4 * KS) {
    uint4 a[TM], bb[TM];
    load(k0 + lq * KL, true, a, bb);
    mma(a, bb);
  }
  if (k0 < d) {                                     // the tail step (d % KL == 0: a lane's group lies inside the row or outside)
    uint4 a[TM], bb[TM];
    load(k0 + lq * KL, k0 + lq * KL < d, a, bb);
    mma(a, bb);
  }
  // C/D fragment: column (bin) = lane & 15, row (action row) = 4 * (lane >> 4) + i
#pragma unroll
  for (int m = 0; m < TM; ++m)
#pragma unroll
    for (int n = 0; n < TM; ++n)
#pragma unroll
      for (int i = 0; i < 4; ++i) red[((wv * NT + m * TM + n) * 16 + 4 * lq + i) * 17 + lr] = acc[m][n][i];
  __syncthreads();
#pragma unroll
  for (int m = 0; m < TM; ++m)
#pragma unroll
    for (int n = 0; n < TM; ++n) {
      const int row = tid >> 4, col = tid & 15;
      const int e = ((m * TM + n) * 16 + row) * 17 + col;
      const float s = ((red[e] + red[NT * 272 + e]) + red[2 * NT * 272 + e]) + red[3 * NT * 272 + e];
      const int64_t r = (rg * TM + m) * 16 + row;
      const int nn = (bg * TM + n) * 16 + col;
      if (r < rows && nn < NB) stf<T>(logits + r * NB + nn, s);
    }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int ticket = __hip_atomic_fetch_add(cnt + rg, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool last = ticket == nbg - 1;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    red[FLAG] = last ? 1.f : 0.f;
  }
  __syncthreads();
  if (red[FLAG] == 0.f) return;
  // the first index of the row's maximum (a NaN counts as the maximum, as in torch.argmax): 16 lanes per row
  auto better = [](float v, int i, float bv, int bj) {
    const bool vn = v != v, bn = bv != bv;
    const bool gt = (vn && !bn) || (!vn && !bn && v > bv);
    const bool eq = (vn && bn) || v == bv;
    return gt || (eq && i < bj);
  };
#pragma unroll
  for (int m = 0; m < TM; ++m) {
    const int64_t r = (rg * TM + m) * 16 + (tid >> 4);
    float best = -INFINITY;
    int bi = 0x7fffffff;
    if (r < rows) {
      for (int n = tid & 15; n < NB; n += 16) {
        const float v = ldf<T>(logits + r * NB + n);
        if (better(v, n, best, bi)) { best = v; bi = n; }
      }
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
      const float ov = __shfl_xor(best, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (better(ov, oi, best, bi)) { best = ov; bi = oi; }
    }
    if (r < rows && (tid & 15) == 0) {
      bin[r] = bi;
      action[r] = ((float)bi / (float)NB) * 2.f - 1.f;
    }
  }
}

constexpr int64_t ACTION_BINS_WIDE_MIN_TILES = 1024;   // 16 x 16 output tiles from which a workgroup takes 2 x 2 of them

}  // namespace

extern "C" int dxa_action_rows_fwd(const void* h, const int64_t* off, void* y, int64_t B, int64_t Sq, int64_t d, int64_t n_rows,
                                   int skip, int dtype, dxa_stream_t stream) {
  if (int rc = check_action_dtypes("dxa_action_rows_fwd", dtype, dtype)) return rc;
  DXA_CHECK_ARG(h && off && y, "dxa_action_rows_fwd: null h / off / y");
  if (int rc = check_action_sizes("dxa_action_rows_fwd", B, Sq, d, n_rows, 1, skip)) return rc;
  if (B == 0) return DXA_OK;
  hipStream_t st = (hipStream_t)stream;
  const int vec = dtype == DXA_BF16 ? 8 : 4;
  const bool vec_ok = al16(h) && al16(y) && d % vec == 0;
  dim3 grid((unsigned)(B * n_rows));
#define ROWS(T_, V_) hipLaunchKernelGGL((action_rows_fwd_k<T_, V_>), grid, dim3(256), 0, st, (const T_*)h, off, (T_*)y, Sq, d, n_rows, skip)
  if (dtype == DXA_BF16) { if (vec_ok) ROWS(bf16_t, 8); else ROWS(bf16_t, 1); }
  else { if (vec_ok) ROWS(float, 4); else ROWS(float, 1); }
#undef ROWS
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}

extern "C" int dxa_action_rows_bwd(const void* dy, const int64_t* off, void* dh, int64_t B, int64_t Sq, int64_t d, int64_t n_rows,
                                   int skip, int dtype, dxa_stream_t stream) {
  if (int rc = check_action_dtypes("dxa_action_rows_bwd", dtype, dtype)) return rc;
  DXA_CHECK_ARG(dy && off && dh, "dxa_action_rows_bwd: null dy / off / dh");
  if (int rc = check_action_sizes("dxa_action_rows_bwd", B, Sq, d, n_rows, 1, skip)) return rc;
  if (B == 0) return DXA_OK;
  hipStream_t st = (hipStream_t)stream;
  const int vec = dtype == DXA_BF16 ? 8 : 4;
  const bool vec_ok = al16(dy) && al16(dh) && d % vec == 0;
  dim3 grid((unsigned)dxa_grid1d(B * Sq, 1, 256 * 8));
#define ROWSB(T_, V_) hipLaunchKernelGGL((action_rows_bwd_k<T_, V_>), grid, dim3(256), 0, st, (const T_*)dy, off, (T_*)dh, B, Sq, d, n_rows, skip)
  if (dtype == DXA_BF16) { if (vec_ok) ROWSB(bf16_t, 8); else ROWSB(bf16_t, 1); }
  else { if (vec_ok) ROWSB(float, 4); else ROWSB(float, 1); }
#undef ROWSB
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}

extern "C" int dxa_action_fill_fwd(void* x, const void* row, const void* state, const int64_t* off, int64_t B, int64_t Sq, int64_t d,
                                   int64_t n_rows, int dtype, int row_dtype, dxa_stream_t stream) {
  if (int rc = check_action_dtypes("dxa_action_fill_fwd", dtype, row_dtype == DXA_F32 ? DXA_F32 : dtype)) return rc;
  DXA_CHECK_ARG(row_dtype == DXA_F32 || row_dtype == dtype, "dxa_action_fill_fwd: the row is fp32 or in the dtype of x (%d,%d)", dtype, row_dtype);
  DXA_CHECK_ARG(x && row && off, "dxa_action_fill_fwd: null x / row / off");
  const int skip = state ? 1 : 0;
  if (int rc = check_action_sizes("dxa_action_fill_fwd", B, Sq, d, n_rows, 1, skip)) return rc;
  if (B == 0) return DXA_OK;
  hipStream_t st = (hipStream_t)stream;
  const int vec = dtype == DXA_BF16 ? 8 : 4;
  const bool vec_ok = al16(x) && al16(row) && (!state || al16(state)) && d % vec == 0;
  dim3 grid((unsigned)(B * (n_rows + skip)));
#define FILL(T_, TQ_, V_) hipLaunchKernelGGL((action_put_fwd_k<T_, TQ_, V_>), grid, dim3(256), 0, st, (T_*)x, (const TQ_*)row, (const T_*)state, off, Sq, d, n_rows, skip, (int64_t)0)
  if (dtype == DXA_BF16 && row_dtype == DXA_BF16) { if (vec_ok) FILL(bf16_t, bf16_t, 8); else FILL(bf16_t, bf16_t, 1); }
  else if (dtype == DXA_BF16) { if (vec_ok) FILL(bf16_t, float, 8); else FILL(bf16_t, float, 1); }
  else { if (vec_ok) FILL(float, float, 4); else FILL(float, float, 1); }
#undef FILL
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}

extern "C" int dxa_action_fill_bwd_blocks(int64_t rows) {
  if (rows < 1) rows = 1;
  return (int)((rows + FILL_CHUNK - 1) / FILL_CHUNK);
}

extern "C" int dxa_action_fill_bwd(const void* dx, const int64_t* off, float* drow, void* dstate, float* partial, int64_t B, int64_t Sq,
                                   int64_t d, int64_t n_rows, int skip, int accumulate, int dtype, dxa_stream_t stream) {
  if (int rc = check_action_dtypes("dxa_action_fill_bwd", dtype, dtype)) return rc;
  DXA_CHECK_ARG(dx && off && drow && partial, "dxa_action_fill_bwd: null dx / off / drow / partial");
  DXA_CHECK_ARG(!dstate || skip == 1, "dxa_action_fill_bwd: dstate without a state row (skip = 0)");
  if (int rc = check_action_sizes("dxa_action_fill_bwd", B, Sq, d, n_rows, 1, skip)) return rc;
  DXA_CHECK_ARG(B >= 1 && B <= 32767 && B * n_rows <= (1ll << 19),                 // (chunks + B workgroups along grid y)
                "dxa_action_fill_bwd: B = %lld outside [1, 32767] or B * n_rows = %lld above 2^19", (long long)B, (long long)(B * n_rows));
  hipStream_t st = (hipStream_t)stream;
  const int64_t chunks = dxa_action_fill_bwd_blocks(B * n_rows);
  const int vec = dtype == DXA_BF16 ? 8 : 4;
  const bool vec_ok = al16(dx) && al16(partial) && (!dstate || al16(dstate)) && d % vec == 0;
  {
    const int v = vec_ok ? vec : 1;
    dim3 grid((unsigned)dxa_cdiv(d, 256 * v), (unsigned)(chunks + (dstate ? B : 0)));
#define FILLB(T_, V_) hipLaunchKernelGGL((action_fill_bwd_part_k<T_, V_>), grid, dim3(256), 0, st, (const T_*)dx, off, partial, (T_*)dstate, B, Sq, d, n_rows, skip, chunks)
    if (dtype == DXA_BF16) { if (vec_ok) FILLB(bf16_t, 8); else FILLB(bf16_t, 1); }
    else { if (vec_ok) FILLB(float, 4); else FILLB(float, 1); }
#undef FILLB
    DXA_CHECK_LAUNCH();
  }
  const bool v4 = al16(partial) && al16(drow) && d % 4 == 0;
  if (v4) hipLaunchKernelGGL((action_fill_bwd_fold_k<4>), dim3((unsigned)dxa_cdiv(d, 1024)), dim3(256), 0, st, partial, drow, d, chunks, accumulate);
  else hipLaunchKernelGGL((action_fill_bwd_fold_k<1>), dim3((unsigned)dxa_cdiv(d, 256)), dim3(256), 0, st, partial, drow, d, chunks, accumulate);
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}

extern "C" int dxa_action_bins_counters(int64_t rows) {
  if (rows < 1) rows = 1;
  return (int)(((rows + 15) / 16 + 3) / 4 * 4);
}

extern "C" int dxa_action_bins_fwd(const void* h, const int64_t* off, const void* w_bins, void* bin_logits, int64_t* bin, float* action,
                                   int32_t* counters, int64_t B, int64_t Sq, int64_t d, int64_t n_rows, int skip, int64_t n_bins,
                                   int dtype, dxa_stream_t stream) {
  if (int rc = check_action_dtypes("dxa_action_bins_fwd", dtype, dtype)) return rc;
  DXA_CHECK_ARG(h && off && w_bins && bin_logits && bin && action && counters,
                "dxa_action_bins_fwd: null h / off / w_bins / bin_logits / bin / action / counters");
  if (int rc = check_action_sizes("dxa_action_bins_fwd", B, Sq, d, n_rows, 1, skip)) return rc;
  DXA_CHECK_ARG(n_bins >= 1 && n_bins <= (1 << 16), "dxa_action_bins_fwd: n_bins = %lld outside [1, 65536]", (long long)n_bins);
  DXA_CHECK_ARG(B * n_rows <= (1ll << 24), "dxa_action_bins_fwd: B * n_rows = %lld above 2^24", (long long)(B * n_rows));
  const int kl = dtype == DXA_BF16 ? 8 : 4;
  if (d % kl != 0 || !al16(h) || !al16(w_bins) || (reinterpret_cast<uintptr_t>(counters) & 15) != 0) {
    dxa_set_error("dxa_action_bins_fwd: d = %lld must be a multiple of %d and h / w_bins / counters 16-byte aligned (the MFMA operands "
                  "are loaded 16 bytes per lane)", (long long)d, kl);
    return DXA_ERR_UNSUPPORTED;
  }
  if (B == 0) return DXA_OK;
  hipStream_t st = (hipStream_t)stream;
  const int64_t rows = B * n_rows;
  const int64_t nbt = (n_bins + 15) / 16, rtiles = (rows + 15) / 16;
  const int tm = rtiles * nbt >= ACTION_BINS_WIDE_MIN_TILES ? 2 : 1;
  const int nbg = (int)((nbt + tm - 1) / tm);
  const int64_t rgroups = (rtiles + tm - 1) / tm;
  // the tickets of this call: zeroed on the stream ahead of the launch, every call
  DXA_CHECK_HIP(hipMemsetAsync(counters, 0, (size_t)dxa_action_bins_counters(rows) * sizeof(int32_t), st));
  dim3 grid((unsigned)(rgroups * nbg));
#define BINS(T_, M_) hipLaunchKernelGGL((action_bins_k<T_, M_>), grid, dim3(256), 0, st, (const T_*)h, off, (const T_*)w_bins, (T_*)bin_logits, bin, action, (int*)counters, rows, Sq, d, n_rows, skip, (int)n_bins, nbg)
  if (dtype == DXA_BF16) { if (tm == 2) BINS(bf16_t, 2); else BINS(bf16_t, 1); }
  else { if (tm == 2) BINS(float, 2); else BINS(float, 1); }
#undef BINS
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}
