// RMSNorm / LayerNorm forward+backward and column sums (HBM-bound; wave64 shuffle reductions).
// One wavefront owns one row in the forward (no LDS, no barriers): 16-byte loads, fp32 statistics,
// row re-read from L1/L2 for the normalise pass.  The backward keeps one row per wavefront too and
// accumulates the weight/bias gradient partials of a workgroup's rows in a per-workgroup fp32 slab
// (L2 resident), reduced afterwards by dxa_colsum: deterministic, no atomics.
#include <stdlib.h>

#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------- RMSNorm
template <typename T, typename TW, int VEC>
__global__ __launch_bounds__(256) void rmsnorm_fwd_k(const T* __restrict__ x, const TW* __restrict__ w,
                                                     T* __restrict__ y, float* __restrict__ rstd_out,
                                                     int64_t rows, int64_t cols, float eps) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const T* xr = x + row * cols;
  float ss = 0.f;
  for (int64_t c = (int64_t)lane * VEC; c < cols; c += 64 * VEC) {
    float v[VEC];
    Vec<T, VEC>::ld(v, xr + c);
#pragma unroll
    for (int i = 0; i < VEC; ++i) ss += v[i] * v[i];
  }
  ss = wave_sum(ss);
  const float rstd = rsqrtf(ss / (float)cols + eps);
  if (lane == 0 && rstd_out) rstd_out[row] = rstd;
  T* yr = y + row * cols;
  for (int64_t c = (int64_t)lane * VEC; c < cols; c += 64 * VEC) {
    float v[VEC], g[VEC];
    Vec<T, VEC>::ld(v, xr + c);
    if (w) {
      Vec<TW, VEC>::ld(g, w + c);
    } else {
#pragma unroll
      for (int i = 0; i < VEC; ++i) g[i] = 1.f;
    }
#pragma unroll
    for (int i = 0; i < VEC; ++i) v[i] = g[i] * rnd<T>(v[i] * rstd);
    Vec<T, VEC>::st(yr + c, v);
  }
}

// partial_dw: [gridDim.x][cols]; every block zeroes its own slab first
template <typename T, typename TW, int VEC>
__global__ __launch_bounds__(256) void rmsnorm_bwd_k(const T* __restrict__ dy, const T* __restrict__ x,
                                                     const TW* __restrict__ w, const float* __restrict__ rstd,
                                                     T* __restrict__ dx, const T* __restrict__ res,
                                                     float* __restrict__ partial, int64_t rows, int64_t cols) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* slab = w ? partial + (int64_t)blockIdx.x * cols : nullptr;
  if (w) {
    for (int64_t c = threadIdx.x; c < cols; c += 256) slab[c] = 0.f;
    __syncthreads();
  }
  // rows are dealt round-robin: block b takes rows b*4+wave + k*gridDim.x*4.  The four waves of a block
  // add into the same slab columns -> serialise them wave by wave (deterministic order).
  for (int64_t base = (int64_t)blockIdx.x * 4; base < rows; base += (int64_t)gridDim.x * 4) {
    const int64_t row = base + wave;
    const bool ok = row < rows;
    float rs = 0.f, cterm = 0.f;
    if (ok) {
      rs = rstd[row];
      const T* xr = x + row * cols;
      const T* gr = dy + row * cols;
      float s = 0.f;
      for (int64_t c = (int64_t)lane * VEC; c < cols; c += 64 * VEC) {
        float xv[VEC], gv[VEC], wv[VEC];
        Vec<T, VEC>::ld(xv, xr + c);
        Vec<T, VEC>::ld(gv, gr + c);
        if (w) Vec<TW, VEC>::ld(wv, w + c);
#pragma unroll
        for (int i = 0; i < VEC; ++i) s += gv[i] * (w ? wv[i] : 1.f) * (xv[i] * rs);
      }
      cterm = wave_sum(s) / (float)cols;
      T* dxr = dx + row * cols;
      for (int64_t c = (int64_t)lane * VEC; c < cols; c += 64 * VEC) {
        float xv[VEC], gv[VEC], wv[VEC], o[VEC];
        Vec<T, VEC>::ld(xv, xr + c);
        Vec<T, VEC>::ld(gv, gr + c);
        if (w) Vec<TW, VEC>::ld(wv, w + c);
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          const float xh = xv[i] * rs;
          o[i] = rs * (gv[i] * (w ? wv[i] : 1.f) - xh * cterm);
        }
        if (res) {
          float rv[VEC];
          Vec<T, VEC>::ld(rv, res + row * cols + c);
#pragma unroll
          for (int i = 0; i < VEC; ++i) o[i] += rv[i];
        }
        Vec<T, VEC>::st(dxr + c, o);
      }
    }
    if (w) {
      for (int turn = 0; turn < 4; ++turn) {
        if (turn == wave && ok) {
          const T* xr = x + row * cols;
          const T* gr = dy + row * cols;
          for (int64_t c = (int64_t)lane * VEC; c < cols; c += 64 * VEC) {
            float xv[VEC], gv[VEC];
            Vec<T, VEC>::ld(xv, xr + c);
            Vec<T, VEC>::ld(gv, gr + c);
#pragma unroll
            for (int i = 0; i < VEC; ++i) slab[c + i] += gv[i] * rnd<T>(xv[i] * rs);
          }
        }
        __syncthreads();
      }
    }
  }
}

// ----------------------------------------------------------------------------------------- LayerNorm
// ADD (dxa_add_layernorm_fwd/bwd): the normalised row is x + x2, formed in fp32 from the two inputs wherever the row is read and
// never rounded or written; compiled away otherwise
template <typename T, int VEC, bool ADD>
__device__ __forceinline__ void ld_row(float (&v)[VEC], const T* xr, const T* x2r, int64_t c) {
  Vec<T, VEC>::ld(v, xr + c);
  if constexpr (ADD) {
    float a[VEC];
    Vec<T, VEC>::ld(a, x2r + c);
#pragma unroll
    for (int i = 0; i < VEC; ++i) v[i] += a[i];
  }
}

template <typename T, typename TW, int VEC, bool ADD = false>
__global__ __launch_bounds__(256) void layernorm_fwd_k(const T* __restrict__ x, const TW* __restrict__ w,
                                                       const TW* __restrict__ b, T* __restrict__ y,
                                                       float* __restrict__ mean_out, float* __restrict__ rstd_out,
                                                       int64_t rows, int64_t cols, float eps, const T* __restrict__ x2 = nullptr) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const T* xr = x + row * cols;
  const T* x2r = ADD ? x2 + row * cols : nullptr;
  float s = 0.f;
  for (int64_t c = (int64_t)lane * VEC; c < cols; c += 64 * VEC) {
    float v[VEC];
    ld_row<T, VEC, ADD>(v, xr, x2r, c);
#pragma unroll
    for (int i = 0; i < VEC; ++i) s += v[i];
  }
  const float mean = wave_sum(s) / (float)cols;
  float ss = 0.f;
  for (int64_t c = (int64_t)lane * VEC; c < cols; c += 64 * VEC) {
    float v[VEC];
    ld_row<T, VEC, ADD>(v, xr, x2r, c);
#pragma unroll
    for (int i = 0; i < VEC; ++i) { const float d = v[i] - mean; ss += d * d; }
  }
  const float rstd = rsqrtf(wave_sum(ss) / (float)cols + eps);
  if (lane == 0) {
    if (mean_out) mean_out[row] = mean;
    if (rstd_out) rstd_out[row] = rstd;
  }
  T* yr = y + row * cols;
  for (int64_t c = (int64_t)lane * VEC; c < cols; c += 64 * VEC) {
    float v[VEC], g[VEC], bb[VEC];
    ld_row<T, VEC, ADD>(v, xr, x2r, c);
    if (w) Vec<TW, VEC>::ld(g, w + c);
    if (b) Vec<TW, VEC>::ld(bb, b + c);
#pragma unroll
    for (int i = 0; i < VEC; ++i) v[i] = (v[i] - mean) * rstd * (w ? g[i] : 1.f) + (b ? bb[i] : 0.f);
    Vec<T, VEC>::st(yr + c, v);
  }
}

// partial: [gridDim.x][2*cols] = (dw | db)
template <typename T, typename TW, int VEC, bool ADD = false>
__global__ __launch_bounds__(256) void layernorm_bwd_k(const T* __restrict__ dy, const T* __restrict__ x,
                                                       const TW* __restrict__ w, const float* __restrict__ mean,
                                                       const float* __restrict__ rstd, T* __restrict__ dx,
                                                       const T* __restrict__ res, float* __restrict__ partial,
                                                       int64_t rows, int64_t cols, const T* __restrict__ x2 = nullptr) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* slab = partial ? partial + (int64_t)blockIdx.x * 2 * cols : nullptr;
  if (slab) {
    for (int64_t c = threadIdx.x; c < 2 * cols; c += 256) slab[c] = 0.f;
    __syncthreads();
  }
  for (int64_t base = (int64_t)blockIdx.x * 4; base < rows; base += (int64_t)gridDim.x * 4) {
    const int64_t row = base + wave;
    const bool ok = row < rows;
    float rs = 0.f, mu = 0.f;
    if (ok) {
      rs = rstd[row];
      mu = mean[row];
      const T* xr = x + row * cols;
      const T* x2r = ADD ? x2 + row * cols : nullptr;
      const T* gr = dy + row * cols;
      float s1 = 0.f, s2 = 0.f;
      for (int64_t c = (int64_t)lane * VEC; c < cols; c += 64 * VEC) {
        float xv[VEC], gv[VEC], wv[VEC];
        ld_row<T, VEC, ADD>(xv, xr, x2r, c);
        Vec<T, VEC>::ld(gv, gr + c);
        if (w) Vec<TW, VEC>::ld(wv, w + c);
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          const float g = gv[i] * (w ? wv[i] : 1.f);
          s1 += g;
          s2 += g * ((xv[i] - mu) * rs);
        }
      }
      const float c1 = wave_sum(s1) / (float)cols, c2 = wave_sum(s2) / (float)cols;
      T* dxr = dx + row * cols;
      for (int64_t c = (int64_t)lane * VEC; c < cols; c += 64 * VEC) {
        float xv[VEC], gv[VEC], wv[VEC], o[VEC];
        ld_row<T, VEC, ADD>(xv, xr, x2r, c);
        Vec<T, VEC>::ld(gv, gr + c);
        if (w) Vec<TW, VEC>::ld(wv, w + c);
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          const float g = gv[i] * (w ? wv[i] : 1.f);
          o[i] = rs * (g - c1 - (xv[i] - mu) * rs * c2);
        }
        if (res) {
          float rv[VEC];
          Vec<T, VEC>::ld(rv, res + row * cols + c);
#pragma unroll
          for (int i = 0; i < VEC; ++i) o[i] += rv[i];
        }
        Vec<T, VEC>::st(dxr + c, o);
      }
    }
    if (slab) {
      for (int turn = 0; turn < 4; ++turn) {
        if (turn == wave && ok) {
          const T* xr = x + row * cols;
          const T* x2r = ADD ? x2 + row * cols : nullptr;
          const T* gr = dy + row * cols;
          for (int64_t c = (int64_t)lane * VEC; c < cols; c += 64 * VEC) {
            float xv[VEC], gv[VEC];
            ld_row<T, VEC, ADD>(xv, xr, x2r, c);
            Vec<T, VEC>::ld(gv, gr + c);
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
              slab[c + i] += gv[i] * ((xv[i] - mu) * rs);
              slab[cols + c + i] += gv[i];
            }
          }
        }
        __syncthreads();
      }
    }
  }
}

// -------------------------------------------------------------------------------------------- colsum
// stage 1: grid (col tiles of 256, row splits); block 256 = 4 waves; lane owns 4 consecutive columns
// DIRECT: a single row split — the block's sums are the result: written (or accumulated) straight into `part` = out
template <typename T, bool DIRECT = false>
__global__ __launch_bounds__(256) void colsum_stage1_k(const T* __restrict__ x, int64_t ld, float* __restrict__ part,
                                                       int64_t rows, int64_t cols, int vec, int accumulate = 0) {
  __shared__ float red[4][256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t c0 = (int64_t)blockIdx.x * 256 + lane * 4;
  const int64_t per = (rows + gridDim.y - 1) / gridDim.y;
  const int64_t r0 = (int64_t)blockIdx.y * per, r1 = min(rows, r0 + per);
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  if (c0 < cols) {
    const int n_ok = (int)min((int64_t)4, cols - c0);
    for (int64_t r = r0 + wave; r < r1; r += 4) {
      const T* p = x + r * ld + c0;
      if (vec && n_ok == 4) {
        float v[4];
        Vec<T, 4>::ld(v, p);
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] += v[i];
      } else {
        for (int i = 0; i < n_ok; ++i) a[i] += ldf<T>(p + i);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) red[wave][lane * 4 + i] = a[i];
  __syncthreads();
  const int t = threadIdx.x;
  const int64_t c = (int64_t)blockIdx.x * 256 + t;
  if (c < cols) {
    const float sum = red[0][t] + red[1][t] + red[2][t] + red[3][t];
    if (DIRECT) part[c] = accumulate ? part[c] + sum : sum;
    else part[(int64_t)blockIdx.y * cols + c] = sum;
  }
}
__global__ void colsum_stage2_k(const float* __restrict__ part, float* __restrict__ out, int nsplit, int64_t cols,
                                int accumulate) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= cols) return;
  // fixed order (split 0, 1, 2, ...), eight independent loads in flight
  float s = 0.f;
  int i = 0;
  for (; i + 8 <= nsplit; i += 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = part[(int64_t)(i + u) * cols + c];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += v[u];
  }
  for (; i < nsplit; ++i) s += part[(int64_t)i * cols + c];
  out[c] = accumulate ? out[c] + s : s;
}

// Both stages in ONE launch: every (column tile, row split) workgroup publishes its partial sums with write-through (sc1)
// stores and bumps the column tile's arrival counter; the LAST workgroup to arrive adds the splits' partials in split order —
// the same order, hence the same bits, as colsum_stage2_k — and leaves the counter zeroed for the next launch.  Saves one
// launch (~4.5 us of kernel + a boundary) per bias / norm-weight gradient: ~280 of them in a DB-CogACT step.
template <typename T>
__global__ __launch_bounds__(256) void colsum_fused_k(const T* __restrict__ x, int64_t ld, float* __restrict__ part,
                                                      float* __restrict__ out, int64_t rows, int64_t cols, int vec,
                                                      int accumulate, int* __restrict__ cnt) {
  __shared__ float red[4][256];
  __shared__ int last;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t c0 = (int64_t)blockIdx.x * 256 + lane * 4;
  const int64_t per = (rows + gridDim.y - 1) / gridDim.y;
  const int64_t r0 = (int64_t)blockIdx.y * per, r1 = min(rows, r0 + per);
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  if (c0 < cols) {
    const int n_ok = (int)min((int64_t)4, cols - c0);
    for (int64_t r = r0 + wave; r < r1; r += 4) {
      const T* p = x + r * ld + c0;
      if (vec && n_ok == 4) {
        float v[4];
        Vec<T, 4>::ld(v, p);
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] += v[i];
      } else {
        for (int i = 0; i < n_ok; ++i) a[i] += ldf<T>(p + i);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) red[wave][lane * 4 + i] = a[i];
  __syncthreads();
  const int t = threadIdx.x;
  const int64_t c = (int64_t)blockIdx.x * 256 + t;
  if (c < cols)
    __hip_atomic_store(part + (int64_t)blockIdx.y * cols + c, red[0][t] + red[1][t] + red[2][t] + red[3][t], __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // the write-through stores are acknowledged before the ticket
  __syncthreads();
  if (t == 0) {
    const int arrived = __hip_atomic_fetch_add(cnt + blockIdx.x, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1;
    last = arrived == (int)gridDim.y;
    if (last) __hip_atomic_store(cnt + blockIdx.x, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (!last || c >= cols) return;
  const int nsplit = (int)gridDim.y;
  float s = 0.f;
  int i = 0;
  for (; i + 8 <= nsplit; i += 8) {                         // fixed order (split 0, 1, 2, ...), eight loads in flight
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = __hip_atomic_load(part + (int64_t)(i + u) * cols + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (int u = 0; u < 8; ++u) s += v[u];
  }
  for (; i < nsplit; ++i) s += __hip_atomic_load(part + (int64_t)i * cols + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  out[c] = accumulate ? out[c] + s : s;
}

// Fast backward (cols % 4 == 0, cols <= 4096): a wave owns whole rows, keeps its weight/bias-gradient partial
// sums in REGISTERS (16 x 4 columns per lane) over all its rows; no LDS, no barriers, no serialisation between the
// waves of a workgroup until the very end, where the four waves fold into ONE partial row; x/dy are read twice
// (second pass from L1/L2).  `res` (optional) is added to dx: the gradient of the residual branch around the norm'd
// sub-block, which used to be a separate add kernel.  partial: [gridDim.x][(LN ? 2 : 1) * cols].
template <typename T, typename TW, bool LN>
__global__ __launch_bounds__(256) void norm_bwd_fast_k(const T* __restrict__ dy, const T* __restrict__ x,
                                                       const TW* __restrict__ w, const float* __restrict__ mean,
                                                       const float* __restrict__ rstd, T* __restrict__ dx,
                                                       const T* __restrict__ res, float* __restrict__ partial,
                                                       int64_t rows, int64_t cols) {
  constexpr int NIT = 16;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t prow = (int64_t)blockIdx.x * 4 + wave;
  float aw[NIT][4], ab[NIT][4];
#pragma unroll
  for (int it = 0; it < NIT; ++it)
#pragma unroll
    for (int i = 0; i < 4; ++i) { aw[it][i] = 0.f; ab[it][i] = 0.f; }
  for (int64_t row = prow; row < rows; row += (int64_t)gridDim.x * 4) {
    const float rs = rstd[row];
    const float mu = LN ? mean[row] : 0.f;
    const T* xr = x + row * cols;
    const T* gr = dy + row * cols;
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int64_t c = ((int64_t)it * 64 + lane) * 4;
      if (c < cols) {
        float xv[4], gv[4], wv[4] = {1.f, 1.f, 1.f, 1.f};
        Vec<T, 4>::ld(xv, xr + c);
        Vec<T, 4>::ld(gv, gr + c);
        if (w) Vec<TW, 4>::ld(wv, w + c);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float g = gv[i] * wv[i];
          s1 += g;
          s2 += g * ((xv[i] - mu) * rs);
        }
      }
    }
    const float c1 = LN ? wave_sum(s1) / (float)cols : 0.f;
    const float c2 = wave_sum(s2) / (float)cols;
    T* dxr = dx + row * cols;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int64_t c = ((int64_t)it * 64 + lane) * 4;
      if (c < cols) {
        float xv[4], gv[4], wv[4] = {1.f, 1.f, 1.f, 1.f}, o[4];
        Vec<T, 4>::ld(xv, xr + c);
        Vec<T, 4>::ld(gv, gr + c);
        if (w) Vec<TW, 4>::ld(wv, w + c);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float xh = (xv[i] - mu) * rs;
          o[i] = rs * (gv[i] * wv[i] - c1 - xh * c2);
          aw[it][i] += gv[i] * (LN ? xh : rnd<T>(xh));
          ab[it][i] += gv[i];
        }
        if (res) {                     // residual branch of the block: dx = norm backward + the gradient that bypassed it
          float rv[4];
          Vec<T, 4>::ld(rv, res + row * cols + c);
#pragma unroll
          for (int i = 0; i < 4; ++i) o[i] += rv[i];
        }
        Vec<T, 4>::st(dxr + c, o);
      }
    }
  }
  if (partial) {
    // the four waves fold their register partials through LDS in a fixed order (3, 2, 1, then wave 0 adds its own and
    // writes): ONE partial row per workgroup — a quarter of the former partial traffic and of the column sum after it
    __shared__ float sh[(LN ? 2 : 1) * 4096];
    for (int turn = 3; turn >= 1; --turn) {
      if (wave == turn) {
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
          const int64_t c = ((int64_t)it * 64 + lane) * 4;
          if (c < cols) {
            float4* pw = reinterpret_cast<float4*>(sh + c);
            float4* pb = reinterpret_cast<float4*>(sh + cols + c);
            if (turn == 3) {
              *pw = make_float4(aw[it][0], aw[it][1], aw[it][2], aw[it][3]);
              if (LN) *pb = make_float4(ab[it][0], ab[it][1], ab[it][2], ab[it][3]);
            } else {
              float4 t = *pw;
              *pw = make_float4(t.x + aw[it][0], t.y + aw[it][1], t.z + aw[it][2], t.w + aw[it][3]);
              if (LN) { t = *pb; *pb = make_float4(t.x + ab[it][0], t.y + ab[it][1], t.z + ab[it][2], t.w + ab[it][3]); }
            }
          }
        }
      }
      __syncthreads();
    }
    if (wave == 0) {
      float* pr = partial + (int64_t)blockIdx.x * (LN ? 2 : 1) * cols;
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        const int64_t c = ((int64_t)it * 64 + lane) * 4;
        if (c < cols) {
          const float4 t = *reinterpret_cast<const float4*>(sh + c);
          *reinterpret_cast<float4*>(pr + c) = make_float4(t.x + aw[it][0], t.y + aw[it][1], t.z + aw[it][2], t.w + aw[it][3]);
          if (LN) {
            const float4 u = *reinterpret_cast<const float4*>(sh + cols + c);
            *reinterpret_cast<float4*>(pr + cols + c) = make_float4(u.x + ab[it][0], u.y + ab[it][1], u.z + ab[it][2], u.w + ab[it][3]);
          }
        }
      }
    }
  }
}

// bf16 rows, cols % 8 == 0, cols <= 4096: the same backward with 16-byte accesses (8 columns per lane per step) and the row
// (x, dy) held in registers between the statistics pass and the dx pass: x and dy are read ONCE.
template <typename TW, bool LN>
__global__ __launch_bounds__(256) void norm_bwd_fast8_k(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
                                                        const TW* __restrict__ w, const float* __restrict__ mean,
                                                        const float* __restrict__ rstd, bf16_t* __restrict__ dx,
                                                        const bf16_t* __restrict__ res, float* __restrict__ partial,
                                                        int64_t rows, int64_t cols) {
  constexpr int NIT = 8;
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t prow = (int64_t)blockIdx.x * 4 + wave;
  float aw[NIT][8], ab[LN ? NIT : 1][8];
#pragma unroll
  for (int it = 0; it < NIT; ++it)
#pragma unroll
    for (int i = 0; i < 8; ++i) { aw[it][i] = 0.f; if (LN) ab[it][i] = 0.f; }
  auto unpack = [](const u32x4& v, float (&o)[8]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) { o[2 * e] = __uint_as_float(v[e] << 16); o[2 * e + 1] = __uint_as_float(v[e] & 0xffff0000u); }
  };
  for (int64_t row = prow; row < rows; row += (int64_t)gridDim.x * 4) {
    const float rs = rstd[row];
    const float mu = LN ? mean[row] : 0.f;
    const bf16_t* xr = x + row * cols;
    const bf16_t* gr = dy + row * cols;
    u32x4 xv[NIT], gv[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int64_t c = ((int64_t)it * 64 + lane) * 8;
      xv[it] = c < cols ? *reinterpret_cast<const u32x4*>(xr + c) : (u32x4){0u, 0u, 0u, 0u};
      gv[it] = c < cols ? *reinterpret_cast<const u32x4*>(gr + c) : (u32x4){0u, 0u, 0u, 0u};
    }
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int64_t c = ((int64_t)it * 64 + lane) * 8;
      if (c < cols) {
        float xf[8], gf[8], w0[4] = {1.f, 1.f, 1.f, 1.f}, w1[4] = {1.f, 1.f, 1.f, 1.f};
        unpack(xv[it], xf); unpack(gv[it], gf);
        if (w) { Vec<TW, 4>::ld(w0, w + c); Vec<TW, 4>::ld(w1, w + c + 4); }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float g = gf[i] * (i < 4 ? w0[i] : w1[i - 4]);
          s1 += g;
          s2 += g * ((xf[i] - mu) * rs);
        }
      }
    }
    const float c1 = LN ? wave_sum(s1) / (float)cols : 0.f;
    const float c2 = wave_sum(s2) / (float)cols;
    bf16_t* dxr = dx + row * cols;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int64_t c = ((int64_t)it * 64 + lane) * 8;
      if (c < cols) {
        float xf[8], gf[8], o[8], w0[4] = {1.f, 1.f, 1.f, 1.f}, w1[4] = {1.f, 1.f, 1.f, 1.f};
        unpack(xv[it], xf); unpack(gv[it], gf);
        if (w) { Vec<TW, 4>::ld(w0, w + c); Vec<TW, 4>::ld(w1, w + c + 4); }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float xh = (xf[i] - mu) * rs;
          o[i] = rs * (gf[i] * (i < 4 ? w0[i] : w1[i - 4]) - c1 - xh * c2);
          aw[it][i] += gf[i] * (LN ? xh : rnd<bf16_t>(xh));
          if (LN) ab[it][i] += gf[i];
        }
        if (res) {
          float rf[8];
          unpack(*reinterpret_cast<const u32x4*>(res + row * cols + c), rf);
#pragma unroll
          for (int i = 0; i < 8; ++i) o[i] += rf[i];
        }
        u32x4 ov;
#pragma unroll
        for (int e = 0; e < 4; ++e) ov[e] = pack_bf16x2(o[2 * e], o[2 * e + 1]);
        *reinterpret_cast<u32x4*>(dxr + c) = ov;
      }
    }
  }
  if (partial) {
    __shared__ float sh[(LN ? 2 : 1) * 4096];
    for (int turn = 3; turn >= 1; --turn) {
      if (wave == turn) {
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
          const int64_t c = ((int64_t)it * 64 + lane) * 8;
          if (c < cols) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
              sh[c + i] = turn == 3 ? aw[it][i] : sh[c + i] + aw[it][i];
              if (LN) sh[cols + c + i] = turn == 3 ? ab[it][i] : sh[cols + c + i] + ab[it][i];
            }
          }
        }
      }
      __syncthreads();
    }
    if (wave == 0) {
      float* pr = partial + (int64_t)blockIdx.x * (LN ? 2 : 1) * cols;
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        const int64_t c = ((int64_t)it * 64 + lane) * 8;
        if (c < cols) {
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            pr[c + i] = sh[c + i] + aw[it][i];
            if (LN) pr[cols + c + i] = sh[cols + c + i] + ab[it][i];
          }
        }
      }
    }
  }
}

// RMSNorm backward, bf16 rows, cols % 16 == 0, cols <= 8192 (round 5).  norm_bwd_fast8_k gives a wave a whole row: x and dy
// of the row (2 x 28 registers at 3584 columns) and the wave's column sums (56) leave two waves per SIMD, and every wave walks
// load -> reduce -> load residual -> store for 2-3 rows in sequence: 57 us for 139 MB (2.4 TB/s) on the decoder's [4592, 3584]
// rows.  Here a row is split between TWO waves (columns [0, cols/2) and [cols/2, cols)) of an 8-wave workgroup (4 rows at a
// time, as before): half the registers per wave, so twice the waves — and twice the bytes — in flight per CU; the residual is
// requested together with x and dy; the two halves of the row statistic meet in LDS and are added in a fixed order
// (deterministic).  Same partial-sum layout as the other backward kernels: one row of column sums per workgroup.
// NIT 16-byte chunks per lane: NIT x 64 lanes x 8 columns per half row (4: cols <= 4096); NS rows per workgroup pass (2 NS waves)
template <typename TW, int NIT, int NS>
__global__ __launch_bounds__(NS * 128, (NIT <= 4 ? NS : 2)) void rmsnorm_bwd_split_k(
    const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x, const TW* __restrict__ w, const float* __restrict__ rstd,
    bf16_t* __restrict__ dx, const bf16_t* __restrict__ res, float* __restrict__ partial, int64_t rows, int64_t cols) {
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  __shared__ float red[2][NS][2];          // [iteration parity][row slot][column half]
  __shared__ float sh[2][NIT * 512];       // hand-over of a row slot's column sums: [column half][column of the half]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int slot = wave >> 1, half = wave & 1;
  const int64_t hc = cols >> 1, col0 = half * hc;
  auto unpack = [](const u32x4& v, float (&o)[8]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) { o[2 * e] = __uint_as_float(v[e] << 16); o[2 * e + 1] = __uint_as_float(v[e] & 0xffff0000u); }
  };
  float aw[NIT][8];
#pragma unroll
  for (int it = 0; it < NIT; ++it)
#pragma unroll
    for (int i = 0; i < 8; ++i) aw[it][i] = 0.f;
  const int64_t stride = (int64_t)gridDim.x * NS;
  const int64_t iters = (rows + stride - 1) / stride;      // the same trip count for every wave: the loop holds a barrier
  const float inv_cols = 1.f / (float)cols;
  for (int64_t k = 0; k < iters; ++k) {
    const int64_t row = (int64_t)blockIdx.x * NS + slot + k * stride;
    const bool live = row < rows;
    const float rs = live ? rstd[row] : 0.f;
    u32x4 xv[NIT], gv[NIT], rv[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int64_t c = ((int64_t)it * 64 + lane) * 8;
      const bool in = live && c < hc;
      const int64_t off = row * cols + col0 + c;
      xv[it] = in ? *reinterpret_cast<const u32x4*>(x + off) : (u32x4){0u, 0u, 0u, 0u};
      gv[it] = in ? *reinterpret_cast<const u32x4*>(dy + off) : (u32x4){0u, 0u, 0u, 0u};
      rv[it] = (in && res) ? *reinterpret_cast<const u32x4*>(res + off) : (u32x4){0u, 0u, 0u, 0u};
    }
    float s2 = 0.f;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int64_t c = ((int64_t)it * 64 + lane) * 8;
      if (c < hc) {
        float xf[8], gf[8], w0[4] = {1.f, 1.f, 1.f, 1.f}, w1[4] = {1.f, 1.f, 1.f, 1.f};
        unpack(xv[it], xf); unpack(gv[it], gf);
        if (w) { Vec<TW, 4>::ld(w0, w + col0 + c); Vec<TW, 4>::ld(w1, w + col0 + c + 4); }
#pragma unroll
        for (int i = 0; i < 8; ++i) s2 += gf[i] * (i < 4 ? w0[i] : w1[i - 4]) * (xf[i] * rs);
      }
    }
    s2 = wave_sum(s2);
    if (lane == 0) red[k & 1][slot][half] = s2;
    __syncthreads();                       // (parity-indexed slots: the next iteration's writes cannot overtake these reads)
    const float c2 = (red[k & 1][slot][0] + red[k & 1][slot][1]) * inv_cols;
    if (live) {
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        const int64_t c = ((int64_t)it * 64 + lane) * 8;
        if (c < hc) {
          float xf[8], gf[8], rf[8], o[8], w0[4] = {1.f, 1.f, 1.f, 1.f}, w1[4] = {1.f, 1.f, 1.f, 1.f};
          unpack(xv[it], xf); unpack(gv[it], gf); unpack(rv[it], rf);
          if (w) { Vec<TW, 4>::ld(w0, w + col0 + c); Vec<TW, 4>::ld(w1, w + col0 + c + 4); }
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const float xh = xf[i] * rs;
            o[i] = rs * (gf[i] * (i < 4 ? w0[i] : w1[i - 4]) - xh * c2) + rf[i];
            aw[it][i] += gf[i] * rnd<bf16_t>(xh);
          }
          u32x4 ov;
#pragma unroll
          for (int e = 0; e < 4; ++e) ov[e] = pack_bf16x2(o[2 * e], o[2 * e + 1]);
          *reinterpret_cast<u32x4*>(dx + row * cols + col0 + c) = ov;
        }
      }
    }
  }
  if (partial) {
    // column sums: row slots NS-1 .. 1 hand theirs to slot 0's waves (same column half) through LDS, one after the other — a
    // fixed order of additions — and slot 0 writes the workgroup's row
    for (int turn = NS - 1; turn >= 1; --turn) {
      __syncthreads();
      if (slot == turn) {
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
          const int64_t c = ((int64_t)it * 64 + lane) * 8;
          if (c < hc) {
            *reinterpret_cast<float4*>(&sh[half][c]) = make_float4(aw[it][0], aw[it][1], aw[it][2], aw[it][3]);
            *reinterpret_cast<float4*>(&sh[half][c + 4]) = make_float4(aw[it][4], aw[it][5], aw[it][6], aw[it][7]);
          }
        }
      }
      __syncthreads();
      if (slot == 0) {
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
          const int64_t c = ((int64_t)it * 64 + lane) * 8;
          if (c < hc) {
            const float4 a = *reinterpret_cast<const float4*>(&sh[half][c]), b = *reinterpret_cast<const float4*>(&sh[half][c + 4]);
            aw[it][0] += a.x; aw[it][1] += a.y; aw[it][2] += a.z; aw[it][3] += a.w;
            aw[it][4] += b.x; aw[it][5] += b.y; aw[it][6] += b.z; aw[it][7] += b.w;
          }
        }
      }
    }
    if (slot == 0) {
      float* pr = partial + (int64_t)blockIdx.x * cols + col0;
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        const int64_t c = ((int64_t)it * 64 + lane) * 8;
        if (c < hc) {
          *reinterpret_cast<float4*>(pr + c) = make_float4(aw[it][0], aw[it][1], aw[it][2], aw[it][3]);
          *reinterpret_cast<float4*>(pr + c + 4) = make_float4(aw[it][4], aw[it][5], aw[it][6], aw[it][7]);
        }
      }
    }
  }
}

constexpr int NORM_BWD_MAX_BLOCKS = 512;
constexpr int64_t NORM_BWD_FAST_MAX_COLS = 4096;
constexpr size_t DS_LN_MAX_LDS = 60 * 1024;      // partial sums of rows up to 7680 columns stay in LDS (default 64 KB ceiling)
constexpr int ADARMS_BWD_MAX_GROUPS = 128;
// arrival counters of colsum_fused_k: COLSUM_CNT ints per (device, stream), zeroed once (the kernel leaves them zeroed),
// allocated on first use; under capture before they exist the counters are null and the two-launch form, which needs none, runs
constexpr int COLSUM_CNT = 4096;

}  // namespace

// number of partial rows both backward kernels write: one per workgroup (the generic fallback launches as many
// workgroups as the fast kernel, one slab each)
extern "C" int dxa_norm_bwd_blocks(int64_t rows) {
  int64_t g = (rows + 3) / 4;
  if (g < 1) g = 1;
  if (g > NORM_BWD_MAX_BLOCKS) g = NORM_BWD_MAX_BLOCKS;
  return (int)g;
}

extern "C" int dxa_adarms_bwd_groups(int64_t rows_per_sample) {
  int64_t g = (rows_per_sample + 3) / 4;
  if (g < 1) g = 1;
  if (g > ADARMS_BWD_MAX_GROUPS) g = ADARMS_BWD_MAX_GROUPS;
  return (int)g;
}

static int check_norm_dtypes(int dtype, int w_dtype, const char* who) {
  if (!(dtype == DXA_F32 || dtype == DXA_BF16) || !(w_dtype == DXA_F32 || w_dtype == DXA_BF16) ||
      (dtype == DXA_F32 && w_dtype == DXA_BF16)) {
    dxa_set_error("%s: unsupported dtype combination (%d,%d)", who, dtype, w_dtype);
    return DXA_ERR_UNSUPPORTED;
  }
  return DXA_OK;
}

// ---- The route of a norm call: every choice between kernel instantiations of the entry points below is made in norm_plan, from
// the call's sizes, dtypes, optional operands and pointer alignments alone (nothing is dereferenced and HIP is not touched, so
// dxa_norm_plan answers without a GPU).  The launchers launch what the plan names and hold no condition of their own.
// Within a group of instantiations the index is: + 2 * tw + (scalar) for the (T, TW) pairs tw = (bf16, bf16), (bf16, float),
// (float, float) and the 4-/1-wide (ds: 16-byte/1-wide) forms; + 2 * av + gated for the adarms vector widths av (below).
#define NORM_KERNELS(X)                                                                                                              \
  X(K_RMS_FWD_FAST, "rmsnorm_fwd_fast_k<bf16>") X(K_RMS_FWD_FAST_F, "rmsnorm_fwd_fast_k<float>")                                     \
  X(K_RMS_FWD, "rmsnorm_fwd_k<bf16,bf16,4>") X(K_RMS_FWD_1, "rmsnorm_fwd_k<bf16,bf16,1>")                                           \
  X(K_RMS_FWD_BF4, "rmsnorm_fwd_k<bf16,float,4>") X(K_RMS_FWD_BF1, "rmsnorm_fwd_k<bf16,float,1>")                                   \
  X(K_RMS_FWD_FF4, "rmsnorm_fwd_k<float,float,4>") X(K_RMS_FWD_FF1, "rmsnorm_fwd_k<float,float,1>")                                 \
  X(K_RMS_SPLIT, "rmsnorm_bwd_split_k<bf16,4,4>") X(K_RMS_SPLIT_B8, "rmsnorm_bwd_split_k<bf16,8,4>")                                \
  X(K_RMS_SPLIT_F4, "rmsnorm_bwd_split_k<float,4,4>") X(K_RMS_SPLIT_F8, "rmsnorm_bwd_split_k<float,8,4>")                           \
  X(K_RMS_FAST8, "norm_bwd_fast8_k<bf16,false>") X(K_RMS_FAST8_F, "norm_bwd_fast8_k<float,false>")                                  \
  X(K_RMS_FAST, "norm_bwd_fast_k<bf16,bf16,false>") X(K_RMS_FAST_BF, "norm_bwd_fast_k<bf16,float,false>")                           \
  X(K_RMS_FAST_FF, "norm_bwd_fast_k<float,float,false>")                                                                            \
  X(K_RMS_BWD, "rmsnorm_bwd_k<bf16,bf16,4>") X(K_RMS_BWD_1, "rmsnorm_bwd_k<bf16,bf16,1>")                                           \
  X(K_RMS_BWD_BF4, "rmsnorm_bwd_k<bf16,float,4>") X(K_RMS_BWD_BF1, "rmsnorm_bwd_k<bf16,float,1>")                                   \
  X(K_RMS_BWD_FF4, "rmsnorm_bwd_k<float,float,4>") X(K_RMS_BWD_FF1, "rmsnorm_bwd_k<float,float,1>")                                 \
  X(K_LN_FWD, "layernorm_fwd_k<bf16,bf16,4>") X(K_LN_FWD_1, "layernorm_fwd_k<bf16,bf16,1>")                                         \
  X(K_LN_FWD_BF4, "layernorm_fwd_k<bf16,float,4>") X(K_LN_FWD_BF1, "layernorm_fwd_k<bf16,float,1>")                                 \
  X(K_LN_FWD_FF4, "layernorm_fwd_k<float,float,4>") X(K_LN_FWD_FF1, "layernorm_fwd_k<float,float,1>")                               \
  X(K_LN_FAST, "norm_bwd_fast_k<bf16,bf16,true>") X(K_LN_FAST_BF, "norm_bwd_fast_k<bf16,float,true>")                               \
  X(K_LN_FAST_FF, "norm_bwd_fast_k<float,float,true>")                                                                              \
  X(K_LN_BWD, "layernorm_bwd_k<bf16,bf16,4>") X(K_LN_BWD_1, "layernorm_bwd_k<bf16,bf16,1>")                                         \
  X(K_LN_BWD_BF4, "layernorm_bwd_k<bf16,float,4>") X(K_LN_BWD_BF1, "layernorm_bwd_k<bf16,float,1>")                                 \
  X(K_LN_BWD_FF4, "layernorm_bwd_k<float,float,4>") X(K_LN_BWD_FF1, "layernorm_bwd_k<float,float,1>")                               \
  X(K_ADDLN_FWD, "layernorm_fwd_k<bf16,bf16,4,true>") X(K_ADDLN_FWD_1, "layernorm_fwd_k<bf16,bf16,1,true>")                         \
  X(K_ADDLN_FWD_BF4, "layernorm_fwd_k<bf16,float,4,true>") X(K_ADDLN_FWD_BF1, "layernorm_fwd_k<bf16,float,1,true>")                 \
  X(K_ADDLN_FWD_FF4, "layernorm_fwd_k<float,float,4,true>") X(K_ADDLN_FWD_FF1, "layernorm_fwd_k<float,float,1,true>")               \
  X(K_ADDLN_BWD, "layernorm_bwd_k<bf16,bf16,4,true>") X(K_ADDLN_BWD_1, "layernorm_bwd_k<bf16,bf16,1,true>")                         \
  X(K_ADDLN_BWD_BF4, "layernorm_bwd_k<bf16,float,4,true>") X(K_ADDLN_BWD_BF1, "layernorm_bwd_k<bf16,float,1,true>")                 \
  X(K_ADDLN_BWD_FF4, "layernorm_bwd_k<float,float,4,true>") X(K_ADDLN_BWD_FF1, "layernorm_bwd_k<float,float,1,true>")               \
  X(K_CS_DIRECT, "colsum_stage1_k<bf16,true>") X(K_CS_DIRECT_F, "colsum_stage1_k<float,true>")                                      \
  X(K_CS_FUSED, "colsum_fused_k<bf16>") X(K_CS_FUSED_F, "colsum_fused_k<float>")                                                    \
  X(K_CS_STAGE1, "colsum_stage1_k<bf16,false>") X(K_CS_STAGE1_F, "colsum_stage1_k<float,false>")                                    \
  X(K_CS_STAGE2, "colsum_stage2_k")                                                                                                 \
  X(K_DS_FWD, "ds_layernorm_fwd_k<bf16,bf16,8>") X(K_DS_FWD_1, "ds_layernorm_fwd_k<bf16,bf16,1>")                                   \
  X(K_DS_FWD_BF8, "ds_layernorm_fwd_k<bf16,float,8>") X(K_DS_FWD_BF1, "ds_layernorm_fwd_k<bf16,float,1>")                           \
  X(K_DS_FWD_FF4, "ds_layernorm_fwd_k<float,float,4>") X(K_DS_FWD_FF1, "ds_layernorm_fwd_k<float,float,1>")                         \
  X(K_DS_BWD, "ds_layernorm_bwd_k<bf16,bf16,8>") X(K_DS_BWD_1, "ds_layernorm_bwd_k<bf16,bf16,1>")                                   \
  X(K_DS_BWD_BF8, "ds_layernorm_bwd_k<bf16,float,8>") X(K_DS_BWD_BF1, "ds_layernorm_bwd_k<bf16,float,1>")                           \
  X(K_DS_BWD_FF4, "ds_layernorm_bwd_k<float,float,4>") X(K_DS_BWD_FF1, "ds_layernorm_bwd_k<float,float,1>")                         \
  X(K_AR_FWD_FAST, "adarms_fwd_fast_k<false>") X(K_AR_FWD_FAST_G, "adarms_fwd_fast_k<true>")                                        \
  X(K_AR_FWD, "adarms_fwd_k<bf16,8,false>") X(K_AR_FWD_B8G, "adarms_fwd_k<bf16,8,true>")                                            \
  X(K_AR_FWD_B4, "adarms_fwd_k<bf16,4,false>") X(K_AR_FWD_B4G, "adarms_fwd_k<bf16,4,true>")                                         \
  X(K_AR_FWD_B1, "adarms_fwd_k<bf16,1,false>") X(K_AR_FWD_B1G, "adarms_fwd_k<bf16,1,true>")                                         \
  X(K_AR_FWD_F4, "adarms_fwd_k<float,4,false>") X(K_AR_FWD_F4G, "adarms_fwd_k<float,4,true>")                                       \
  X(K_AR_FWD_F1, "adarms_fwd_k<float,1,false>") X(K_AR_FWD_F1G, "adarms_fwd_k<float,1,true>")                                       \
  X(K_GR_FWD, "gated_residual_fwd_k<bf16,8>") X(K_GR_FWD_B4, "gated_residual_fwd_k<bf16,4>")                                        \
  X(K_GR_FWD_B1, "gated_residual_fwd_k<bf16,1>") X(K_GR_FWD_F4, "gated_residual_fwd_k<float,4>")                                    \
  X(K_GR_FWD_F1, "gated_residual_fwd_k<float,1>")                                                                                   \
  X(K_AR_BWD, "adarms_bwd_k<bf16,8,false>") X(K_AR_BWD_B8G, "adarms_bwd_k<bf16,8,true>")                                            \
  X(K_AR_BWD_B4, "adarms_bwd_k<bf16,4,false>") X(K_AR_BWD_B4G, "adarms_bwd_k<bf16,4,true>")                                         \
  X(K_AR_BWD_B1, "adarms_bwd_k<bf16,1,false>") X(K_AR_BWD_B1G, "adarms_bwd_k<bf16,1,true>")                                         \
  X(K_AR_BWD_F4, "adarms_bwd_k<float,4,false>") X(K_AR_BWD_F4G, "adarms_bwd_k<float,4,true>")                                       \
  X(K_AR_BWD_F1, "adarms_bwd_k<float,1,false>") X(K_AR_BWD_F1G, "adarms_bwd_k<float,1,true>")                                       \
  X(K_GR_BWD, "gated_residual_bwd_k<bf16,8>") X(K_GR_BWD_B4, "gated_residual_bwd_k<bf16,4>")                                        \
  X(K_GR_BWD_B1, "gated_residual_bwd_k<bf16,1>") X(K_GR_BWD_F4, "gated_residual_bwd_k<float,4>")                                    \
  X(K_GR_BWD_F1, "gated_residual_bwd_k<float,1>")                                                                                   \
  X(K_FOLD, "adarms_fold_k<bf16>") X(K_FOLD_F, "adarms_fold_k<float>")

namespace {
#define NORM_KERNEL_ID(id, name) id,
enum NormKernel { NORM_KERNELS(NORM_KERNEL_ID) K_NONE };
#undef NORM_KERNEL_ID
#define NORM_KERNEL_NAME(id, name) name,
const char* const NORM_KERNEL_NAMES[] = {NORM_KERNELS(NORM_KERNEL_NAME)};
#undef NORM_KERNEL_NAME

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool al8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

struct NormPlan {
  int k = K_NONE, k2 = K_NONE;   // the launch(es); K_NONE: nothing to launch (rows == 0)
  const char* mode = nullptr;
  int vec = 1;
  dim3 grid{1, 1, 1}, grid2{1, 1, 1};
  int block = 256, block2 = 256;
  size_t lds = 0;
  int use_lds = 0;               // ds_layernorm_bwd_k: the partial sums live in LDS
  int nsplit = 0;
  int64_t trips = 0;
};

int tw_index(int dtype, int w_dtype) { return dtype == DXA_F32 ? 2 : w_dtype == DXA_BF16 ? 0 : 1; }
int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

int check_downsample_args(const char* who, int64_t N, int64_t G, int64_t C) {
  DXA_CHECK_ARG(N >= 0 && G > 0 && C > 0 && G <= 4096 && C <= (1 << 20) && N <= (1ll << 31),
                "%s: bad sizes N=%lld G=%lld C=%lld", who, (long long)N, (long long)G, (long long)C);
  return DXA_OK;
}

// widest access every pointer and stride allows: 8 (bf16 only), 4 or 1 elements
int adarms_vec(int dtype, int64_t cols, int64_t gate_ld, std::initializer_list<const void*> ptrs) {
  const size_t es = dtype == DXA_BF16 ? 2 : 4;
  int vec = dtype == DXA_BF16 ? 8 : 4;
  for (; vec > 1; vec >>= 1) {
    bool ok = cols % vec == 0 && gate_ld % vec == 0;
    for (const void* p : ptrs) ok = ok && (reinterpret_cast<uintptr_t>(p) % (vec * es)) == 0;
    if (ok) break;
  }
  return vec;
}
// index of an adarms / gated-residual vector width within its group: bf16 8, 4, 1, then fp32 4, 1
int adarms_vidx(int dtype, int vec) { return dtype == DXA_BF16 ? (vec == 8 ? 0 : vec == 4 ? 1 : 2) : (vec == 4 ? 3 : 4); }

int check_adarms(const char* who, int64_t rows, int64_t rps, int64_t cols, int dtype) {
  DXA_CHECK_ARG(dtype == DXA_F32 || dtype == DXA_BF16, "%s: unsupported dtype %d", who, dtype);
  DXA_CHECK_ARG(cols > 0 && rows >= 0 && rps > 0, "%s: bad sizes (rows %lld, rows_per_sample %lld, cols %lld)", who, (long long)rows,
                (long long)rps, (long long)cols);
  DXA_CHECK_ARG(rows % rps == 0, "%s: %lld rows are not a whole number of samples of %lld rows", who, (long long)rows, (long long)rps);
  DXA_CHECK_ARG(rows / rps <= 65535, "%s: more than 65535 samples", who);
  return DXA_OK;
}

// backward kernels with a grid-stride row loop: one workgroup per four rows up to NORM_BWD_MAX_BLOCKS
void plan_bwd_grid(NormPlan* p, int64_t rows) {
  p->grid = dim3((unsigned)dxa_norm_bwd_blocks(rows));
  p->trips = cdiv(rows, (int64_t)p->grid.x * 4);
}

int plan_rmsnorm_fwd(const dxa_norm_desc* d, NormPlan* p) {
  if (int rc = check_norm_dtypes(d->dtype, d->w_dtype, "dxa_rmsnorm_fwd")) return rc;
  const int64_t rows = d->rows, cols = d->cols;
  DXA_CHECK_ARG(d->x && d->y && rows >= 0 && cols > 0, "dxa_rmsnorm_fwd: bad args");
  if (rows == 0) return DXA_OK;
  const bool vec_ok = al16(d->x) && al16(d->y) && (!d->w || al16(d->w));
  p->grid = dim3((unsigned)((rows + 3) / 4));
  p->trips = 1;
  if (d->dtype == DXA_BF16 && vec_ok && cols % 8 == 0 && cols <= 8192) {
    p->k = K_RMS_FWD_FAST + (d->w_dtype == DXA_F32);
    p->vec = 8;
  } else {
    p->vec = vec_ok && cols % 4 == 0 ? 4 : 1;
    p->k = K_RMS_FWD + 2 * tw_index(d->dtype, d->w_dtype) + (p->vec == 1);
  }
  return DXA_OK;
}

// RMSNorm (LN = false) and LayerNorm backward
int plan_norm_bwd(const dxa_norm_desc* d, NormPlan* p, bool LN) {
  const char* who = LN ? "dxa_layernorm_bwd" : "dxa_rmsnorm_bwd";
  if (int rc = check_norm_dtypes(d->dtype, d->w_dtype, who)) return rc;
  const int64_t rows = d->rows, cols = d->cols;
  if (LN) {
    DXA_CHECK_ARG(d->dy && d->x && d->mean && d->rstd && d->dx && rows >= 0 && cols > 0, "dxa_layernorm_bwd: bad args");
    DXA_CHECK_ARG(!d->w || d->partial, "dxa_layernorm_bwd: partial_dwdb required when w is given");
  } else {
    DXA_CHECK_ARG(d->dy && d->x && d->rstd && d->dx && rows >= 0 && cols > 0, "dxa_rmsnorm_bwd: bad args");
    DXA_CHECK_ARG(!d->w || d->partial, "dxa_rmsnorm_bwd: partial_dw required when w is given");
  }
  if (rows == 0) return DXA_OK;
  const bool vec_ok = al16(d->x) && al16(d->dy) && al16(d->dx) && (!d->w || al16(d->w)) && (!d->partial || al16(d->partial)) &&
                      (!d->residual || al16(d->residual));
  const int tw = tw_index(d->dtype, d->w_dtype);
  plan_bwd_grid(p, rows);
  if (!LN && vec_ok && d->dtype == DXA_BF16 && cols % 16 == 0 && cols <= 8192) {
    // the row split between two waves (A/B against the one-wave-per-row kernels: profiles/r05_norm_bwd_split.txt); four rows
    // per workgroup pass (512 threads at 128 registers: a dozen spilled dwords); the three-row form (384 threads, 168
    // registers, no spill) against it: profiles/r05_norm_bwd_split.txt
    p->k = K_RMS_SPLIT + 2 * (d->w_dtype == DXA_F32) + (cols > 4096);
    p->vec = 8;
    p->block = 4 * 128;
  } else if (vec_ok && cols % 4 == 0 && cols <= NORM_BWD_FAST_MAX_COLS) {
    if (!LN && d->dtype == DXA_BF16 && cols % 8 == 0) {   // RMSNorm: 16-byte accesses, one read of x and dy (LayerNorm's second
                                                          // set of partial sums costs it the registers: measured 27 vs 24 us)
      p->k = K_RMS_FAST8 + (d->w_dtype == DXA_F32);
      p->vec = 8;
    } else {
      p->k = (LN ? K_LN_FAST : K_RMS_FAST) + tw;
      p->vec = 4;
    }
  } else {
    p->vec = vec_ok && cols % 4 == 0 ? 4 : 1;
    p->k = (LN ? K_LN_BWD : K_RMS_BWD) + 2 * tw + (p->vec == 1);
  }
  return DXA_OK;
}

int plan_layernorm_fwd(const dxa_norm_desc* d, NormPlan* p) {
  if (int rc = check_norm_dtypes(d->dtype, d->w_dtype, "dxa_layernorm_fwd")) return rc;
  const int64_t rows = d->rows, cols = d->cols;
  DXA_CHECK_ARG(d->x && d->y && rows >= 0 && cols > 0, "dxa_layernorm_fwd: bad args");
  if (rows == 0) return DXA_OK;
  const bool vec_ok = al16(d->x) && al16(d->y) && (!d->w || al16(d->w)) && (!d->b || al16(d->b));
  p->grid = dim3((unsigned)((rows + 3) / 4));
  p->trips = 1;
  p->vec = vec_ok && cols % 4 == 0 ? 4 : 1;
  p->k = K_LN_FWD + 2 * tw_index(d->dtype, d->w_dtype) + (p->vec == 1);
  return DXA_OK;
}

int plan_add_layernorm_fwd(const dxa_norm_desc* d, NormPlan* p) {
  if (int rc = check_norm_dtypes(d->dtype, d->w_dtype, "dxa_add_layernorm_fwd")) return rc;
  const int64_t rows = d->rows, cols = d->cols;
  DXA_CHECK_ARG(d->x && d->x2 && d->y, "dxa_add_layernorm_fwd: null x / res / y");
  DXA_CHECK_ARG(rows >= 0 && cols > 0, "dxa_add_layernorm_fwd: bad sizes (rows %lld, cols %lld)", (long long)rows, (long long)cols);
  if (rows == 0) return DXA_OK;
  const bool vec = al16(d->x) && al16(d->x2) && al16(d->y) && (!d->w || al16(d->w)) && (!d->b || al16(d->b)) && cols % 4 == 0;
  p->grid = dim3((unsigned)((rows + 3) / 4));
  p->trips = 1;
  p->vec = vec ? 4 : 1;
  p->k = K_ADDLN_FWD + 2 * tw_index(d->dtype, d->w_dtype) + !vec;
  return DXA_OK;
}

int plan_add_layernorm_bwd(const dxa_norm_desc* d, NormPlan* p) {
  if (int rc = check_norm_dtypes(d->dtype, d->w_dtype, "dxa_add_layernorm_bwd")) return rc;
  const int64_t rows = d->rows, cols = d->cols;
  DXA_CHECK_ARG(d->dy && d->x && d->x2 && d->mean && d->rstd && d->dx, "dxa_add_layernorm_bwd: null dy / x / res / mean / rstd / dx");
  DXA_CHECK_ARG(rows >= 0 && cols > 0, "dxa_add_layernorm_bwd: bad sizes (rows %lld, cols %lld)", (long long)rows, (long long)cols);
  DXA_CHECK_ARG(!d->w || d->partial, "dxa_add_layernorm_bwd: partial_dwdb required when w is given");
  if (rows == 0) return DXA_OK;
  const bool vec = al16(d->x) && al16(d->x2) && al16(d->dy) && al16(d->dx) && (!d->w || al16(d->w)) && cols % 4 == 0;
  plan_bwd_grid(p, rows);
  p->vec = vec ? 4 : 1;
  p->k = K_ADDLN_BWD + 2 * tw_index(d->dtype, d->w_dtype) + !vec;
  return DXA_OK;
}

int plan_colsum(const dxa_norm_desc* d, NormPlan* p) {
  const int64_t rows = d->rows, cols = d->cols;
  DXA_CHECK_ARG(d->x && d->y && rows >= 0 && cols > 0 && d->ld >= cols, "dxa_colsum: bad args");
  DXA_CHECK_ARG(d->dtype == DXA_F32 || d->dtype == DXA_BF16, "dxa_colsum: bad dtype");
  // row splits of >= 32 rows, at most 64 of them: the <= 512 partial rows of a norm backward become 16 x 14 workgroups
  int nsplit = (int)((rows + 31) / 32);
  if (nsplit < 1) nsplit = 1;
  if (nsplit > 64) nsplit = 64;
  DXA_CHECK_ARG(d->partial && d->partial_bytes >= (size_t)nsplit * cols * sizeof(float),
                "dxa_colsum: scratch too small (need %zu bytes)", (size_t)nsplit * cols * sizeof(float));
  const size_t es = d->dtype == DXA_BF16 ? 2 : 4;
  const int f32 = d->dtype == DXA_F32;
  p->vec = ((reinterpret_cast<uintptr_t>(d->x) % (4 * es)) == 0) && (d->ld % 4 == 0) ? 4 : 1;
  const unsigned gx = (unsigned)((cols + 255) / 256);
  if (rows <= 32) {
    // a handful of rows: one launch, the block's sums are the result
    p->mode = "direct";
    p->k = K_CS_DIRECT + f32;
    p->nsplit = 1;
  } else if (gx <= COLSUM_CNT && (d->have_counters || !d->capturing)) {
    p->mode = "fused";
    p->k = K_CS_FUSED + f32;
    p->nsplit = nsplit;
  } else {
    p->mode = "two_launch";
    p->k = K_CS_STAGE1 + f32;
    p->nsplit = nsplit;
    p->k2 = K_CS_STAGE2;     // one wave per 64 columns: 56 workgroups for 3584 columns instead of 14
    p->grid2 = dim3((unsigned)((cols + 63) / 64));
    p->block2 = 64;
  }
  p->grid = dim3(gx, (unsigned)p->nsplit);
  p->trips = cdiv(cdiv(rows, p->nsplit), 4);
  return DXA_OK;
}

int plan_downsample(const dxa_norm_desc* d, NormPlan* p, bool bwd) {
  const char* who = bwd ? "dxa_downsample_layernorm_bwd" : "dxa_downsample_layernorm_fwd";
  if (int rc = check_norm_dtypes(d->dtype, d->w_dtype, who)) return rc;
  if (bwd) {
    DXA_CHECK_ARG(d->dy && d->x && d->mean && d->rstd && d->dx, "dxa_downsample_layernorm_bwd: null dy / x / mean / rstd / dx");
    DXA_CHECK_ARG(!d->w || d->partial, "dxa_downsample_layernorm_bwd: partial_dwdb required when w is given");
  } else {
    DXA_CHECK_ARG(d->x && d->y, "dxa_downsample_layernorm_fwd: null x / y");
  }
  const int64_t N = d->rows, G = d->G, C = d->cols;
  if (int rc = check_downsample_args(who, N, G, C)) return rc;
  const int h = (int)((G + 1) / 2);
  const int64_t rows = N * h * h;
  if (rows == 0) return DXA_OK;
  const int vec = d->dtype == DXA_BF16 ? 8 : 4;              // 16 bytes per access
  const bool vec_ok = bwd ? al16(d->x) && al16(d->dy) && al16(d->dx) && (!d->w || al16(d->w)) && C % vec == 0
                          : al16(d->x) && al16(d->y) && (!d->w || al16(d->w)) && (!d->b || al16(d->b)) && C % vec == 0;
  p->vec = vec_ok ? vec : 1;
  p->k = (bwd ? K_DS_BWD : K_DS_FWD) + 2 * tw_index(d->dtype, d->w_dtype) + !vec_ok;
  if (bwd) {
    plan_bwd_grid(p, rows);
    const size_t sums = d->w ? (size_t)8 * C * sizeof(float) : 0;
    p->use_lds = sums > 0 && sums <= DS_LN_MAX_LDS;
    p->lds = p->use_lds ? sums : 0;
  } else {
    p->grid = dim3((unsigned)((rows + 3) / 4));
    p->trips = 1;
  }
  return DXA_OK;
}

int plan_adarms(const dxa_norm_desc* d, NormPlan* p, bool bwd, bool gated_residual) {
  const char* who = gated_residual ? (bwd ? "dxa_gated_residual_bwd" : "dxa_gated_residual_fwd") : (bwd ? "dxa_adarms_bwd" : "dxa_adarms_fwd");
  const int64_t rows = d->rows, cols = d->cols, rps = d->rows_per_sample;
  const int dtype = d->dtype;
  if (int rc = check_adarms(who, rows, rps, cols, dtype)) return rc;
  const void* branch = d->x2;
  if (!gated_residual && !bwd) {
    DXA_CHECK_ARG(d->x && d->mod && d->y, "dxa_adarms_fwd: null x / mod / y");
    DXA_CHECK_ARG(!branch || (d->gate && d->aux && d->gate_ld >= cols), "dxa_adarms_fwd: a branch needs gate_prev, r_out and gate_ld >= cols");
  } else if (gated_residual && !bwd) {
    DXA_CHECK_ARG(d->x && branch && d->gate && d->y && d->gate_ld >= cols, "dxa_gated_residual_fwd: null x / branch / gate / y, or gate_ld < cols");
  } else if (!gated_residual) {
    DXA_CHECK_ARG(d->dy && d->x && d->mod && d->rstd && d->dx && d->dmod && d->partial, "dxa_adarms_bwd: null dy / r / mod / rstd / dr / dmod / partial");
    DXA_CHECK_ARG(!branch || (d->gate && d->aux && d->dgate && d->gate_ld >= cols && d->dgate_ld >= cols),
                  "dxa_adarms_bwd: a branch needs gate_prev, dbranch, dgate_prev and gate_ld, dgate_ld >= cols");
  } else {
    DXA_CHECK_ARG(d->dy && branch && d->gate && d->dx && d->dgate && d->partial, "dxa_gated_residual_bwd: null dy / branch / gate / dbranch / dgate / partial");
    DXA_CHECK_ARG(d->gate_ld >= cols && d->dgate_ld >= cols, "dxa_gated_residual_bwd: gate_ld / dgate_ld < cols");
  }
  if (rows == 0) return DXA_OK;
  if (bwd) {
    const int64_t B = rows / rps;
    const int groups = dxa_adarms_bwd_groups(rps);
    const int ns = gated_residual ? 1 : branch ? 3 : 2;
    const size_t need = (size_t)B * groups * 4 * ns * cols * sizeof(float);
    DXA_CHECK_ARG(d->partial_bytes >= need, "%s: partial too small (need %zu bytes)", who, need);
    p->grid = dim3((unsigned)groups, (unsigned)B);
    p->trips = cdiv(rps, (int64_t)groups * 4);
    p->k2 = K_FOLD + (dtype == DXA_F32);
    p->grid2 = dim3((unsigned)((ns * cols + 255) / 256), (unsigned)B);
  } else {
    p->grid = dim3((unsigned)((rows + 3) / 4));
    p->trips = 1;
  }
  if (gated_residual) {
    p->vec = bwd ? adarms_vec(dtype, cols, d->gate_ld, {d->dy, branch, d->gate, d->dx}) : adarms_vec(dtype, cols, d->gate_ld, {d->x, branch, d->gate, d->y});
    p->k = (bwd ? K_GR_BWD : K_GR_FWD) + adarms_vidx(dtype, p->vec);
  } else if (!bwd) {
    p->vec = adarms_vec(dtype, cols, branch ? d->gate_ld : 0, {d->x, d->mod, d->y, branch, branch ? d->gate : nullptr, branch ? d->aux : nullptr});
    p->k = dtype == DXA_BF16 && p->vec == 8 && cols <= 8192 ? K_AR_FWD_FAST + (branch != nullptr)
                                                            : K_AR_FWD + 2 * adarms_vidx(dtype, p->vec) + (branch != nullptr);
  } else {
    p->vec = adarms_vec(dtype, cols, branch ? d->gate_ld : 0,
                        {d->dy, d->x, d->mod, d->dx, d->residual, branch, branch ? d->gate : nullptr, branch ? d->aux : nullptr});
    p->k = K_AR_BWD + 2 * adarms_vidx(dtype, p->vec) + (branch != nullptr);
  }
  if (p->vec == 2) p->vec = 1;       // a 2-wide fit runs on the scalar kernel (adarms_vidx)
  return DXA_OK;
}

int norm_plan(const dxa_norm_desc* d, NormPlan* p) {
  DXA_CHECK_ARG(d != nullptr, "dxa_norm_plan: null desc");
  switch (d->entry) {
    case DXA_NORM_RMSNORM_FWD: return plan_rmsnorm_fwd(d, p);
    case DXA_NORM_RMSNORM_BWD: return plan_norm_bwd(d, p, false);
    case DXA_NORM_LAYERNORM_FWD: return plan_layernorm_fwd(d, p);
    case DXA_NORM_LAYERNORM_BWD: return plan_norm_bwd(d, p, true);
    case DXA_NORM_ADD_LAYERNORM_FWD: return plan_add_layernorm_fwd(d, p);
    case DXA_NORM_ADD_LAYERNORM_BWD: return plan_add_layernorm_bwd(d, p);
    case DXA_NORM_COLSUM: return plan_colsum(d, p);
    case DXA_NORM_DOWNSAMPLE_FWD: return plan_downsample(d, p, false);
    case DXA_NORM_DOWNSAMPLE_BWD: return plan_downsample(d, p, true);
    case DXA_NORM_ADARMS_FWD: return plan_adarms(d, p, false, false);
    case DXA_NORM_ADARMS_BWD: return plan_adarms(d, p, true, false);
    case DXA_NORM_GATED_RESIDUAL_FWD: return plan_adarms(d, p, false, true);
    case DXA_NORM_GATED_RESIDUAL_BWD: return plan_adarms(d, p, true, true);
  }
  DXA_CHECK_ARG(false, "dxa_norm_plan: unknown entry point %d", d->entry);
  return DXA_ERR_BAD_ARG;
}

// a plan named a kernel its entry point's launcher does not have: cannot happen while the two agree
int unplanned(const char* who, int k) {
  dxa_set_error("%s: no launch for planned kernel %d", who, k);
  return DXA_ERR_UNSUPPORTED;
}
}  // namespace

extern "C" const char* dxa_norm_kernel_name(int i) {
  return i >= 0 && i < (int)K_NONE ? NORM_KERNEL_NAMES[i] : nullptr;
}

extern "C" int dxa_norm_plan(const dxa_norm_desc* d, dxa_norm_plan_info* out) {
  DXA_CHECK_ARG(out != nullptr, "dxa_norm_plan: null output");
  memset(out, 0, sizeof(*out));
  NormPlan p;
  if (int rc = norm_plan(d, &p)) return rc;
  out->kernel = p.k == K_NONE ? nullptr : NORM_KERNEL_NAMES[p.k];
  out->kernel2 = p.k2 == K_NONE || p.k == K_NONE ? nullptr : NORM_KERNEL_NAMES[p.k2];
  out->mode = p.mode;
  out->vec = p.k == K_NONE ? 0 : p.vec;
  out->grid[0] = (int32_t)p.grid.x; out->grid[1] = (int32_t)p.grid.y; out->grid[2] = (int32_t)p.grid.z;
  out->block = p.block;
  out->lds = (int32_t)p.lds;
  out->nsplit = p.nsplit;
  out->trips = p.trips;
  return DXA_OK;
}

namespace {
// bf16 rows of up to 8192 columns (cols % 8 == 0): the wave requests its whole row at once (16 bytes per lane per request, all
// of them in flight together), keeps it in registers for the statistics and the normalisation: ONE read of x, no second pass
template <typename TW>
__global__ __launch_bounds__(256) void rmsnorm_fwd_fast_k(const bf16_t* __restrict__ x, const TW* __restrict__ w,
                                                          bf16_t* __restrict__ y, float* __restrict__ rstd_out, int64_t rows,
                                                          int64_t cols, float eps) {
  constexpr int NIT = 16;
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const bf16_t* xr = x + row * cols;
  u32x4 v[NIT];
  float ss = 0.f;
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int64_t c = ((int64_t)it * 64 + lane) * 8;
    v[it] = c < cols ? *reinterpret_cast<const u32x4*>(xr + c) : (u32x4){0u, 0u, 0u, 0u};
  }
#pragma unroll
  for (int it = 0; it < NIT; ++it)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float a = __uint_as_float(v[it][e] << 16), b = __uint_as_float(v[it][e] & 0xffff0000u);
      ss += a * a + b * b;
    }
  ss = wave_sum(ss);
  const float rstd = rsqrtf(ss / (float)cols + eps);
  if (lane == 0 && rstd_out) rstd_out[row] = rstd;
  bf16_t* yr = y + row * cols;
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int64_t c = ((int64_t)it * 64 + lane) * 8;
    if (c < cols) {
      float g0[4] = {1.f, 1.f, 1.f, 1.f}, g1[4] = {1.f, 1.f, 1.f, 1.f};
      if (w) {
        Vec<TW, 4>::ld(g0, w + c);
        Vec<TW, 4>::ld(g1, w + c + 4);
      }
      const float g[8] = {g0[0], g0[1], g0[2], g0[3], g1[0], g1[1], g1[2], g1[3]};
      u32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float a = __uint_as_float(v[it][e] << 16), b = __uint_as_float(v[it][e] & 0xffff0000u);
        o[e] = pack_bf16x2(g[2 * e] * rnd<bf16_t>(a * rstd), g[2 * e + 1] * rnd<bf16_t>(b * rstd));
      }
      *reinterpret_cast<u32x4*>(yr + c) = o;
    }
  }
}
}  // namespace

extern "C" int dxa_rmsnorm_fwd(const void* x, const void* w, void* y, float* rstd, int64_t rows, int64_t cols,
                               float eps, int dtype, int w_dtype, dxa_stream_t stream) {
  dxa_norm_desc d{};
  d.entry = DXA_NORM_RMSNORM_FWD; d.dtype = dtype; d.w_dtype = w_dtype; d.rows = rows; d.cols = cols;
  d.x = x; d.w = w; d.y = y; d.rstd = rstd;
  NormPlan pl;
  if (int rc = norm_plan(&d, &pl)) return rc;
  if (pl.k == K_NONE) return DXA_OK;
  hipStream_t st = (hipStream_t)stream;
#define RMS_FWD(K_, T_, TW_) hipLaunchKernelGGL(K_, pl.grid, dim3(pl.block), 0, st, (const T_*)x, (const TW_*)w, (T_*)y, rstd, rows, cols, eps)
  switch (pl.k) {
    case K_RMS_FWD_FAST: RMS_FWD((rmsnorm_fwd_fast_k<bf16_t>), bf16_t, bf16_t); break;
    case K_RMS_FWD_FAST_F: RMS_FWD((rmsnorm_fwd_fast_k<float>), bf16_t, float); break;
    case K_RMS_FWD: RMS_FWD((rmsnorm_fwd_k<bf16_t, bf16_t, 4>), bf16_t, bf16_t); break;
    case K_RMS_FWD_1: RMS_FWD((rmsnorm_fwd_k<bf16_t, bf16_t, 1>), bf16_t, bf16_t); break;
    case K_RMS_FWD_BF4: RMS_FWD((rmsnorm_fwd_k<bf16_t, float, 4>), bf16_t, float); break;
    case K_RMS_FWD_BF1: RMS_FWD((rmsnorm_fwd_k<bf16_t, float, 1>), bf16_t, float); break;
    case K_RMS_FWD_FF4: RMS_FWD((rmsnorm_fwd_k<float, float, 4>), float, float); break;
    case K_RMS_FWD_FF1: RMS_FWD((rmsnorm_fwd_k<float, float, 1>), float, float); break;
    default: return unplanned("dxa_rmsnorm_fwd", pl.k);
  }
#undef RMS_FWD
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}

extern "C" int dxa_rmsnorm_bwd(const void* dy, const void* x, const void* w, const float* rstd, void* dx,
                               const void* residual, float* partial_dw, int64_t rows, int64_t cols, int dtype, int w_dtype,
                               dxa_stream_t stream) {
  dxa_norm_desc d{};
  d.entry = DXA_NORM_RMSNORM_BWD; d.dtype = dtype; d.w_dtype = w_dtype; d.rows = rows; d.cols = cols;
  d.dy = dy; d.x = x; d.w = w; d.rstd = rstd; d.dx = dx; d.residual = residual; d.partial = partial_dw;
  NormPlan pl;
  if (int rc = norm_plan(&d, &pl)) return rc;
  if (pl.k == K_NONE) return DXA_OK;
  hipStream_t st = (hipStream_t)stream;
  float* part = w ? partial_dw : nullptr;
  // the fast kernels and the split kernel (dx only without a gain) take no slab without w; rmsnorm_bwd_k decides from w itself
#define RMS_BWD(K_, T_, TW_, P_) hipLaunchKernelGGL(K_, pl.grid, dim3(pl.block), 0, st, (const T_*)dy, (const T_*)x, (const TW_*)w, rstd, (T_*)dx, (const T_*)residual, P_, rows, cols)
#define RMS_FAST(K_, T_, TW_) hipLaunchKernelGGL(K_, pl.grid, dim3(pl.block), 0, st, (const T_*)dy, (const T_*)x, (const TW_*)w, (const float*)nullptr, rstd, (T_*)dx, (const T_*)residual, part, rows, cols)
  switch (pl.k) {
    case K_RMS_SPLIT: RMS_BWD((rmsnorm_bwd_split_k<bf16_t, 4, 4>), bf16_t, bf16_t, part); break;
    case K_RMS_SPLIT_B8: RMS_BWD((rmsnorm_bwd_split_k<bf16_t, 8, 4>), bf16_t, bf16_t, part); break;
    case K_RMS_SPLIT_F4: RMS_BWD((rmsnorm_bwd_split_k<float, 4, 4>), bf16_t, float, part); break;
    case K_RMS_SPLIT_F8: RMS_BWD((rmsnorm_bwd_split_k<float, 8, 4>), bf16_t, float, part); break;
    case K_RMS_FAST8: RMS_FAST((norm_bwd_fast8_k<bf16_t, false>), bf16_t, bf16_t); break;
    case K_RMS_FAST8_F: RMS_FAST((norm_bwd_fast8_k<float, false>), bf16_t, float); break;
    case K_RMS_FAST: RMS_FAST((norm_bwd_fast_k<bf16_t, bf16_t, false>), bf16_t, bf16_t); break;
    case K_RMS_FAST_BF: RMS_FAST((norm_bwd_fast_k<bf16_t, float, false>), bf16_t, float); break;
    case K_RMS_FAST_FF: RMS_FAST((norm_bwd_fast_k<float, float, false>), float, float); break;
    case K_RMS_BWD: RMS_BWD((rmsnorm_bwd_k<bf16_t, bf16_t, 4>), bf16_t, bf16_t, partial_dw); break;
    case K_RMS_BWD_1: RMS_BWD((rmsnorm_bwd_k<bf16_t, bf16_t, 1>), bf16_t, bf16_t, partial_dw); break;
    case K_RMS_BWD_BF4: RMS_BWD((rmsnorm_bwd_k<bf16_t, float, 4>), bf16_t, float, partial_dw); break;
    case K_RMS_BWD_BF1: RMS_BWD((rmsnorm_bwd_k<bf16_t, float, 1>), bf16_t, float, partial_dw); break;
    case K_RMS_BWD_FF4: RMS_BWD((rmsnorm_bwd_k<float, float, 4>), float, float, partial_dw); break;
    case K_RMS_BWD_FF1: RMS_BWD((rmsnorm_bwd_k<float, float, 1>), float, float, partial_dw); break;
    default: return unplanned("dxa_rmsnorm_bwd", pl.k);
  }
#undef RMS_BWD
#undef RMS_FAST
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}

extern "C" int dxa_layernorm_fwd(const void* x, const void* w, const void* b, void* y, float* mean, float* rstd,
                                 int64_t rows, int64_t cols, float eps, int dtype, int w_dtype,
                                 dxa_stream_t stream) {
  dxa_norm_desc d{};
  d.entry = DXA_NORM_LAYERNORM_FWD; d.dtype = dtype; d.w_dtype = w_dtype; d.rows = rows; d.cols = cols;
  d.x = x; d.w = w; d.b = b; d.y = y; d.mean = mean; d.rstd = rstd;
  NormPlan pl;
  if (int rc = norm_plan(&d, &pl)) return rc;
  if (pl.k == K_NONE) return DXA_OK;
  hipStream_t st = (hipStream_t)stream;
#define LN_FWD(K_, T_, TW_) hipLaunchKernelGGL(K_, pl.grid, dim3(pl.block), 0, st, (const T_*)x, (const TW_*)w, (const TW_*)b, (T_*)y, mean, rstd, rows, cols, eps)
  switch (pl.k) {
    case K_LN_FWD: LN_FWD((layernorm_fwd_k<bf16_t, bf16_t, 4>), bf16_t, bf16_t); break;
    case K_LN_FWD_1: LN_FWD((layernorm_fwd_k<bf16_t, bf16_t, 1>), bf16_t, bf16_t); break;
    case K_LN_FWD_BF4: LN_FWD((layernorm_fwd_k<bf16_t, float, 4>), bf16_t, float); break;
    case K_LN_FWD_BF1: LN_FWD((layernorm_fwd_k<bf16_t, float, 1>), bf16_t, float); break;
    case K_LN_FWD_FF4: LN_FWD((layernorm_fwd_k<float, float, 4>), float, float); break;
    case K_LN_FWD_FF1: LN_FWD((layernorm_fwd_k<float, float, 1>), float, float); break;
    default: return unplanned("dxa_layernorm_fwd", pl.k);
  }
#undef LN_FWD
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}

extern "C" int dxa_layernorm_bwd(const void* dy, const void* x, const void* w, const float* mean,
                                 const float* rstd, void* dx, const void* residual, float* partial_dwdb, int64_t rows,
                                 int64_t cols, int dtype, int w_dtype, dxa_stream_t stream) {
  dxa_norm_desc d{};
  d.entry = DXA_NORM_LAYERNORM_BWD; d.dtype = dtype; d.w_dtype = w_dtype; d.rows = rows; d.cols = cols;
  d.dy = dy; d.x = x; d.w = w; d.mean = mean; d.rstd = rstd; d.dx = dx; d.residual = residual; d.partial = partial_dwdb;
  NormPlan pl;
  if (int rc = norm_plan(&d, &pl)) return rc;
  if (pl.k == K_NONE) return DXA_OK;
  hipStream_t st = (hipStream_t)stream;
  float* part = w ? partial_dwdb : nullptr;
#define LN_BWD(K_, T_, TW_) hipLaunchKernelGGL(K_, pl.grid, dim3(pl.block), 0, st, (const T_*)dy, (const T_*)x, (const TW_*)w, mean, rstd, (T_*)dx, (const T_*)residual, part, rows, cols)
  switch (pl.k) {
    case K_LN_FAST: LN_BWD((norm_bwd_fast_k<bf16_t, bf16_t, true>), bf16_t, bf16_t); break;
    case K_LN_FAST_BF: LN_BWD((norm_bwd_fast_k<bf16_t, float, true>), bf16_t, float); break;
    case K_LN_FAST_FF: LN_BWD((norm_bwd_fast_k<float, float, true>), float, float); break;
    case K_LN_BWD: LN_BWD((layernorm_bwd_k<bf16_t, bf16_t, 4>), bf16_t, bf16_t); break;
    case K_LN_BWD_1: LN_BWD((layernorm_bwd_k<bf16_t, bf16_t, 1>), bf16_t, bf16_t); break;
    case K_LN_BWD_BF4: LN_BWD((layernorm_bwd_k<bf16_t, float, 4>), bf16_t, float); break;
    case K_LN_BWD_BF1: LN_BWD((layernorm_bwd_k<bf16_t, float, 1>), bf16_t, float); break;
    case K_LN_BWD_FF4: LN_BWD((layernorm_bwd_k<float, float, 4>), float, float); break;
    case K_LN_BWD_FF1: LN_BWD((layernorm_bwd_k<float, float, 1>), float, float); break;
    default: return unplanned("dxa_layernorm_bwd", pl.k);
  }
#undef LN_BWD
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}

// y = LayerNorm(x + res): layernorm_fwd_k / layernorm_bwd_k with the second addend read beside the first (ADD); the sum exists in
// registers only.  The backward's dx is the gradient of both addends.
extern "C" int dxa_add_layernorm_fwd(const void* x, const void* res, const void* w, const void* b, void* y, float* mean,
                                     float* rstd, int64_t rows, int64_t cols, float eps, int dtype, int w_dtype,
                                     dxa_stream_t stream) {
  dxa_norm_desc d{};
  d.entry = DXA_NORM_ADD_LAYERNORM_FWD; d.dtype = dtype; d.w_dtype = w_dtype; d.rows = rows; d.cols = cols;
  d.x = x; d.x2 = res; d.w = w; d.b = b; d.y = y; d.mean = mean; d.rstd = rstd;
  NormPlan pl;
  if (int rc = norm_plan(&d, &pl)) return rc;
  if (pl.k == K_NONE) return DXA_OK;
  hipStream_t st = (hipStream_t)stream;
#define ADD_LN_FWD(T_, TW_, V_) hipLaunchKernelGGL((layernorm_fwd_k<T_, TW_, V_, true>), pl.grid, dim3(pl.block), 0, st, (const T_*)x, (const TW_*)w, (const TW_*)b, (T_*)y, mean, rstd, rows, cols, eps, (const T_*)res)
  switch (pl.k) {
    case K_ADDLN_FWD: ADD_LN_FWD(bf16_t, bf16_t, 4); break;
    case K_ADDLN_FWD_1: ADD_LN_FWD(bf16_t, bf16_t, 1); break;
    case K_ADDLN_FWD_BF4: ADD_LN_FWD(bf16_t, float, 4); break;
    case K_ADDLN_FWD_BF1: ADD_LN_FWD(bf16_t, float, 1); break;
    case K_ADDLN_FWD_FF4: ADD_LN_FWD(float, float, 4); break;
    case K_ADDLN_FWD_FF1: ADD_LN_FWD(float, float, 1); break;
    default: return unplanned("dxa_add_layernorm_fwd", pl.k);
  }
#undef ADD_LN_FWD
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}

extern "C" int dxa_add_layernorm_bwd(const void* dy, const void* x, const void* res, const void* w, const float* mean,
                                     const float* rstd, void* dx, float* partial_dwdb, int64_t rows, int64_t cols, int dtype,
                                     int w_dtype, dxa_stream_t stream) {
  dxa_norm_desc d{};
  d.entry = DXA_NORM_ADD_LAYERNORM_BWD; d.dtype = dtype; d.w_dtype = w_dtype; d.rows = rows; d.cols = cols;
  d.dy = dy; d.x = x; d.x2 = res; d.w = w; d.mean = mean; d.rstd = rstd; d.dx = dx; d.partial = partial_dwdb;
  NormPlan pl;
  if (int rc = norm_plan(&d, &pl)) return rc;
  if (pl.k == K_NONE) return DXA_OK;
  hipStream_t st = (hipStream_t)stream;
  float* part = w ? partial_dwdb : nullptr;
#define ADD_LN_BWD(T_, TW_, V_) hipLaunchKernelGGL((layernorm_bwd_k<T_, TW_, V_, true>), pl.grid, dim3(pl.block), 0, st, (const T_*)dy, (const T_*)x, (const TW_*)w, mean, rstd, (T_*)dx, (const T_*)nullptr, part, rows, cols, (const T_*)res)
  switch (pl.k) {
    case K_ADDLN_BWD: ADD_LN_BWD(bf16_t, bf16_t, 4); break;
    case K_ADDLN_BWD_1: ADD_LN_BWD(bf16_t, bf16_t, 1); break;
    case K_ADDLN_BWD_BF4: ADD_LN_BWD(bf16_t, float, 4); break;
    case K_ADDLN_BWD_BF1: ADD_LN_BWD(bf16_t, float, 1); break;
    case K_ADDLN_BWD_FF4: ADD_LN_BWD(float, float, 4); break;
    case K_ADDLN_BWD_FF1: ADD_LN_BWD(float, float, 1); break;
    default: return unplanned("dxa_add_layernorm_bwd", pl.k);
  }
#undef ADD_LN_BWD
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}

namespace {
StreamBlock colsum_counters(COLSUM_CNT * sizeof(int));
}  // namespace

extern "C" int dxa_colsum(const void* x, int64_t ld, float* out, int64_t rows, int64_t cols, int dtype,
                          int accumulate, float* scratch, size_t scratch_bytes, dxa_stream_t stream) {
  dxa_norm_desc d{};
  d.entry = DXA_NORM_COLSUM; d.dtype = dtype; d.rows = rows; d.cols = cols; d.ld = ld; d.accumulate = accumulate;
  d.x = x; d.y = out; d.partial = scratch; d.partial_bytes = scratch_bytes;
  d.have_counters = 1;                     // planned as if they existed; their absence is learnt below, where it can be
  NormPlan pl;
  if (int rc = norm_plan(&d, &pl)) return rc;
  hipStream_t st = (hipStream_t)stream;
  int* cnt = nullptr;
  if (pl.k == K_CS_FUSED || pl.k == K_CS_FUSED_F) {
    if (int rc = colsum_counters.get(st, &cnt)) return rc;
    if (cnt == nullptr) {                  // not allocated yet and the stream is capturing
      d.have_counters = 0;
      d.capturing = 1;
      if (int rc = norm_plan(&d, &pl)) return rc;
    }
  }
  const int vec = pl.vec == 4;
  switch (pl.k) {
    case K_CS_DIRECT: hipLaunchKernelGGL((colsum_stage1_k<bf16_t, true>), pl.grid, dim3(pl.block), 0, st, (const bf16_t*)x, ld, out, rows, cols, vec, accumulate); break;
    case K_CS_DIRECT_F: hipLaunchKernelGGL((colsum_stage1_k<float, true>), pl.grid, dim3(pl.block), 0, st, (const float*)x, ld, out, rows, cols, vec, accumulate); break;
    case K_CS_FUSED: hipLaunchKernelGGL((colsum_fused_k<bf16_t>), pl.grid, dim3(pl.block), 0, st, (const bf16_t*)x, ld, scratch, out, rows, cols, vec, accumulate, cnt); break;
    case K_CS_FUSED_F: hipLaunchKernelGGL((colsum_fused_k<float>), pl.grid, dim3(pl.block), 0, st, (const float*)x, ld, scratch, out, rows, cols, vec, accumulate, cnt); break;
    case K_CS_STAGE1: hipLaunchKernelGGL((colsum_stage1_k<bf16_t>), pl.grid, dim3(pl.block), 0, st, (const bf16_t*)x, ld, scratch, rows, cols, vec); break;
    case K_CS_STAGE1_F: hipLaunchKernelGGL((colsum_stage1_k<float>), pl.grid, dim3(pl.block), 0, st, (const float*)x, ld, scratch, rows, cols, vec); break;
    default: return unplanned("dxa_colsum", pl.k);
  }
  if (pl.k2 == K_CS_STAGE2)
    hipLaunchKernelGGL(colsum_stage2_k, pl.grid2, dim3(pl.block2), 0, st, scratch, out, pl.nsplit, cols, accumulate);
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}

// ------------------------------------------------------------------------ 2x2 token merge + LayerNorm
// The `mlp_downsample` projector's DownSampleBlock + nn.LayerNorm(4C) (see include/dexbotic_amd.h): one wavefront owns one
// OUTPUT row, whose four quarters are contiguous runs of C elements of the un-merged input (or zeros, where an odd grid was
// padded).  Structure and statistics of layernorm_fwd_k / layernorm_bwd_k; the merged tensor never exists in memory.
namespace {

template <typename TW, int VEC>
__device__ __forceinline__ void ld_w(float (&o)[VEC], const TW* p) {
  if constexpr (VEC == 8 && sizeof(TW) == 4) {
    float a[4], b[4];
    Vec<float, 4>::ld(a, reinterpret_cast<const float*>(p));
    Vec<float, 4>::ld(b, reinterpret_cast<const float*>(p) + 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) { o[i] = a[i]; o[4 + i] = b[i]; }
  } else {
    Vec<TW, VEC>::ld(o, p);
  }
}

// offset (elements) of quarter q of output row `row` in the un-merged input, or -1 where the quarter is padding
__device__ __forceinline__ int64_t ds_quarter(int64_t row, int q, int G, int h, int C) {
  const int64_t n = row / ((int64_t)h * h);
  const int o = (int)(row - n * h * h);
  const int j = o / h, i = o - j * h;                    // o = j * h + i: column pair major
  const int r = 2 * i + (q >> 1), c = 2 * j + (q & 1);
  return (r < G && c < G) ? ((n * G + r) * G + c) * (int64_t)C : -1;
}

template <typename T, typename TW, int VEC>
__global__ __launch_bounds__(256) void ds_layernorm_fwd_k(const T* __restrict__ x, const TW* __restrict__ w,
                                                          const TW* __restrict__ b, T* __restrict__ y,
                                                          float* __restrict__ mean_out, float* __restrict__ rstd_out,
                                                          int64_t rows, int G, int h, int C, float eps) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int64_t cols = 4 * (int64_t)C;
  int64_t off[4];
  int npad = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) { off[q] = ds_quarter(row, q, G, h, C); npad += off[q] < 0; }
  float s = 0.f;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (off[q] < 0) continue;
    const T* xq = x + off[q];
    for (int k = lane * VEC; k < C; k += 64 * VEC) {
      float v[VEC];
      Vec<T, VEC>::ld(v, xq + k);
#pragma unroll
      for (int i = 0; i < VEC; ++i) s += v[i];
    }
  }
  const float mean = wave_sum(s) / (float)cols;
  float ss = 0.f;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (off[q] < 0) continue;
    const T* xq = x + off[q];
    for (int k = lane * VEC; k < C; k += 64 * VEC) {
      float v[VEC];
      Vec<T, VEC>::ld(v, xq + k);
#pragma unroll
      for (int i = 0; i < VEC; ++i) { const float d = v[i] - mean; ss += d * d; }
    }
  }
  // the padded quarters are zeros: C elements at distance `mean` each
  const float rstd = rsqrtf((wave_sum(ss) + (float)npad * (float)C * mean * mean) / (float)cols + eps);
  if (lane == 0) {
    if (mean_out) mean_out[row] = mean;
    if (rstd_out) rstd_out[row] = rstd;
  }
  T* yr = y + row * cols;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const T* xq = off[q] < 0 ? nullptr : x + off[q];
    for (int k = lane * VEC; k < C; k += 64 * VEC) {
      float v[VEC], g[VEC], bb[VEC];
      if (xq) {
        Vec<T, VEC>::ld(v, xq + k);
      } else {
#pragma unroll
        for (int i = 0; i < VEC; ++i) v[i] = 0.f;
      }
      if (w) ld_w<TW, VEC>(g, w + q * C + k);
      if (b) ld_w<TW, VEC>(bb, b + q * C + k);
#pragma unroll
      for (int i = 0; i < VEC; ++i) v[i] = (v[i] - mean) * rstd * (w ? g[i] : 1.f) + (b ? bb[i] : 0.f);
      Vec<T, VEC>::st(yr + q * C + k, v);
    }
  }
}

// partial: [gridDim.x][2*cols] = (dw | db), cols = 4C.  A wave computes the row statistics and dx of its output row; then the
// 256 threads of the workgroup, each owning fixed columns, add the (up to) four rows of the pass to the workgroup's partial sums
// in row order: deterministic, no atomics, no wave waits for another.  The sums live in LDS (`use_lds`: 2*cols floats of dynamic
// LDS) and are written out once at the end, or directly in the workgroup's slab of `partial` for rows too wide for LDS.
template <typename T, typename TW, int VEC>
__global__ __launch_bounds__(256) void ds_layernorm_bwd_k(const T* __restrict__ dy, const T* __restrict__ x,
                                                          const TW* __restrict__ w, const float* __restrict__ mean,
                                                          const float* __restrict__ rstd, T* __restrict__ dx,
                                                          float* __restrict__ partial, int64_t rows, int G, int h, int C,
                                                          int use_lds) {
  extern __shared__ float ds_sums[];
  __shared__ float st_mu[4], st_rs[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t cols = 4 * (int64_t)C;
  float* slab = partial ? partial + (int64_t)blockIdx.x * 2 * cols : nullptr;
  float* acc = slab ? (use_lds ? ds_sums : slab) : nullptr;
  if (acc) {
    for (int64_t c = threadIdx.x; c < 2 * cols; c += 256) acc[c] = 0.f;
    __syncthreads();
  }
  for (int64_t base = (int64_t)blockIdx.x * 4; base < rows; base += (int64_t)gridDim.x * 4) {
    const int64_t row = base + wave;
    float rs = 0.f, mu = 0.f;
    if (row < rows) {
      rs = rstd[row];
      mu = mean[row];
      int64_t off[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) off[q] = ds_quarter(row, q, G, h, C);
      const T* gr = dy + row * cols;
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const T* xq = off[q] < 0 ? nullptr : x + off[q];
        for (int k = lane * VEC; k < C; k += 64 * VEC) {
          float xv[VEC], gv[VEC], wv[VEC];
          if (xq) {
            Vec<T, VEC>::ld(xv, xq + k);
          } else {
#pragma unroll
            for (int i = 0; i < VEC; ++i) xv[i] = 0.f;
          }
          Vec<T, VEC>::ld(gv, gr + q * C + k);
          if (w) ld_w<TW, VEC>(wv, w + q * C + k);
#pragma unroll
          for (int i = 0; i < VEC; ++i) {
            const float g = gv[i] * (w ? wv[i] : 1.f);
            s1 += g;
            s2 += g * ((xv[i] - mu) * rs);
          }
        }
      }
      const float c1 = wave_sum(s1) / (float)cols, c2 = wave_sum(s2) / (float)cols;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (off[q] < 0) continue;                          // padding has no input element to receive a gradient
        const T* xq = x + off[q];
        T* dxq = dx + off[q];
        for (int k = lane * VEC; k < C; k += 64 * VEC) {
          float xv[VEC], gv[VEC], wv[VEC], o[VEC];
          Vec<T, VEC>::ld(xv, xq + k);
          Vec<T, VEC>::ld(gv, gr + q * C + k);
          if (w) ld_w<TW, VEC>(wv, w + q * C + k);
#pragma unroll
          for (int i = 0; i < VEC; ++i) {
            const float g = gv[i] * (w ? wv[i] : 1.f);
            o[i] = rs * (g - c1 - (xv[i] - mu) * rs * c2);
          }
          Vec<T, VEC>::st(dxq + k, o);
        }
      }
    }
    if (acc) {
      if (lane == 0) { st_mu[wave] = mu; st_rs[wave] = rs; }
      __syncthreads();
      const int nslot = (int)min((int64_t)4, rows - base);
      for (int64_t c = (int64_t)threadIdx.x * VEC; c < cols; c += 256 * VEC) {
        const int q = (int)(c / C), k = (int)(c - (int64_t)q * C);      // C % VEC == 0: a chunk never straddles two quarters
        float aw[VEC], ab[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) { aw[i] = acc[c + i]; ab[i] = acc[cols + c + i]; }
        for (int sl = 0; sl < nslot; ++sl) {
          const int64_t r2 = base + sl;
          const int64_t o2 = ds_quarter(r2, q, G, h, C);
          const float mu2 = st_mu[sl], rs2 = st_rs[sl];
          float xv[VEC], gv[VEC];
          if (o2 >= 0) {
            Vec<T, VEC>::ld(xv, x + o2 + k);
          } else {
#pragma unroll
            for (int i = 0; i < VEC; ++i) xv[i] = 0.f;
          }
          Vec<T, VEC>::ld(gv, dy + r2 * cols + c);
#pragma unroll
          for (int i = 0; i < VEC; ++i) {
            aw[i] += gv[i] * ((xv[i] - mu2) * rs2);
            ab[i] += gv[i];
          }
        }
#pragma unroll
        for (int i = 0; i < VEC; ++i) { acc[c + i] = aw[i]; acc[cols + c + i] = ab[i]; }
      }
      __syncthreads();
    }
  }
  if (acc && use_lds)
    for (int64_t c = threadIdx.x; c < 2 * cols; c += 256) slab[c] = ds_sums[c];
}

}  // namespace

extern "C" int dxa_downsample_layernorm_fwd(const void* x, const void* w, const void* b, void* y, float* mean, float* rstd,
                                            int64_t N, int64_t G, int64_t C, float eps, int dtype, int w_dtype,
                                            dxa_stream_t stream) {
  dxa_norm_desc d{};
  d.entry = DXA_NORM_DOWNSAMPLE_FWD; d.dtype = dtype; d.w_dtype = w_dtype; d.rows = N; d.G = G; d.cols = C;
  d.x = x; d.w = w; d.b = b; d.y = y; d.mean = mean; d.rstd = rstd;
  NormPlan pl;
  if (int rc = norm_plan(&d, &pl)) return rc;
  if (pl.k == K_NONE) return DXA_OK;
  const int h = (int)((G + 1) / 2);
  const int64_t rows = N * h * h;
  hipStream_t st = (hipStream_t)stream;
#define DS_FWD(T_, TW_, V_) hipLaunchKernelGGL((ds_layernorm_fwd_k<T_, TW_, V_>), pl.grid, dim3(pl.block), 0, st, (const T_*)x, (const TW_*)w, (const TW_*)b, (T_*)y, mean, rstd, rows, (int)G, h, (int)C, eps)
  switch (pl.k) {
    case K_DS_FWD: DS_FWD(bf16_t, bf16_t, 8); break;
    case K_DS_FWD_1: DS_FWD(bf16_t, bf16_t, 1); break;
    case K_DS_FWD_BF8: DS_FWD(bf16_t, float, 8); break;
    case K_DS_FWD_BF1: DS_FWD(bf16_t, float, 1); break;
    case K_DS_FWD_FF4: DS_FWD(float, float, 4); break;
    case K_DS_FWD_FF1: DS_FWD(float, float, 1); break;
    default: return unplanned("dxa_downsample_layernorm_fwd", pl.k);
  }
#undef DS_FWD
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}

extern "C" int dxa_downsample_layernorm_bwd(const void* dy, const void* x, const void* w, const float* mean,
                                            const float* rstd, void* dx, float* partial_dwdb, int64_t N, int64_t G,
                                            int64_t C, int dtype, int w_dtype, dxa_stream_t stream) {
  dxa_norm_desc d{};
  d.entry = DXA_NORM_DOWNSAMPLE_BWD; d.dtype = dtype; d.w_dtype = w_dtype; d.rows = N; d.G = G; d.cols = C;
  d.dy = dy; d.x = x; d.w = w; d.mean = mean; d.rstd = rstd; d.dx = dx; d.partial = partial_dwdb;
  NormPlan pl;
  if (int rc = norm_plan(&d, &pl)) return rc;
  if (pl.k == K_NONE) return DXA_OK;
  const int h = (int)((G + 1) / 2);
  const int64_t rows = N * h * h;
  hipStream_t st = (hipStream_t)stream;
  float* part = w ? partial_dwdb : nullptr;
#define DS_BWD(T_, TW_, V_) hipLaunchKernelGGL((ds_layernorm_bwd_k<T_, TW_, V_>), pl.grid, dim3(pl.block), pl.lds, st, (const T_*)dy, (const T_*)x, (const TW_*)w, mean, rstd, (T_*)dx, part, rows, (int)G, h, (int)C, pl.use_lds)
  switch (pl.k) {
    case K_DS_BWD: DS_BWD(bf16_t, bf16_t, 8); break;
    case K_DS_BWD_1: DS_BWD(bf16_t, bf16_t, 1); break;
    case K_DS_BWD_BF8: DS_BWD(bf16_t, float, 8); break;
    case K_DS_BWD_BF1: DS_BWD(bf16_t, float, 1); break;
    case K_DS_BWD_FF4: DS_BWD(float, float, 4); break;
    case K_DS_BWD_FF1: DS_BWD(float, float, 1); break;
    default: return unplanned("dxa_downsample_layernorm_bwd", pl.k);
  }
#undef DS_BWD
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}

// ------------------------------------------------------------------- adaptive RMSNorm + gated residual (pi0.5)
// The action expert of pi0.5 (pi05_arch.py:118-250, transformers_pi05/gemma/modeling_gemma.py:38-120) has no norm gains: every
// norm is modulated PER SAMPLE by mod [B, 3 * cols] = [scale | shift | gate] (a dense layer of the flow-time embedding), and both
// residual adds of a layer are gated.  Sample s = row / rows_per_sample, taken per ROW: a workgroup's four rows may lie in two
// samples.  All arithmetic fp32, every output rounded once.
//   forward    r = x + branch * gate_prev[s]   (optional; r is written: the next add and the backward read it)
//              y = r * rsqrt(mean(r^2) + eps) * (1 + scale[s]) + shift[s]
//   backward   g = dy * (1 + scale[s]);  dr = rstd * (g - xh * mean(g * xh)) (+ residual);  dbranch = dr * gate_prev[s]
//              dscale[s] = sum_rows dy * xh,  dshift[s] = sum_rows dy,  dgate_prev[s] = sum_rows dr * branch
// The per-sample sums are deterministic: a wave adds its rows into a partial row of its own (grid = (row groups, samples), a row
// group = 4 waves), adarms_fold_k adds a sample's partial rows in a fixed order.  No atomics.
namespace {

template <typename T, int VEC, bool GATED>
__global__ __launch_bounds__(256) void adarms_fwd_k(const T* __restrict__ x, const T* __restrict__ branch,
                                                    const T* __restrict__ gate, int64_t gate_ld, const T* __restrict__ mod,
                                                    T* __restrict__ r_out, T* __restrict__ y, float* __restrict__ rstd_out,
                                                    int64_t rows, int64_t rps, int64_t cols, float eps) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int64_t s = row / rps;
  const T* xr = x + row * cols;
  const T* br = GATED ? branch + row * cols : nullptr;
  const T* gt = GATED ? gate + s * gate_ld : nullptr;
  // the row that is normalised: x, or the gated sum rounded to the storage type (what r_out holds and the backward reads)
  auto ld_r = [&](float (&v)[VEC], int64_t c) {
    Vec<T, VEC>::ld(v, xr + c);
    if constexpr (GATED) {
      float b[VEC], g[VEC];
      Vec<T, VEC>::ld(b, br + c);
      Vec<T, VEC>::ld(g, gt + c);
#pragma unroll
      for (int i = 0; i < VEC; ++i) v[i] = rnd<T>(__builtin_fmaf(b[i], g[i], v[i]));
    }
  };
  float ss = 0.f;
  for (int64_t c = (int64_t)lane * VEC; c < cols; c += 64 * VEC) {
    float v[VEC];
    ld_r(v, c);
    if constexpr (GATED) Vec<T, VEC>::st(r_out + row * cols + c, v);
#pragma unroll
    for (int i = 0; i < VEC; ++i) ss += v[i] * v[i];
  }
  const float rstd = rsqrtf(wave_sum(ss) / (float)cols + eps);
  if (lane == 0 && rstd_out) rstd_out[row] = rstd;
  const T* sc = mod + s * 3 * cols;
  const T* sh = sc + cols;
  T* yr = y + row * cols;
  for (int64_t c = (int64_t)lane * VEC; c < cols; c += 64 * VEC) {
    float v[VEC], a[VEC], b[VEC];
    ld_r(v, c);
    Vec<T, VEC>::ld(a, sc + c);
    Vec<T, VEC>::ld(b, sh + c);
#pragma unroll
    for (int i = 0; i < VEC; ++i) v[i] = v[i] * rstd * (1.f + a[i]) + b[i];
    Vec<T, VEC>::st(yr + c, v);
  }
}

// bf16 rows of up to 8192 columns (cols % 8 == 0), as rmsnorm_fwd_fast_k: the wave requests its whole row at once and keeps it in
// registers — x and branch are read ONCE, the gated sum is formed, written and normalised from the same registers
template <bool GATED>
__global__ __launch_bounds__(256) void adarms_fwd_fast_k(const bf16_t* __restrict__ x, const bf16_t* __restrict__ branch,
                                                         const bf16_t* __restrict__ gate, int64_t gate_ld,
                                                         const bf16_t* __restrict__ mod, bf16_t* __restrict__ r_out,
                                                         bf16_t* __restrict__ y, float* __restrict__ rstd_out, int64_t rows,
                                                         int64_t rps, int64_t cols, float eps) {
  constexpr int NIT = 16;
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int64_t s = row / rps;
  const bf16_t* xr = x + row * cols;
  auto unpack = [](const u32x4& v, float (&o)[8]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) { o[2 * e] = __uint_as_float(v[e] << 16); o[2 * e + 1] = __uint_as_float(v[e] & 0xffff0000u); }
  };
  u32x4 v[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int64_t c = ((int64_t)it * 64 + lane) * 8;
    v[it] = c < cols ? *reinterpret_cast<const u32x4*>(xr + c) : (u32x4){0u, 0u, 0u, 0u};
  }
  if constexpr (GATED) {
    const bf16_t* br = branch + row * cols;
    const bf16_t* gt = gate + s * gate_ld;
    bf16_t* ro = r_out + row * cols;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int64_t c = ((int64_t)it * 64 + lane) * 8;
      if (c < cols) {
        float xf[8], bf[8], gf[8];
        unpack(v[it], xf);
        Vec<bf16_t, 8>::ld(bf, br + c);
        Vec<bf16_t, 8>::ld(gf, gt + c);
#pragma unroll
        for (int e = 0; e < 4; ++e)
          v[it][e] = pack_bf16x2(__builtin_fmaf(bf[2 * e], gf[2 * e], xf[2 * e]), __builtin_fmaf(bf[2 * e + 1], gf[2 * e + 1], xf[2 * e + 1]));
        *reinterpret_cast<u32x4*>(ro + c) = v[it];
      }
    }
  }
  float ss = 0.f;
#pragma unroll
  for (int it = 0; it < NIT; ++it)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float a = __uint_as_float(v[it][e] << 16), b = __uint_as_float(v[it][e] & 0xffff0000u);
      ss += a * a + b * b;
    }
  const float rstd = rsqrtf(wave_sum(ss) / (float)cols + eps);
  if (lane == 0 && rstd_out) rstd_out[row] = rstd;
  const bf16_t* sc = mod + s * 3 * cols;
  const bf16_t* sh = sc + cols;
  bf16_t* yr = y + row * cols;
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int64_t c = ((int64_t)it * 64 + lane) * 8;
    if (c < cols) {
      float rf[8], a[8], b[8];
      unpack(v[it], rf);
      Vec<bf16_t, 8>::ld(a, sc + c);
      Vec<bf16_t, 8>::ld(b, sh + c);
      u32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        o[e] = pack_bf16x2(rf[2 * e] * rstd * (1.f + a[2 * e]) + b[2 * e], rf[2 * e + 1] * rstd * (1.f + a[2 * e + 1]) + b[2 * e + 1]);
      *reinterpret_cast<u32x4*>(yr + c) = o;
    }
  }
}

// y = x + branch * gate[s]: the add that ends a layer (the norm that follows belongs to the next layer's autograd node)
template <typename T, int VEC>
__global__ __launch_bounds__(256) void gated_residual_fwd_k(const T* __restrict__ x, const T* __restrict__ branch,
                                                            const T* __restrict__ gate, int64_t gate_ld, T* __restrict__ y,
                                                            int64_t rows, int64_t rps, int64_t cols) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const T* gt = gate + (row / rps) * gate_ld;
  for (int64_t c = (int64_t)lane * VEC; c < cols; c += 64 * VEC) {
    float v[VEC], b[VEC], g[VEC];
    Vec<T, VEC>::ld(v, x + row * cols + c);
    Vec<T, VEC>::ld(b, branch + row * cols + c);
    Vec<T, VEC>::ld(g, gt + c);
#pragma unroll
    for (int i = 0; i < VEC; ++i) v[i] = __builtin_fmaf(b[i], g[i], v[i]);
    Vec<T, VEC>::st(y + row * cols + c, v);
  }
}

// grid (row groups, samples).  Wave w of row group b owns rows b * 4 + w, + 4 * gridDim.x, ... of its sample and partial row
// (sample * gridDim.x + b) * 4 + w of `partial` [..][NS * cols] = (dscale | dshift | dgate_prev): written on the wave's first row,
// added to on the following ones (or zeroed, for a wave without a row) — every element by the one lane that owns its column.
template <typename T, int VEC, bool GATED>
__global__ __launch_bounds__(256) void adarms_bwd_k(const T* __restrict__ dy, const T* __restrict__ r, const T* __restrict__ mod,
                                                    const float* __restrict__ rstd, const T* __restrict__ res, T* __restrict__ dr,
                                                    const T* __restrict__ branch, const T* __restrict__ gate, int64_t gate_ld,
                                                    T* __restrict__ dbranch, float* __restrict__ partial, int64_t rps,
                                                    int64_t cols) {
  constexpr int NS = GATED ? 3 : 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t s = blockIdx.y;
  float* slab = partial + ((s * gridDim.x + blockIdx.x) * 4 + wave) * NS * cols;
  const T* sc = mod + s * 3 * cols;
  const T* gt = GATED ? gate + s * gate_ld : nullptr;
  bool first = true;
  for (int64_t i = (int64_t)blockIdx.x * 4 + wave; i < rps; i += (int64_t)gridDim.x * 4) {
    const int64_t off = (s * rps + i) * cols;
    const float rs = rstd[s * rps + i];
    float s2 = 0.f;
    for (int64_t c = (int64_t)lane * VEC; c < cols; c += 64 * VEC) {
      float xv[VEC], gv[VEC], a[VEC];
      Vec<T, VEC>::ld(xv, r + off + c);
      Vec<T, VEC>::ld(gv, dy + off + c);
      Vec<T, VEC>::ld(a, sc + c);
#pragma unroll
      for (int k = 0; k < VEC; ++k) s2 += gv[k] * (1.f + a[k]) * (xv[k] * rs);
    }
    const float c2 = wave_sum(s2) / (float)cols;
    for (int64_t c = (int64_t)lane * VEC; c < cols; c += 64 * VEC) {
      float xv[VEC], gv[VEC], a[VEC], o[VEC];
      Vec<T, VEC>::ld(xv, r + off + c);
      Vec<T, VEC>::ld(gv, dy + off + c);
      Vec<T, VEC>::ld(a, sc + c);
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const float xh = xv[k] * rs;
        o[k] = rs * (gv[k] * (1.f + a[k]) - xh * c2);
        xv[k] = gv[k] * xh;                                  // this row's share of dscale
      }
      if (res) {
        float rv[VEC];
        Vec<T, VEC>::ld(rv, res + off + c);
#pragma unroll
        for (int k = 0; k < VEC; ++k) o[k] += rv[k];
      }
      Vec<T, VEC>::st(dr + off + c, o);
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        slab[c + k] = first ? xv[k] : slab[c + k] + xv[k];
        slab[cols + c + k] = first ? gv[k] : slab[cols + c + k] + gv[k];
      }
      if constexpr (GATED) {
        float bv[VEC], g[VEC], ob[VEC];
        Vec<T, VEC>::ld(bv, branch + off + c);
        Vec<T, VEC>::ld(g, gt + c);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          ob[k] = o[k] * g[k];
          const float t = o[k] * bv[k];
          slab[2 * cols + c + k] = first ? t : slab[2 * cols + c + k] + t;
        }
        Vec<T, VEC>::st(dbranch + off + c, ob);
      }
    }
    first = false;
  }
  if (first)
    for (int64_t c = lane; c < NS * cols; c += 64) slab[c] = 0.f;
}

// backward of gated_residual_fwd_k, same grid and partial rows ([..][cols] = dgate): dbranch = dy * gate[s], dgate[s] = sum dy * branch
template <typename T, int VEC>
__global__ __launch_bounds__(256) void gated_residual_bwd_k(const T* __restrict__ dy, const T* __restrict__ branch,
                                                            const T* __restrict__ gate, int64_t gate_ld, T* __restrict__ dbranch,
                                                            float* __restrict__ partial, int64_t rps, int64_t cols) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t s = blockIdx.y;
  float* slab = partial + ((s * gridDim.x + blockIdx.x) * 4 + wave) * cols;
  const T* gt = gate + s * gate_ld;
  bool first = true;
  for (int64_t i = (int64_t)blockIdx.x * 4 + wave; i < rps; i += (int64_t)gridDim.x * 4) {
    const int64_t off = (s * rps + i) * cols;
    for (int64_t c = (int64_t)lane * VEC; c < cols; c += 64 * VEC) {
      float gv[VEC], bv[VEC], g[VEC], ob[VEC];
      Vec<T, VEC>::ld(gv, dy + off + c);
      Vec<T, VEC>::ld(bv, branch + off + c);
      Vec<T, VEC>::ld(g, gt + c);
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        ob[k] = gv[k] * g[k];
        const float t = gv[k] * bv[k];
        slab[c + k] = first ? t : slab[c + k] + t;
      }
      Vec<T, VEC>::st(dbranch + off + c, ob);
    }
    first = false;
  }
  if (first)
    for (int64_t c = lane; c < cols; c += 64) slab[c] = 0.f;
}

// a sample's `nrow` partial rows [n] added in row order (eight loads in flight), rounded once: columns [0, n_a) go to out_a
// (row stride ld_a), the rest to out_b (row stride ld_b) — the gate belongs to ANOTHER modulation tensor than scale and shift
template <typename T>
__global__ __launch_bounds__(256) void adarms_fold_k(const float* __restrict__ partial, int nrow, int64_t n, T* __restrict__ out_a,
                                                     int64_t ld_a, int64_t n_a, T* __restrict__ out_b, int64_t ld_b) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t s = blockIdx.y;
  if (j >= n) return;
  const float* p = partial + s * nrow * n + j;
  float acc = 0.f;
  int i = 0;
  for (; i + 8 <= nrow; i += 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = p[(int64_t)(i + u) * n];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc += v[u];
  }
  for (; i < nrow; ++i) acc += p[(int64_t)i * n];
  if (j < n_a) stf<T>(out_a + s * ld_a + j, acc);
  else stf<T>(out_b + s * ld_b + (j - n_a), acc);
}

}  // namespace

extern "C" int dxa_adarms_fwd(const void* x, const void* branch, const void* gate_prev, int64_t gate_ld, const void* mod,
                              void* r_out, void* y, float* rstd, int64_t rows, int64_t rows_per_sample, int64_t cols, float eps,
                              int dtype, dxa_stream_t stream) {
  dxa_norm_desc d{};
  d.entry = DXA_NORM_ADARMS_FWD; d.dtype = dtype; d.rows = rows; d.rows_per_sample = rows_per_sample; d.cols = cols; d.gate_ld = gate_ld;
  d.x = x; d.x2 = branch; d.gate = gate_prev; d.mod = mod; d.aux = r_out; d.y = y; d.rstd = rstd;
  NormPlan pl;
  if (int rc = norm_plan(&d, &pl)) return rc;
  if (pl.k == K_NONE) return DXA_OK;
  hipStream_t st = (hipStream_t)stream;
#define ADARMS_FWD_G(K_, T_) hipLaunchKernelGGL(K_, pl.grid, dim3(pl.block), 0, st, (const T_*)x, (const T_*)branch, (const T_*)gate_prev, gate_ld, (const T_*)mod, (T_*)r_out, (T_*)y, rstd, rows, rows_per_sample, cols, eps)
#define ADARMS_FWD(K_, T_) hipLaunchKernelGGL(K_, pl.grid, dim3(pl.block), 0, st, (const T_*)x, (const T_*)nullptr, (const T_*)nullptr, (int64_t)0, (const T_*)mod, (T_*)nullptr, (T_*)y, rstd, rows, rows_per_sample, cols, eps)
  switch (pl.k) {
    case K_AR_FWD_FAST: ADARMS_FWD((adarms_fwd_fast_k<false>), bf16_t); break;
    case K_AR_FWD_FAST_G: ADARMS_FWD_G((adarms_fwd_fast_k<true>), bf16_t); break;
    case K_AR_FWD: ADARMS_FWD((adarms_fwd_k<bf16_t, 8, false>), bf16_t); break;
    case K_AR_FWD_B8G: ADARMS_FWD_G((adarms_fwd_k<bf16_t, 8, true>), bf16_t); break;
    case K_AR_FWD_B4: ADARMS_FWD((adarms_fwd_k<bf16_t, 4, false>), bf16_t); break;
    case K_AR_FWD_B4G: ADARMS_FWD_G((adarms_fwd_k<bf16_t, 4, true>), bf16_t); break;
    case K_AR_FWD_B1: ADARMS_FWD((adarms_fwd_k<bf16_t, 1, false>), bf16_t); break;
    case K_AR_FWD_B1G: ADARMS_FWD_G((adarms_fwd_k<bf16_t, 1, true>), bf16_t); break;
    case K_AR_FWD_F4: ADARMS_FWD((adarms_fwd_k<float, 4, false>), float); break;
    case K_AR_FWD_F4G: ADARMS_FWD_G((adarms_fwd_k<float, 4, true>), float); break;
    case K_AR_FWD_F1: ADARMS_FWD((adarms_fwd_k<float, 1, false>), float); break;
    case K_AR_FWD_F1G: ADARMS_FWD_G((adarms_fwd_k<float, 1, true>), float); break;
    default: return unplanned("dxa_adarms_fwd", pl.k);
  }
#undef ADARMS_FWD
#undef ADARMS_FWD_G
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}

extern "C" int dxa_gated_residual_fwd(const void* x, const void* branch, const void* gate, int64_t gate_ld, void* y, int64_t rows,
                                      int64_t rows_per_sample, int64_t cols, int dtype, dxa_stream_t stream) {
  dxa_norm_desc d{};
  d.entry = DXA_NORM_GATED_RESIDUAL_FWD; d.dtype = dtype; d.rows = rows; d.rows_per_sample = rows_per_sample; d.cols = cols;
  d.gate_ld = gate_ld; d.x = x; d.x2 = branch; d.gate = gate; d.y = y;
  NormPlan pl;
  if (int rc = norm_plan(&d, &pl)) return rc;
  if (pl.k == K_NONE) return DXA_OK;
  hipStream_t st = (hipStream_t)stream;
#define GATED_FWD(T_, V_) hipLaunchKernelGGL((gated_residual_fwd_k<T_, V_>), pl.grid, dim3(pl.block), 0, st, (const T_*)x, (const T_*)branch, (const T_*)gate, gate_ld, (T_*)y, rows, rows_per_sample, cols)
  switch (pl.k) {
    case K_GR_FWD: GATED_FWD(bf16_t, 8); break;
    case K_GR_FWD_B4: GATED_FWD(bf16_t, 4); break;
    case K_GR_FWD_B1: GATED_FWD(bf16_t, 1); break;
    case K_GR_FWD_F4: GATED_FWD(float, 4); break;
    case K_GR_FWD_F1: GATED_FWD(float, 1); break;
    default: return unplanned("dxa_gated_residual_fwd", pl.k);
  }
#undef GATED_FWD
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}

extern "C" int dxa_adarms_bwd(const void* dy, const void* r, const void* mod, const float* rstd, const void* residual, void* dr,
                              void* dmod, const void* branch, const void* gate_prev, int64_t gate_ld, void* dbranch,
                              void* dgate_prev, int64_t dgate_ld, float* partial, size_t partial_bytes, int64_t rows,
                              int64_t rows_per_sample, int64_t cols, int dtype, dxa_stream_t stream) {
  dxa_norm_desc d{};
  d.entry = DXA_NORM_ADARMS_BWD; d.dtype = dtype; d.rows = rows; d.rows_per_sample = rows_per_sample; d.cols = cols;
  d.gate_ld = gate_ld; d.dgate_ld = dgate_ld; d.partial_bytes = partial_bytes;
  d.dy = dy; d.x = r; d.mod = mod; d.rstd = rstd; d.residual = residual; d.dx = dr; d.dmod = dmod; d.x2 = branch; d.gate = gate_prev;
  d.aux = dbranch; d.dgate = dgate_prev; d.partial = partial;
  NormPlan pl;
  if (int rc = norm_plan(&d, &pl)) return rc;
  if (pl.k == K_NONE) return DXA_OK;
  hipStream_t st = (hipStream_t)stream;
  const int nrow = (int)pl.grid.x * 4;
#define ADARMS_BWD_G(T_, V_) hipLaunchKernelGGL((adarms_bwd_k<T_, V_, true>), pl.grid, dim3(pl.block), 0, st, (const T_*)dy, (const T_*)r, (const T_*)mod, rstd, (const T_*)residual, (T_*)dr, (const T_*)branch, (const T_*)gate_prev, gate_ld, (T_*)dbranch, partial, rows_per_sample, cols)
#define ADARMS_BWD(T_, V_) hipLaunchKernelGGL((adarms_bwd_k<T_, V_, false>), pl.grid, dim3(pl.block), 0, st, (const T_*)dy, (const T_*)r, (const T_*)mod, rstd, (const T_*)residual, (T_*)dr, (const T_*)nullptr, (const T_*)nullptr, (int64_t)0, (T_*)nullptr, partial, rows_per_sample, cols)
  switch (pl.k) {
    case K_AR_BWD: ADARMS_BWD(bf16_t, 8); break;
    case K_AR_BWD_B8G: ADARMS_BWD_G(bf16_t, 8); break;
    case K_AR_BWD_B4: ADARMS_BWD(bf16_t, 4); break;
    case K_AR_BWD_B4G: ADARMS_BWD_G(bf16_t, 4); break;
    case K_AR_BWD_B1: ADARMS_BWD(bf16_t, 1); break;
    case K_AR_BWD_B1G: ADARMS_BWD_G(bf16_t, 1); break;
    case K_AR_BWD_F4: ADARMS_BWD(float, 4); break;
    case K_AR_BWD_F4G: ADARMS_BWD_G(float, 4); break;
    case K_AR_BWD_F1: ADARMS_BWD(float, 1); break;
    case K_AR_BWD_F1G: ADARMS_BWD_G(float, 1); break;
    default: return unplanned("dxa_adarms_bwd", pl.k);
  }
#undef ADARMS_BWD
#undef ADARMS_BWD_G
  const int64_t n = (int64_t)(branch ? 3 : 2) * cols;
  if (pl.k2 == K_FOLD)
    hipLaunchKernelGGL((adarms_fold_k<bf16_t>), pl.grid2, dim3(pl.block2), 0, st, partial, nrow, n, (bf16_t*)dmod, 3 * cols, 2 * cols, (bf16_t*)dgate_prev, dgate_ld);
  else
    hipLaunchKernelGGL((adarms_fold_k<float>), pl.grid2, dim3(pl.block2), 0, st, partial, nrow, n, (float*)dmod, 3 * cols, 2 * cols, (float*)dgate_prev, dgate_ld);
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}

extern "C" int dxa_gated_residual_bwd(const void* dy, const void* branch, const void* gate, int64_t gate_ld, void* dbranch,
                                      void* dgate, int64_t dgate_ld, float* partial, size_t partial_bytes, int64_t rows,
                                      int64_t rows_per_sample, int64_t cols, int dtype, dxa_stream_t stream) {
  dxa_norm_desc d{};
  d.entry = DXA_NORM_GATED_RESIDUAL_BWD; d.dtype = dtype; d.rows = rows; d.rows_per_sample = rows_per_sample; d.cols = cols;
  d.gate_ld = gate_ld; d.dgate_ld = dgate_ld; d.partial_bytes = partial_bytes;
  d.dy = dy; d.x2 = branch; d.gate = gate; d.dx = dbranch; d.dgate = dgate; d.partial = partial;
  NormPlan pl;
  if (int rc = norm_plan(&d, &pl)) return rc;
  if (pl.k == K_NONE) return DXA_OK;
  hipStream_t st = (hipStream_t)stream;
  const int nrow = (int)pl.grid.x * 4;
#define GATED_BWD(T_, V_) hipLaunchKernelGGL((gated_residual_bwd_k<T_, V_>), pl.grid, dim3(pl.block), 0, st, (const T_*)dy, (const T_*)branch, (const T_*)gate, gate_ld, (T_*)dbranch, partial, rows_per_sample, cols)
  switch (pl.k) {
    case K_GR_BWD: GATED_BWD(bf16_t, 8); break;
    case K_GR_BWD_B4: GATED_BWD(bf16_t, 4); break;
    case K_GR_BWD_B1: GATED_BWD(bf16_t, 1); break;
    case K_GR_BWD_F4: GATED_BWD(float, 4); break;
    case K_GR_BWD_F1: GATED_BWD(float, 1); break;
    default: return unplanned("dxa_gated_residual_bwd", pl.k);
  }
#undef GATED_BWD
  if (pl.k2 == K_FOLD)
    hipLaunchKernelGGL((adarms_fold_k<bf16_t>), pl.grid2, dim3(pl.block2), 0, st, partial, nrow, cols, (bf16_t*)nullptr, (int64_t)0, (int64_t)0, (bf16_t*)dgate, dgate_ld);
  else
    hipLaunchKernelGGL((adarms_fold_k<float>), pl.grid2, dim3(pl.block2), 0, st, partial, nrow, cols, (float*)nullptr, (int64_t)0, (int64_t)0, (float*)dgate, dgate_ld);
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}
