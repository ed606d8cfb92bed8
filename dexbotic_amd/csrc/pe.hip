// Perception Encoder vision tower (dexbotic/model/modules/mm_vision/pe/pe_model.py): the three memory-bound pieces between its GEMMs.
//   rope2d              in-place interleaved-pair rotation of the q and k thirds of the packed qkv rows, from cos/sin tables
//   layerscale_residual y = x + gamma[c] * h, and its backward (dh, per-column partial sums of dgamma)
//   conv3x3s2           im2col rows of a 3x3 / stride 2 / pad 1 convolution over a token-major grid, and the adjoint gather
// 16-byte accesses where the rows allow, narrower ones otherwise; no atomics; sums in a fixed order.
#include "common.h"

namespace {

// N elements into floats: one access where Vec has that width, 16-byte pieces for eight floats, element by element for a pair
template <typename T, int N>
__device__ __forceinline__ void ld_n(float (&o)[N], const T* p) {
  if constexpr (N == 2) {
    o[0] = ldf<T>(p); o[1] = ldf<T>(p + 1);
  } else if constexpr (N == 8 && sizeof(T) == 4) {
    float a[4], b[4];
    Vec<T, 4>::ld(a, p); Vec<T, 4>::ld(b, p + 4);
#pragma unroll
    for (int k = 0; k < 4; ++k) { o[k] = a[k]; o[4 + k] = b[k]; }
  } else {
    Vec<T, N>::ld(o, p);
  }
}

// ------------------------------------------------------------------------------------------------ 2-D RoPE
// One thread owns VEC consecutive columns of one head of q or k: VEC / 2 whole (even, odd) pairs.  The q and k thirds of a token row
// [3][H][D] are its first 2*H*D elements, so a token's work items are contiguous.  BWD applies the transposed rotation.
// A chunk whose angles are all zero (the CLS row) is not written at all.
template <typename T, int VEC, bool BWD>
__global__ __launch_bounds__(256) void rope2d_k(T* __restrict__ qkv, const float* __restrict__ cos_t, const float* __restrict__ sin_t,
                                                int64_t rows, int T_, int HD, int D) {
  const int per_row = 2 * HD / VEC;
  const int64_t total = rows * per_row;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t row = i / per_row;
    const int col = (int)(i - row * per_row) * VEC;          // column in [0, 2*H*D)
    const int d = col % D;
    const int t = (int)(row % T_);
    float c[VEC], s[VEC], x[VEC], y[VEC];
    ld_n<float, VEC>(c, cos_t + (int64_t)t * D + d);
    ld_n<float, VEC>(s, sin_t + (int64_t)t * D + d);
    bool ident = true;
#pragma unroll
    for (int k = 0; k < VEC; ++k) ident = ident && c[k] == 1.f && s[k] == 0.f;
    if (ident) continue;
    T* p = qkv + row * 3 * HD + col;
    ld_n<T, VEC>(x, p);
#pragma unroll
    for (int k = 0; k < VEC; k += 2) {
      // every product rounded on its own, then one add (no contraction): the fp32 arithmetic of t * cos + rotate_half(t) * sin
      if (!BWD) {
        y[k] = __fadd_rn(__fmul_rn(x[k], c[k]), __fmul_rn(-x[k + 1], s[k]));
        y[k + 1] = __fadd_rn(__fmul_rn(x[k + 1], c[k + 1]), __fmul_rn(x[k], s[k + 1]));
      } else {
        y[k] = __fadd_rn(__fmul_rn(x[k], c[k]), __fmul_rn(x[k + 1], s[k + 1]));
        y[k + 1] = __fadd_rn(__fmul_rn(x[k + 1], c[k + 1]), __fmul_rn(-x[k], s[k]));
      }
    }
    if constexpr (VEC == 2) { stf<T>(p, y[0]); stf<T>(p + 1, y[1]); }
    else Vec<T, VEC>::st(p, y);
  }
}

// ------------------------------------------------------------------------------------------------ LayerScale + residual
template <typename T, int VEC>
__global__ __launch_bounds__(256) void layerscale_residual_fwd_k(const T* __restrict__ x, const T* __restrict__ h,
                                                                 const T* __restrict__ gamma, T* __restrict__ y, int64_t rows,
                                                                 int64_t cols) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  for (int64_t c = (int64_t)lane * VEC; c < cols; c += 64 * VEC) {
    float v[VEC], b[VEC], g[VEC];
    Vec<T, VEC>::ld(v, x + row * cols + c);
    Vec<T, VEC>::ld(b, h + row * cols + c);
    Vec<T, VEC>::ld(g, gamma + c);
#pragma unroll
    for (int i = 0; i < VEC; ++i) v[i] = __builtin_fmaf(b[i], g[i], v[i]);
    Vec<T, VEC>::st(y + row * cols + c, v);
  }
}

// grid (row groups, column tiles of 64 * VEC).  Wave w of row group b owns rows b * 4 + w, + 4 * gridDim.x, ... and partial row
// b * 4 + w of `partial` [4 * gridDim.x][cols]; a lane owns VEC columns of the tile for the whole launch: gamma and the running sums
// of dy * h stay in registers, added in row order, and are written once at the end (zeros for a wave without a row).
template <typename T, int VEC>
__global__ __launch_bounds__(256) void layerscale_residual_bwd_k(const T* __restrict__ dy, const T* __restrict__ h,
                                                                 const T* __restrict__ gamma, T* __restrict__ dh,
                                                                 float* __restrict__ partial, int64_t rows, int64_t cols) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t c = ((int64_t)blockIdx.y * 64 + lane) * VEC;
  if (c >= cols) return;
  float g[VEC], acc[VEC];
  Vec<T, VEC>::ld(g, gamma + c);
#pragma unroll
  for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
#pragma unroll 2
  for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < rows; r += (int64_t)gridDim.x * 4) {
    float gv[VEC], hv[VEC], o[VEC];
    Vec<T, VEC>::ld(gv, dy + r * cols + c);
    Vec<T, VEC>::ld(hv, h + r * cols + c);
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      o[k] = gv[k] * g[k];
      acc[k] = __builtin_fmaf(gv[k], hv[k], acc[k]);
    }
    Vec<T, VEC>::st(dh + r * cols + c, o);
  }
  float* slab = partial + ((int64_t)blockIdx.x * 4 + wave) * cols + c;
  if constexpr (VEC % 4 == 0) {
#pragma unroll
    for (int k = 0; k < VEC; k += 4) *reinterpret_cast<float4*>(slab + k) = make_float4(acc[k], acc[k + 1], acc[k + 2], acc[k + 3]);
  } else {
#pragma unroll
    for (int k = 0; k < VEC; ++k) slab[k] = acc[k];
  }
}

constexpr int LAYERSCALE_BWD_MAX_BLOCKS = 256;

// widest access the column count and every pointer allow: 8 (bf16 only), 4 or 1 elements
int pe_vec(int dtype, int64_t cols, std::initializer_list<const void*> ptrs) {
  const size_t es = dtype == DXA_BF16 ? 2 : 4;
  int vec = dtype == DXA_BF16 ? 8 : 4;
  for (; vec > 1; vec >>= 1) {
    bool ok = cols % vec == 0;
    for (const void* p : ptrs) ok = ok && (reinterpret_cast<uintptr_t>(p) % (vec * es)) == 0;
    if (ok) break;
  }
  return vec;
}

// ------------------------------------------------------------------------------------------------ 3x3 stride-2 convolution rows
// x [B, T*T, C] token-major -> rows [B*To*To, 9*C], column c*9 + ky*3 + kx (the flattening of the Conv2d weight [C', C, 3, 3]) =
// x[b, 2*oy + ky - 1, 2*ox + kx - 1, c], zero outside the grid.  One thread owns VEC channels of one output position: nine VEC-wide
// loads (one per tap), transposed in registers, leave as nine VEC-wide stores of its 9 * VEC consecutive columns.
template <typename T, int VEC>
__global__ __launch_bounds__(256) void conv3x3s2_im2col_k(const T* __restrict__ x, T* __restrict__ rows, int64_t B, int T_, int To,
                                                          int C) {
  const int cv = C / VEC;
  const int64_t total = B * To * To * cv;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c0 = (int)(i % cv) * VEC;
    const int64_t r = i / cv;                                  // output row (b, oy, ox)
    const int ox = (int)(r % To), oy = (int)((r / To) % To);
    const int64_t b = r / ((int64_t)To * To);
    float o[9 * VEC];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int iy = 2 * oy + tap / 3 - 1, ix = 2 * ox + tap % 3 - 1;
      float v[VEC];
      if (iy >= 0 && iy < T_ && ix >= 0 && ix < T_) {
        Vec<T, VEC>::ld(v, x + ((b * T_ + iy) * T_ + ix) * C + c0);
      } else {
#pragma unroll
        for (int k = 0; k < VEC; ++k) v[k] = 0.f;
      }
#pragma unroll
      for (int k = 0; k < VEC; ++k) o[k * 9 + tap] = v[k];
    }
    T* dst = rows + r * 9 * C + (int64_t)c0 * 9;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
      float v[VEC];
#pragma unroll
      for (int k = 0; k < VEC; ++k) v[k] = o[j * VEC + k];
      Vec<T, VEC>::st(dst + j * VEC, v);
    }
  }
}

// The adjoint as a gather: dx[b, y, x, c] = sum over the taps (ky, kx) for which (y + 1 - ky, x + 1 - kx) is twice an output position
// in range, of drows[(b, oy, ox), c*9 + ky*3 + kx] — at most four of them, added in (ky, kx) order in fp32.  Every dx element is
// written.
template <typename T, int VEC>
__global__ __launch_bounds__(256) void conv3x3s2_col2im_k(const T* __restrict__ drows, T* __restrict__ dx, int64_t B, int T_, int To,
                                                          int C) {
  const int cv = C / VEC;
  const int64_t total = B * T_ * T_ * cv;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c0 = (int)(i % cv) * VEC;
    const int64_t pix = i / cv;
    const int xx = (int)(pix % T_), yy = (int)((pix / T_) % T_);
    const int64_t b = pix / ((int64_t)T_ * T_);
    float acc[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
    for (int ky = 0; ky < 3; ++ky) {
      const int ty = yy + 1 - ky;
      if (ty < 0 || (ty & 1) || ty / 2 >= To) continue;
      for (int kx = 0; kx < 3; ++kx) {
        const int tx = xx + 1 - kx;
        if (tx < 0 || (tx & 1) || tx / 2 >= To) continue;
        const T* src = drows + ((b * To + ty / 2) * To + tx / 2) * 9 * C + (int64_t)c0 * 9 + ky * 3 + kx;
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] += ldf<T>(src + k * 9);
      }
    }
    Vec<T, VEC>::st(dx + pix * C + c0, acc);
  }
}

int check_conv(const char* who, const void* a, const void* b, int64_t B, int T_, int C, int dtype) {
  DXA_CHECK_ARG(dtype == DXA_F32 || dtype == DXA_BF16, "%s: unsupported dtype %d", who, dtype);
  DXA_CHECK_ARG(a && b, "%s: null pointer", who);
  DXA_CHECK_ARG(B >= 0 && T_ > 0 && C > 0, "%s: bad sizes (B %lld, T %d, C %d)", who, (long long)B, T_, C);
  DXA_CHECK_ARG((int64_t)T_ * T_ * 9 * C < ((int64_t)1 << 40), "%s: grid too large", who);
  return DXA_OK;
}

}  // namespace

static int rope2d_launch(void* qkv, const float* cos_t, const float* sin_t, int64_t N, int T_, int H, int D, int dtype, bool bwd,
                         dxa_stream_t stream, const char* who) {
  DXA_CHECK_ARG(dtype == DXA_F32 || dtype == DXA_BF16, "%s: unsupported dtype %d", who, dtype);
  DXA_CHECK_ARG(qkv && cos_t && sin_t, "%s: null qkv / cos / sin", who);
  DXA_CHECK_ARG(N >= 0 && T_ > 0 && H > 0 && D > 0, "%s: bad sizes (N %lld, T %d, H %d, D %d)", who, (long long)N, T_, H, D);
  DXA_CHECK_ARG(D % 4 == 0, "%s: head width %d is not a multiple of 4", who, D);
  DXA_CHECK_ARG((int64_t)H * D <= (1 << 24), "%s: H * D too large", who);
  if (N == 0) return DXA_OK;
  hipStream_t st = (hipStream_t)stream;
  const int HD = H * D;
  const int64_t rows = N * T_;
  // D % 4 == 0 keeps every chunk inside one head; the fp32 tables are read four floats at a time, and two where they (or the
  // rows) are not 16-byte aligned — a pair never splits
  int vec = pe_vec(dtype, D, {qkv});
  if (vec < 4 || ((reinterpret_cast<uintptr_t>(cos_t) | reinterpret_cast<uintptr_t>(sin_t)) % 16) != 0) vec = 2;
  const int grid = dxa_grid1d(rows * (2 * HD / vec), 256);
#define ROPE2D(T_T, V_) do { \
    if (bwd) hipLaunchKernelGGL((rope2d_k<T_T, V_, true>), dim3(grid), dim3(256), 0, st, (T_T*)qkv, cos_t, sin_t, rows, T_, HD, D); \
    else hipLaunchKernelGGL((rope2d_k<T_T, V_, false>), dim3(grid), dim3(256), 0, st, (T_T*)qkv, cos_t, sin_t, rows, T_, HD, D); } while (0)
  if (dtype == DXA_BF16) { if (vec == 8) ROPE2D(bf16_t, 8); else if (vec == 4) ROPE2D(bf16_t, 4); else ROPE2D(bf16_t, 2); }
  else { if (vec == 4) ROPE2D(float, 4); else ROPE2D(float, 2); }
#undef ROPE2D
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}

extern "C" int dxa_rope2d_fwd(void* qkv, const float* cos_t, const float* sin_t, int64_t N, int T, int H, int D, int dtype,
                              dxa_stream_t stream) {
  return rope2d_launch(qkv, cos_t, sin_t, N, T, H, D, dtype, false, stream, "dxa_rope2d_fwd");
}

extern "C" int dxa_rope2d_bwd(void* dqkv, const float* cos_t, const float* sin_t, int64_t N, int T, int H, int D, int dtype,
                              dxa_stream_t stream) {
  return rope2d_launch(dqkv, cos_t, sin_t, N, T, H, D, dtype, true, stream, "dxa_rope2d_bwd");
}

extern "C" int dxa_layerscale_residual_fwd(const void* x, const void* h, const void* gamma, void* y, int64_t rows, int64_t cols,
                                           int dtype, dxa_stream_t stream) {
  DXA_CHECK_ARG(dtype == DXA_F32 || dtype == DXA_BF16, "dxa_layerscale_residual_fwd: unsupported dtype %d", dtype);
  DXA_CHECK_ARG(x && h && gamma && y && rows >= 0 && cols > 0, "dxa_layerscale_residual_fwd: null x / h / gamma / y or bad sizes");
  if (rows == 0) return DXA_OK;
  hipStream_t st = (hipStream_t)stream;
  const int vec = pe_vec(dtype, cols, {x, h, gamma, y});
  dim3 grid((unsigned)((rows + 3) / 4));
#define LS_FWD(T_, V_) hipLaunchKernelGGL((layerscale_residual_fwd_k<T_, V_>), grid, dim3(256), 0, st, (const T_*)x, (const T_*)h, (const T_*)gamma, (T_*)y, rows, cols)
  if (dtype == DXA_BF16) { if (vec == 8) LS_FWD(bf16_t, 8); else if (vec == 4) LS_FWD(bf16_t, 4); else LS_FWD(bf16_t, 1); }
  else { if (vec == 4) LS_FWD(float, 4); else LS_FWD(float, 1); }
#undef LS_FWD
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}

extern "C" int dxa_layerscale_bwd_rows(int64_t rows) {
  int64_t g = (rows + 3) / 4;
  if (g < 1) g = 1;
  if (g > LAYERSCALE_BWD_MAX_BLOCKS) g = LAYERSCALE_BWD_MAX_BLOCKS;
  return (int)g * 4;
}

extern "C" int dxa_layerscale_residual_bwd(const void* dy, const void* h, const void* gamma, void* dh, float* partial,
                                           size_t partial_bytes, int64_t rows, int64_t cols, int dtype, dxa_stream_t stream) {
  DXA_CHECK_ARG(dtype == DXA_F32 || dtype == DXA_BF16, "dxa_layerscale_residual_bwd: unsupported dtype %d", dtype);
  DXA_CHECK_ARG(dy && h && gamma && dh && partial && rows >= 0 && cols > 0,
                "dxa_layerscale_residual_bwd: null dy / h / gamma / dh / partial or bad sizes");
  const int prow = dxa_layerscale_bwd_rows(rows);
  const size_t need = (size_t)prow * cols * sizeof(float);
  DXA_CHECK_ARG(partial_bytes >= need, "dxa_layerscale_residual_bwd: partial too small (need %zu bytes)", need);
  hipStream_t st = (hipStream_t)stream;
  DXA_CHECK_ARG(reinterpret_cast<uintptr_t>(partial) % 16 == 0, "dxa_layerscale_residual_bwd: partial is not 16-byte aligned");
  const int vec = pe_vec(dtype, cols, {dy, h, gamma, dh});
  dim3 grid((unsigned)(prow / 4),(unsigned)((cols + 64 * vec - 1) / (64 * vec)));
#define LS_BWD(T_, V_) hipLaunchKernelGGL((layerscale_residual_bwd_k<T_, V_>), grid, dim3(256), 0, st, (const T_*)dy, (const T_*)h, (const T_*)gamma, (T_*)dh, partial, rows, cols)
  if (dtype == DXA_BF16) { if (vec == 8) LS_BWD(bf16_t, 8); else if (vec == 4) LS_BWD(bf16_t, 4); else LS_BWD(bf16_t, 1); }
  else { if (vec == 4) LS_BWD(float, 4); else LS_BWD(float, 1); }
#undef LS_BWD
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}

extern "C" int dxa_conv3x3s2_im2col(const void* x, void* rows, int64_t B, int T, int C, int dtype, dxa_stream_t stream) {
  if (int rc = check_conv("dxa_conv3x3s2_im2col", x, rows, B, T, C, dtype)) return rc;
  if (B == 0) return DXA_OK;
  hipStream_t st = (hipStream_t)stream;
  const int To = (T - 1) / 2 + 1;
  // a thread's 9 * VEC output columns start at c0 * 9: a multiple of VEC elements, as the row length 9 * C is
  const int vec = pe_vec(dtype, C, {x, rows});
  const int grid = dxa_grid1d(B * To * To * (C / vec), 256);
#define CONV_I2C(T_, V_) hipLaunchKernelGGL((conv3x3s2_im2col_k<T_, V_>), dim3(grid), dim3(256), 0, st, (const T_*)x, (T_*)rows, B, T, To, C)
  if (dtype == DXA_BF16) { if (vec == 8) CONV_I2C(bf16_t, 8); else if (vec == 4) CONV_I2C(bf16_t, 4); else CONV_I2C(bf16_t, 1); }
  else { if (vec == 4) CONV_I2C(float, 4); else CONV_I2C(float, 1); }
#undef CONV_I2C
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}

extern "C" int dxa_conv3x3s2_col2im(const void* drows, void* dx, int64_t B, int T, int C, int dtype, dxa_stream_t stream) {
  if (int rc = check_conv("dxa_conv3x3s2_col2im", drows, dx, B, T, C, dtype)) return rc;
  if (B == 0) return DXA_OK;
  hipStream_t st = (hipStream_t)stream;
  const int To = (T - 1) / 2 + 1;
  const int vec = pe_vec(dtype, C, {dx});                      // drows is read element by element (stride 9)
  const int grid = dxa_grid1d(B * T * T * (C / vec), 256);
#define CONV_C2I(T_, V_) hipLaunchKernelGGL((conv3x3s2_col2im_k<T_, V_>), dim3(grid), dim3(256), 0, st, (const T_*)drows, (T_*)dx, B, T, To, C)
  if (dtype == DXA_BF16) { if (vec == 8) CONV_C2I(bf16_t, 8); else if (vec == 4) CONV_C2I(bf16_t, 4); else CONV_C2I(bf16_t, 1); }
  else { if (vec == 4) CONV_C2I(float, 4); else CONV_C2I(float, 1); }
#undef CONV_C2I
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}
