// The two ends of one Euler step of the DM0-prog flow-matching sampler (dexbotic/model/dm0/dm0_prog_arch.py: get_suffix_hidden_states
// :360-400 up to the input of action_time_mlp_in, and _denoise_step :567-576 from the expert's last layer on), one launch each.  The
// suffix of a sample is p + n rows: p in {0, 1} progress rows in front of the n = chunk_size action rows.  All arithmetic fp32, fixed
// summation orders, no atomics; every global write is a plain per-lane store.
#include "common.h"

namespace {

constexpr int64_t FLOW_MAX_DA = 8192;   // the tail keeps one normalised row in LDS (32 KB); the limit of adarms' one-pass kernel
constexpr int64_t FLOW_MAX_A = 1024;    // suffix_in keeps one action row in LDS (4 KB)

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ------------------------------------------------------------------------------------------------ suffix_in
// One workgroup per suffix row, out [B * (p + n), 2 * da]:
//   progress row (j < p):  out[:da] = progress[b] * w_p + b_p                                    (progress_in_proj, K = 1)
//   action row i = j - p:  out[:da] = W_in . rnd(x[b, i, :]) + b_in, k ascending                 (action_in_proj, K = A)
//   every row:             out[da:] = te[b, :]
// x is rounded to T first (what the cast in front of the composed product does), the sum is rounded once on store.  Thread t owns the
// columns [c, c + VEC) for c = t * VEC, t * VEC + 256 * VEC, ...; `wvec`: A % VEC == 0 and W_in 16-byte aligned, so a row of W_in is
// read VEC elements at a time as well.
template <typename T, int VEC>
__global__ __launch_bounds__(256) void flow_suffix_in_k(const float* __restrict__ x, int64_t ldx, const float* __restrict__ progress,
                                                        int64_t ldp, const T* __restrict__ te, const T* __restrict__ w_in,
                                                        const T* __restrict__ b_in, const T* __restrict__ w_p,
                                                        const T* __restrict__ b_p, T* __restrict__ out, int64_t n, int64_t A,
                                                        int64_t da, int p, int wvec) {
  __shared__ float xs[FLOW_MAX_A];
  const int64_t R = n + p;
  const int64_t b = blockIdx.x / R, j = blockIdx.x - b * R;
  T* orow = out + (int64_t)blockIdx.x * 2 * da;
  if (j < p) {                                               // (uniform over the workgroup)
    const float pr = progress[b * ldp];
    for (int64_t c = (int64_t)threadIdx.x * VEC; c < da; c += 256 * VEC) {
      float w[VEC], bb[VEC], o[VEC];
      Vec<T, VEC>::ld(w, w_p + c);
      Vec<T, VEC>::ld(bb, b_p + c);
#pragma unroll
      for (int i = 0; i < VEC; ++i) o[i] = pr * w[i] + bb[i];
      Vec<T, VEC>::st(orow + c, o);
    }
  } else {
    const float* xr = x + b * ldx + (j - p) * A;
    for (int64_t k = threadIdx.x; k < A; k += 256) xs[k] = rnd<T>(xr[k]);
    __syncthreads();
    for (int64_t c = (int64_t)threadIdx.x * VEC; c < da; c += 256 * VEC) {
      float acc[VEC], bb[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[i] = 0.f;
      bool done = false;
      if constexpr (VEC > 1) {
        if (wvec) {
          for (int64_t k0 = 0; k0 < A; k0 += VEC) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
              float w[VEC];
              Vec<T, VEC>::ld(w, w_in + (c + i) * A + k0);
#pragma unroll
              for (int q = 0; q < VEC; ++q) acc[i] = fmaf(w[q], xs[k0 + q], acc[i]);
            }
          }
          done = true;
        }
      }
      if (!done) {
#pragma unroll
        for (int i = 0; i < VEC; ++i)
          for (int64_t k = 0; k < A; ++k) acc[i] = fmaf(ldf<T>(w_in + (c + i) * A + k), xs[k], acc[i]);
      }
      Vec<T, VEC>::ld(bb, b_in + c);
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[i] += bb[i];
      Vec<T, VEC>::st(orow + c, acc);
    }
  }
  const T* ter = te + b * da;
  for (int64_t c = (int64_t)threadIdx.x * VEC; c < da; c += 256 * VEC) {
    float v[VEC];
    Vec<T, VEC>::ld(v, ter + c);
    Vec<T, VEC>::st(orow + da + c, v);
  }
}

// ------------------------------------------------------------------------------------------------ euler_tail
// One workgroup per suffix row of h [B * (p + n), da], the expert's rows BEFORE its final norm:
//   y = h * rsqrt(mean(h^2) + eps) * g                                (Qwen3 RMSNorm), kept in LDS as fp32
//   action row i:   x[b, i, a] += dt * (W_out[a, :] . y + b_out[a])   for every a < A, in place
//   progress row:   e = w_q . y + b_q;  prog_min[b] = min(prog_min[b], e), a NaN e wins (torch.min over the stacked steps)
// y and the velocity are NOT rounded to T in between: one rounding fewer than final norm -> slice -> action_out_proj -> .float(),
// which hands a bf16 y to the product and a bf16 velocity to the Euler update.
// Order of the sums: mean(h^2) — thread t adds its elements ascending (chunks t * VEC + k * 256 * VEC), then block_sum (xor-shuffle
// tree of the wave, the 4 waves in order); each dot product — wave a % 4 takes output a, lane l adds the columns of its chunks
// l * VEC + k * 64 * VEC ascending with fma, then the xor-shuffle tree over 64 lanes, then the bias.  One workgroup owns a sample's
// progress row, so the running minimum is a plain load and store.
template <typename T, int VEC>
__global__ __launch_bounds__(256) void flow_euler_tail_k(const T* __restrict__ h, const T* __restrict__ g, const T* __restrict__ w_out,
                                                         const T* __restrict__ b_out, const T* __restrict__ w_q,
                                                         const T* __restrict__ b_q, float* __restrict__ x, int64_t ldx,
                                                         float* __restrict__ prog_min, int64_t ldm, int64_t n, int64_t A, int64_t da,
                                                         int p, float eps, float dt) {
  __shared__ float ys[FLOW_MAX_DA];
  __shared__ float red[16];
  const int64_t R = n + p;
  const int64_t b = blockIdx.x / R, j = blockIdx.x - b * R;
  const T* hr = h + (int64_t)blockIdx.x * da;
  float ss = 0.f;
  for (int64_t c = (int64_t)threadIdx.x * VEC; c < da; c += 256 * VEC) {
    float v[VEC];
    Vec<T, VEC>::ld(v, hr + c);
#pragma unroll
    for (int i = 0; i < VEC; ++i) { ss += v[i] * v[i]; ys[c + i] = v[i]; }
  }
  const float rstd = rsqrtf(block_sum(ss, red) / (float)da + eps);
  for (int64_t c = (int64_t)threadIdx.x * VEC; c < da; c += 256 * VEC) {       // (the elements this thread staged itself)
    float gv[VEC];
    Vec<T, VEC>::ld(gv, g + c);
#pragma unroll
    for (int i = 0; i < VEC; ++i) ys[c + i] = ys[c + i] * rstd * gv[i];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const bool prog = j < p;                                   // (uniform over the workgroup)
  const int64_t n_out = prog ? 1 : A;
  const T* W = prog ? w_q : w_out;
  for (int64_t a = wv; a < n_out; a += 4) {
    const T* wr = W + a * da;
    float s = 0.f;
    for (int64_t c = (int64_t)lane * VEC; c < da; c += 64 * VEC) {
      float w[VEC];
      Vec<T, VEC>::ld(w, wr + c);
#pragma unroll
      for (int i = 0; i < VEC; ++i) s = fmaf(w[i], ys[c + i], s);
    }
    s = wave_sum(s);
    if (lane == 0) {
      if (prog) {
        const float e = s + ldf<T>(b_q);
        float* m = prog_min + b * ldm;
        const float cur = *m;
        *m = (e != e || e < cur) ? e : cur;
      } else {
        float* xp = x + b * ldx + (j - p) * A + a;
        *xp = fmaf(dt, s + ldf<T>(b_out + a), *xp);
      }
    }
  }
}

int check_flow(const char* who, int64_t B, int64_t n, int64_t A, int64_t da, int p, int64_t ldx, int dtype) {
  if (!(dtype == DXA_F32 || dtype == DXA_BF16)) {
    dxa_set_error("%s: unsupported dtype %d (fp32 / bf16 only)", who, dtype);
    return DXA_ERR_UNSUPPORTED;
  }
  DXA_CHECK_ARG(p == 0 || p == 1, "%s: p = %d progress rows per sample (0 or 1)", who, p);
  DXA_CHECK_ARG(B > 0 && n > 0 && A > 0 && da > 0, "%s: non-positive size B=%lld n=%lld A=%lld da=%lld", who, (long long)B, (long long)n,
                (long long)A, (long long)da);
  DXA_CHECK_ARG(da <= FLOW_MAX_DA, "%s: da = %lld above %lld (a row is staged in LDS as fp32)", who, (long long)da, (long long)FLOW_MAX_DA);
  DXA_CHECK_ARG(A <= FLOW_MAX_A && n <= (1 << 20) && B <= (1 << 20) && B * (n + p) <= (1ll << 24),
                "%s: sizes out of range B=%lld n=%lld A=%lld (A <= %lld, B * (p + n) <= 2^24)", who, (long long)B, (long long)n,
                (long long)A, (long long)FLOW_MAX_A);
  DXA_CHECK_ARG(ldx >= n * A, "%s: ldx = %lld below n * A = %lld", who, (long long)ldx, (long long)(n * A));
  return DXA_OK;
}

}  // namespace

extern "C" int dxa_flow_suffix_in(const float* x, int64_t ldx, const float* progress, int64_t ldp, const void* te, const void* w_in,
                                  const void* b_in, const void* w_p, const void* b_p, void* out, int64_t B, int64_t n, int64_t A,
                                  int64_t da, int p, int dtype, dxa_stream_t stream) {
  DXA_CHECK_ARG(x && te && w_in && b_in && out, "dxa_flow_suffix_in: null x / te / w_in / b_in / out");
  if (int rc = check_flow("dxa_flow_suffix_in", B, n, A, da, p, ldx, dtype)) return rc;
  DXA_CHECK_ARG(p == 0 || (progress && w_p && b_p && ldp >= 1), "dxa_flow_suffix_in: p = 1 needs progress (ldp >= 1), w_p and b_p");
  hipStream_t st = (hipStream_t)stream;
  const int vec = dtype == DXA_BF16 ? 8 : 4;
  const bool vec_ok = da % vec == 0 && al16(te) && al16(b_in) && al16(out) && (!p || (al16(w_p) && al16(b_p)));
  const int wvec = A % vec == 0 && al16(w_in);
  dim3 grid((unsigned)(B * (n + p)));
#define SUF(T_, V_) hipLaunchKernelGGL((flow_suffix_in_k<T_, V_>), grid, dim3(256), 0, st, x, ldx, progress, ldp, (const T_*)te, (const T_*)w_in, (const T_*)b_in, (const T_*)w_p, (const T_*)b_p, (T_*)out, n, A, da, p, wvec)
  if (dtype == DXA_BF16) { if (vec_ok) SUF(bf16_t, 8); else SUF(bf16_t, 1); }
  else { if (vec_ok) SUF(float, 4); else SUF(float, 1); }
#undef SUF
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}

extern "C" int dxa_flow_euler_tail(const void* h, const void* g, const void* w_out, const void* b_out, const void* w_q, const void* b_q,
                                   float* x, int64_t ldx, float* prog_min, int64_t ldm, int64_t B, int64_t n, int64_t A, int64_t da,
                                   int p, float eps, float dt, int dtype, dxa_stream_t stream) {
  DXA_CHECK_ARG(h && g && w_out && b_out && x, "dxa_flow_euler_tail: null h / g / w_out / b_out / x");
  if (int rc = check_flow("dxa_flow_euler_tail", B, n, A, da, p, ldx, dtype)) return rc;
  DXA_CHECK_ARG(p == 0 || (prog_min && w_q && b_q && ldm >= 1), "dxa_flow_euler_tail: p = 1 needs prog_min (ldm >= 1), w_q and b_q");
  hipStream_t st = (hipStream_t)stream;
  const int vec = dtype == DXA_BF16 ? 8 : 4;
  const bool vec_ok = da % vec == 0 && al16(h) && al16(g) && al16(w_out) && (!p || al16(w_q));
  dim3 grid((unsigned)(B * (n + p)));
#define TAIL(T_, V_) hipLaunchKernelGGL((flow_euler_tail_k<T_, V_>), grid, dim3(256), 0, st, (const T_*)h, (const T_*)g, (const T_*)w_out, (const T_*)b_out, (const T_*)w_q, (const T_*)b_q, x, ldx, prog_min, ldm, n, A, da, p, eps, dt)
  if (dtype == DXA_BF16) { if (vec_ok) TAIL(bf16_t, 8); else TAIL(bf16_t, 1); }
  else { if (vec_ok) TAIL(float, 4); else TAIL(float, 1); }
#undef TAIL
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}
