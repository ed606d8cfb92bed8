// ColorJitter of the training augmentations (dexbotic/data/dataset/augmentations.py: policy_v3 / policy_color /
// policy_color_dm0) on uint8 RGB frames in HBM, in place, every frame with its own parameters.  The arithmetic is
// color_jitter.h's.  Contrast needs the mean L of the whole frame as the ops before it left it, so there are two launches:
//   jitter_mean_k   recomputes those ops per pixel and adds L up per frame: 64-bit integer sums, one atomic per workgroup
//                   (integer addition does not depend on the order, so the result is deterministic)
//   jitter_apply_k  applies the four ops per pixel in registers and stores the frame back
// Byte work: a lane owns four pixels = three dwords of interleaved RGB when the frame is dword-aligned, bytes otherwise.
#include "color_jitter.h"
#include "common.h"

namespace {

constexpr int PIX_PER_LANE = 4;
constexpr int PIX_PER_BLOCK = 256 * PIX_PER_LANE;

// four pixels of a frame from / to byte offset 3 * px; `whole` = all four exist and the frame is dword-aligned
__device__ __forceinline__ void load4(const uint8_t* f, int64_t px, int cnt, bool whole, cj_rgb (&c)[PIX_PER_LANE]) {
  if (whole) {
    const uint32_t* q = reinterpret_cast<const uint32_t*>(f + 3 * px);
    const uint32_t a = q[0], b = q[1], d = q[2];
    c[0] = cj_rgb{(int)(a & 255), (int)((a >> 8) & 255), (int)((a >> 16) & 255)};
    c[1] = cj_rgb{(int)(a >> 24), (int)(b & 255), (int)((b >> 8) & 255)};
    c[2] = cj_rgb{(int)((b >> 16) & 255), (int)(b >> 24), (int)(d & 255)};
    c[3] = cj_rgb{(int)((d >> 8) & 255), (int)((d >> 16) & 255), (int)(d >> 24)};
    return;
  }
#pragma unroll
  for (int i = 0; i < PIX_PER_LANE; ++i) {
    c[i] = cj_rgb{0, 0, 0};
    if (i < cnt) c[i] = cj_rgb{f[3 * (px + i)], f[3 * (px + i) + 1], f[3 * (px + i) + 2]};
  }
}

__device__ __forceinline__ void store4(uint8_t* f, int64_t px, int cnt, bool whole, const cj_rgb (&c)[PIX_PER_LANE]) {
  if (whole) {
    uint32_t* q = reinterpret_cast<uint32_t*>(f + 3 * px);
    q[0] = (uint32_t)c[0].r | ((uint32_t)c[0].g << 8) | ((uint32_t)c[0].b << 16) | ((uint32_t)c[1].r << 24);
    q[1] = (uint32_t)c[1].g | ((uint32_t)c[1].b << 8) | ((uint32_t)c[2].r << 16) | ((uint32_t)c[2].g << 24);
    q[2] = (uint32_t)c[2].b | ((uint32_t)c[3].r << 8) | ((uint32_t)c[3].g << 16) | ((uint32_t)c[3].b << 24);
    return;
  }
#pragma unroll
  for (int i = 0; i < PIX_PER_LANE; ++i)
    if (i < cnt) {
      f[3 * (px + i)] = (uint8_t)c[i].r;
      f[3 * (px + i) + 1] = (uint8_t)c[i].g;
      f[3 * (px + i) + 2] = (uint8_t)c[i].b;
    }
}

// grid (workgroups per frame, n); a workgroup walks the frame in steps of gridDim.x * PIX_PER_BLOCK pixels
template <bool APPLY>
__global__ __launch_bounds__(256) void jitter_k(uint8_t* pixels, int64_t npix, const dxa_jitter_params* params,
                                                unsigned long long* sums) {
  __shared__ unsigned long long red[4];
  const int img = blockIdx.y;
  const dxa_jitter_params jp = params[img];
  if (!jp.apply) return;                                  // uniform per workgroup
  uint8_t* f = pixels + (size_t)img * npix * 3;
  const bool aligned = ((uintptr_t)f & 3) == 0;
  int m = 0;
  if (APPLY) m = (int)((2 * sums[img] + (unsigned long long)npix) / (2 * (unsigned long long)npix));
  unsigned long long acc = 0;
  for (int64_t p0 = (int64_t)blockIdx.x * PIX_PER_BLOCK; p0 < npix; p0 += (int64_t)gridDim.x * PIX_PER_BLOCK) {
    const int64_t px = p0 + PIX_PER_LANE * threadIdx.x;
    const int64_t left = npix - px;
    const int cnt = left >= PIX_PER_LANE ? PIX_PER_LANE : (left > 0 ? (int)left : 0);
    if (cnt == 0) continue;
    const bool whole = aligned && cnt == PIX_PER_LANE;
    cj_rgb c[PIX_PER_LANE];
    load4(f, px, cnt, whole, c);
    if (APPLY) {
#pragma unroll
      for (int i = 0; i < PIX_PER_LANE; ++i) c[i] = cj_all_ops(c[i], jp, m);
      store4(f, px, cnt, whole, c);
    } else {
#pragma unroll
      for (int i = 0; i < PIX_PER_LANE; ++i)
        if (i < cnt) {
          const cj_rgb v = cj_before_contrast(c[i], jp);
          acc += (unsigned)cj_grey(v.r, v.g, v.b);
        }
    }
  }
  if (!APPLY) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(sums + img, red[0] + red[1] + red[2] + red[3]);
  }
}

bool params_ok(const dxa_jitter_params& q) {
  int seen = 0;
  for (int i = 0; i < 4; ++i)
    if (q.order[i] >= 0 && q.order[i] < 4) seen |= 1 << q.order[i];
  const float f[3] = {q.brightness, q.contrast, q.saturation};
  for (int i = 0; i < 3; ++i)
    if (!(f[i] >= 0.f && f[i] <= 1e6f)) return false;
  return seen == 15 && q.hue >= -0.5f && q.hue <= 0.5f;
}

}  // namespace

extern "C" int dxa_color_jitter(void* pixels, int n, int h, int w, const dxa_jitter_params* params,
                                const dxa_jitter_params* params_host, uint64_t* sums, dxa_stream_t stream) {
  DXA_CHECK_ARG(n >= 0 && h > 0 && w > 0, "dxa_color_jitter: bad frame size");
  if (n == 0) return DXA_OK;
  DXA_CHECK_ARG(pixels && sums, "dxa_color_jitter: null buffer");
  DXA_CHECK_ARG(params && params_host, "dxa_color_jitter: null parameter table");
  DXA_CHECK_ARG(n <= 65535, "dxa_color_jitter: too many frames per call");
  DXA_CHECK_ARG((uintptr_t)sums % 8 == 0, "dxa_color_jitter: sums must be 8-byte aligned");
  bool any = false;
  for (int i = 0; i < n; ++i) {
    if (!params_host[i].apply) continue;
    any = true;
    DXA_CHECK_ARG(params_ok(params_host[i]),
                  "dxa_color_jitter: frame %d: order must be a permutation of the four ops, factors >= 0, |hue| <= 0.5", i);
  }
  if (!any) return DXA_OK;
  const int64_t npix = (int64_t)h * w;
  hipStream_t st = (hipStream_t)stream;
  DXA_CHECK_HIP(hipMemsetAsync(sums, 0, (size_t)n * sizeof(uint64_t), st));
  // enough workgroups per frame to fill the chip with a batch of one, no more than the frame has blocks of work
  int per_frame = dxa_cdiv(npix, PIX_PER_BLOCK);
  if (per_frame > 1024) per_frame = 1024;
  unsigned long long* s64 = reinterpret_cast<unsigned long long*>(sums);
  hipLaunchKernelGGL(jitter_k<false>, dim3(per_frame, n), dim3(256), 0, st, (uint8_t*)pixels, npix, params, s64);
  DXA_CHECK_LAUNCH();
  hipLaunchKernelGGL(jitter_k<true>, dim3(per_frame, n), dim3(256), 0, st, (uint8_t*)pixels, npix, params, s64);
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}

extern "C" int dxa_color_jitter_pixels_host(void* pixels, int64_t k, const dxa_jitter_params* params, int m) {
  DXA_CHECK_ARG(k >= 0, "dxa_color_jitter_pixels_host: negative pixel count");
  if (k == 0) return DXA_OK;
  DXA_CHECK_ARG(pixels && params, "dxa_color_jitter_pixels_host: null buffer");
  DXA_CHECK_ARG(params_ok(*params),
                "dxa_color_jitter_pixels_host: order must be a permutation of the four ops, factors >= 0, |hue| <= 0.5");
  DXA_CHECK_ARG(m >= 0 && m <= 255, "dxa_color_jitter_pixels_host: contrast mean outside 0..255");
  uint8_t* px = (uint8_t*)pixels;
  for (int64_t i = 0; i < k; ++i) {
    const cj_rgb c = cj_all_ops(cj_rgb{px[3 * i], px[3 * i + 1], px[3 * i + 2]}, *params, m);
    px[3 * i] = (uint8_t)c.r;
    px[3 * i + 1] = (uint8_t)c.g;
    px[3 * i + 2] = (uint8_t)c.b;
  }
  return DXA_OK;
}
