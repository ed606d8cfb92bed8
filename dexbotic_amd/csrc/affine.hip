// Bilinear affine warp of the training augmentations (dexbotic/data/dataset/augmentations.py: the Rotate of policy_pi0 and
// policy_dm0) on uint8 RGB frames in HBM, out of place, every frame with its own inverse matrix.  The arithmetic is
// affine_warp.h's.  One launch; byte work with a gather, measured in profiles/device_augment_rotate.txt.
// Thread mapping: a lane owns ONE pixel of the flattened frame, consecutive lanes consecutive pixels.  Under a few degrees the
// sources of neighbouring outputs are neighbours, so the twelve byte loads of a wave each fall on two or three cache lines of a
// source row (a lane that owned four pixels would spread each load over four times as many).  The stores go out as dwords all
// the same: four neighbouring lanes hold twelve bytes = three dwords, lane k < 3 of the four puts dword k together from its
// own pixel and the next lane's (one shuffle) and stores it, so a wave writes 192 contiguous bytes with 48 dword stores.  That
// needs the output frame to start on a dword (every frame does when 3 * h * w is a multiple of 4) and all four pixels to
// exist; otherwise every lane stores its three bytes.
#include "affine_warp.h"
#include "common.h"

namespace {

constexpr int PIX_PER_BLOCK = 256;

// grid (workgroups per frame, n); a workgroup walks the frame in steps of gridDim.x * PIX_PER_BLOCK pixels
__global__ __launch_bounds__(256) void affine_k(const uint8_t* src, uint8_t* dst, int h, int w, const double* mats, uint32_t fill) {
  const int img = blockIdx.y;
  const uint32_t npix = (uint32_t)h * (uint32_t)w;             // < 2^31: checked by the entry point
  const uint8_t* f = src + (size_t)img * npix * 3;
  uint8_t* o = dst + (size_t)img * npix * 3;
  double m[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) m[i] = mats[6 * (size_t)img + i];   // uniform per workgroup
  const bool aligned = ((uintptr_t)o & 3) == 0;
  const uint32_t k = threadIdx.x & 3;
  // p0 is the same in every lane, so the whole workgroup takes every trip and every lane reaches the shuffle
  for (uint32_t p0 = blockIdx.x * PIX_PER_BLOCK; p0 < npix; p0 += gridDim.x * PIX_PER_BLOCK) {
    const uint32_t p = p0 + threadIdx.x;
    const bool valid = p < npix;
    uint32_t c = 0;
    if (valid) {
      const uint32_t y = p / (uint32_t)w;
      c = af_pixel(f, h, w, m, (int)(p - y * (uint32_t)w), (int)y, fill);
    }
    const uint32_t next = __shfl_down(c, 1, 64);               // lane k = 3 never uses it
    const bool whole = aligned && p - k + 3 < npix;            // the same in the four lanes of a group
    if (whole) {
      if (k < 3) *reinterpret_cast<uint32_t*>(o + 3 * (size_t)p + k) = (c >> (8 * k)) | (next << (24 - 8 * k));
    } else if (valid) {
      o[3 * (size_t)p] = (uint8_t)c;
      o[3 * (size_t)p + 1] = (uint8_t)(c >> 8);
      o[3 * (size_t)p + 2] = (uint8_t)(c >> 16);
    }
  }
}

bool mats_finite(const double* m, int n, int* bad) {
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < 6; ++j)
      if (!isfinite(m[6 * (size_t)i + j])) {
        *bad = i;
        return false;
      }
  return true;
}

bool overlap(const void* a, const void* b, size_t bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y ? y - x < bytes : x - y < bytes;
}

}  // namespace

extern "C" int dxa_image_affine(const void* src, void* dst, int n, int h, int w, const double* mats, const double* mats_host,
                                uint32_t fill_rgb, dxa_stream_t stream) {
  DXA_CHECK_ARG(n >= 0 && h > 0 && w > 0, "dxa_image_affine: bad frame size");
  if (n == 0) return DXA_OK;
  DXA_CHECK_ARG(src && dst, "dxa_image_affine: null buffer");
  DXA_CHECK_ARG(mats && mats_host, "dxa_image_affine: null matrix table");
  DXA_CHECK_ARG(n <= 65535, "dxa_image_affine: too many frames per call");
  const int64_t npix = (int64_t)h * w;
  DXA_CHECK_ARG(npix < ((int64_t)1 << 31), "dxa_image_affine: frames of %d x %d are too large (2^31 pixels or more)", h, w);
  DXA_CHECK_ARG(!overlap(src, dst, (size_t)n * npix * 3), "dxa_image_affine: src and dst overlap, the warp is out of place");
  DXA_CHECK_ARG((uintptr_t)mats % 8 == 0, "dxa_image_affine: matrices must be 8-byte aligned");
  int bad = 0;
  DXA_CHECK_ARG(mats_finite(mats_host, n, &bad), "dxa_image_affine: frame %d: matrix is not finite", bad);
  // no more workgroups than the frame has blocks of work, and about 16384 over the batch (a few rounds of the chip's wave
  // slots): past that a workgroup strides through its frame
  int per_frame = dxa_cdiv(npix, PIX_PER_BLOCK);
  const int cap = dxa_cdiv(16384, n);
  if (per_frame > cap) per_frame = cap;
  hipLaunchKernelGGL(affine_k, dim3(per_frame, n), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)src, (uint8_t*)dst, h, w,
                     mats, fill_rgb & 0xffffffu);
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}

extern "C" int dxa_image_affine_host(const void* src, void* dst, int n, int h, int w, const double* mats, uint32_t fill_rgb) {
  DXA_CHECK_ARG(n >= 0 && h > 0 && w > 0, "dxa_image_affine_host: bad frame size");
  if (n == 0) return DXA_OK;
  DXA_CHECK_ARG(src && dst, "dxa_image_affine_host: null buffer");
  DXA_CHECK_ARG(mats, "dxa_image_affine_host: null matrix table");
  const size_t frame = (size_t)h * w * 3;
  DXA_CHECK_ARG(!overlap(src, dst, (size_t)n * frame), "dxa_image_affine_host: src and dst overlap, the warp is out of place");
  int bad = 0;
  DXA_CHECK_ARG(mats_finite(mats, n, &bad), "dxa_image_affine_host: frame %d: matrix is not finite", bad);
  for (int i = 0; i < n; ++i) {
    const uint8_t* f = (const uint8_t*)src + i * frame;
    uint8_t* o = (uint8_t*)dst + i * frame;
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) {
        const uint32_t c = af_pixel(f, h, w, mats + 6 * (size_t)i, x, y, fill_rgb & 0xffffffu);
        uint8_t* d = o + ((size_t)y * w + x) * 3;
        d[0] = (uint8_t)c;
        d[1] = (uint8_t)(c >> 8);
        d[2] = (uint8_t)(c >> 16);
      }
  }
  return DXA_OK;
}
