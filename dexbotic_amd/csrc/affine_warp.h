// Per-pixel arithmetic of the bilinear affine warp, as Pillow 12.2.0 computes Image.transform(size, AFFINE, m, BILINEAR,
// fillcolor) and with it Image.rotate(angle, BILINEAR), for host and device:
//   src/libImaging/Geometry.c   affine_transform        the source position of an output pixel
//                               bilinear_filter32RGB    BILINEAR_HEAD / BILINEAR_BODY, the result cast to UINT8
// One statement of it serves dxa_image_affine's kernel and dxa_image_affine_host, so the checks against Pillow
// (tests/test_affine_ref.py) run on the host over the very code the kernel executes.  Everything is IEEE double and every
// operation is separately rounded (Pillow is built without fused multiply-add): contraction is switched off per function.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#define DXA_AF_HD __host__ __device__ __forceinline__

// a + (b - a) * d: Geometry.c BILINEAR
DXA_AF_HD double af_lerp(double a, double b, double d) {
#pragma clang fp contract(off)
  const double diff = b - a;
  const double prod = diff * d;
  return a + prod;
}

// Output pixel (x, y) of an h x w frame `f` (uint8 RGB, interleaved) under the inverse matrix m[6]: r | g << 8 | b << 16.
// A position outside [0, w) x [0, h), a NaN one included, gives `fill`, so the float -> int conversions only ever see
// values inside the frame.
DXA_AF_HD uint32_t af_pixel(const uint8_t* f, int h, int w, const double* m, int x, int y, uint32_t fill) {
#pragma clang fp contract(off)
  const double xc = (double)x + 0.5, yc = (double)y + 0.5;
  const double ax = m[0] * xc, bx = m[1] * yc, ay = m[3] * xc, by = m[4] * yc;
  double xin = (ax + bx) + m[2];
  double yin = (ay + by) + m[5];
  if (!(xin >= 0.0 && xin < (double)w && yin >= 0.0 && yin < (double)h)) return fill;
  xin -= 0.5;
  yin -= 0.5;
  const double xf = floor(xin), yf = floor(yin);
  const int xi = (int)xf, yi = (int)yf;                     // in [-1, w - 1] and [-1, h - 1]
  const double dx = xin - xf, dy = yin - yf;
  const int x0 = xi < 0 ? 0 : xi;                           // XCLIP(x), XCLIP(x + 1)
  const int x1 = xi + 1 > w - 1 ? w - 1 : xi + 1;
  const uint8_t* r0 = f + (size_t)(yi < 0 ? 0 : yi) * w * 3;
  const bool below = yi + 1 < h;                            // yi + 1 >= 0 always
  const uint8_t* r1 = below ? f + (size_t)(yi + 1) * w * 3 : r0;
  uint32_t out = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double v1 = af_lerp((double)r0[3 * x0 + c], (double)r0[3 * x1 + c], dx);
    const double v2 = below ? af_lerp((double)r1[3 * x0 + c], (double)r1[3 * x1 + c], dx) : v1;
    out |= (uint32_t)(int)af_lerp(v1, v2, dy) << (8 * c);   // (UINT8)v: truncation
  }
  return out;
}
