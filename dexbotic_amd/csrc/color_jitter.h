// Per-pixel colour arithmetic of the ColorJitter augmentation, as Pillow 12.2.0 computes it, for host and device:
//   Image.convert('L')                      src/libImaging/Convert.c   rgb2l
//   ImageEnhance.Brightness/Contrast/Color  src/libImaging/Blend.c     deg + f * (img - deg) in float
//   Image.convert('HSV') and back           src/libImaging/Convert.c   rgb2hsv_row / hsv2rgb_row
// One statement of it serves dxa_color_jitter's kernels and dxa_color_jitter_pixels_host, so the exhaustive checks against
// Pillow (tests/test_augment_ref.py) run on the host over the very code the kernels execute.  Every float operation is a
// separately rounded IEEE operation (Pillow is built without fused multiply-add): contraction is switched off per function.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/dexbotic_amd.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define DXA_CJ_DIV32(a, b) __fdiv_rn((a), (b))   // correctly rounded, whatever the division flags of the build
#else
#define DXA_CJ_DIV32(a, b) ((a) / (b))
#endif
#define DXA_CJ_FLOOR32(a) floorf(a)
#define DXA_CJ_HD __host__ __device__ __forceinline__

struct cj_rgb {
  int r, g, b;
};

DXA_CJ_HD int cj_grey(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// Image.blend(deg, img, f) for one channel: truncation when 0 <= f <= 1, clipped first otherwise
DXA_CJ_HD int cj_blend(int deg, int v, float f) {
#pragma clang fp contract(off)
  const float prod = f * (float)(v - deg);
  const float t = (float)deg + prod;
  if (f >= 0.f && f <= 1.f) return (int)t;
  return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}

DXA_CJ_HD int cj_round8(float x) {
#pragma clang fp contract(off)
  const float y = DXA_CJ_FLOOR32(x + 0.5f);
  return y < 0.f ? 0 : (y > 255.f ? 255 : (int)y);
}

// rgb2hsv_row followed by H += shift (mod 256) and hsv2rgb_row
DXA_CJ_HD cj_rgb cj_hue_shift(cj_rgb c, int shift) {
#pragma clang fp contract(off)
  const int mx = c.r > c.g ? (c.r > c.b ? c.r : c.b) : (c.g > c.b ? c.g : c.b);
  const int mn = c.r < c.g ? (c.r < c.b ? c.r : c.b) : (c.g < c.b ? c.g : c.b);
  if (mx == mn) return c;   // s = 0: (v, v, v) whatever the hue
  const float cr = (float)(mx - mn);
  const int s = (int)((double)DXA_CJ_DIV32(cr, (float)mx) * 255.0);
  // float ratios; the sums, the division by 6 and the fmod in double; h is stored as float in between (exact on all 2^24 colours)
  const double rc = (double)DXA_CJ_DIV32((float)(mx - c.r), cr);
  const double gc = (double)DXA_CJ_DIV32((float)(mx - c.g), cr);
  const double bc = (double)DXA_CJ_DIV32((float)(mx - c.b), cr);
  const float hs = (float)(c.r == mx ? bc - gc : (c.g == mx ? 2.0 + rc - bc : 4.0 + gc - rc));
  double x = (double)hs / 6.0 + 1.0;   // in [5/6, 11/6]: fmod(x, 1.0) is one exact subtraction
  if (x >= 1.0) x -= 1.0;
  const int h = ((int)((double)(float)x * 255.0) + shift) & 255;
  if (s == 0) return cj_rgb{mx, mx, mx};
  const float v = (float)mx;
  const float fs = DXA_CJ_DIV32((float)s, 255.f);
  const float f0 = DXA_CJ_DIV32((float)h * 6.f, 255.f);
  const float fi = DXA_CJ_FLOOR32(f0);
  const float f = f0 - fi;
  const int p = cj_round8(v * (1.f - fs));
  const int q = cj_round8(v * (1.f - fs * f));
  const int t = cj_round8(v * (1.f - fs * (1.f - f)));
  switch ((int)fi % 6) {
    case 0: return cj_rgb{mx, t, p};
    case 1: return cj_rgb{q, mx, p};
    case 2: return cj_rgb{p, mx, t};
    case 3: return cj_rgb{p, q, mx};
    case 4: return cj_rgb{t, p, mx};
    default: return cj_rgb{mx, p, q};
  }
}

DXA_CJ_HD int cj_hue_levels(float hue) {
#pragma clang fp contract(off)
  return (int)(hue * 255.f);   // trunc, as numpy's uint8 cast of hue * 255
}

DXA_CJ_HD cj_rgb cj_apply_op(cj_rgb c, int op, const dxa_jitter_params& jp, int m) {
  switch (op) {
    case DXA_JITTER_BRIGHTNESS:
      return cj_rgb{cj_blend(0, c.r, jp.brightness), cj_blend(0, c.g, jp.brightness), cj_blend(0, c.b, jp.brightness)};
    case DXA_JITTER_CONTRAST:
      return cj_rgb{cj_blend(m, c.r, jp.contrast), cj_blend(m, c.g, jp.contrast), cj_blend(m, c.b, jp.contrast)};
    case DXA_JITTER_SATURATION: {
      const int l = cj_grey(c.r, c.g, c.b);
      return cj_rgb{cj_blend(l, c.r, jp.saturation), cj_blend(l, c.g, jp.saturation), cj_blend(l, c.b, jp.saturation)};
    }
    default:
      return cj_hue_shift(c, cj_hue_levels(jp.hue));
  }
}

// the ops that come before the contrast op in the frame's order: what the frame's mean L is taken over
DXA_CJ_HD cj_rgb cj_before_contrast(cj_rgb c, const dxa_jitter_params& jp) {
  for (int i = 0; i < 4 && jp.order[i] != DXA_JITTER_CONTRAST; ++i) c = cj_apply_op(c, jp.order[i], jp, 0);
  return c;
}

DXA_CJ_HD cj_rgb cj_all_ops(cj_rgb c, const dxa_jitter_params& jp, int m) {
  for (int i = 0; i < 4; ++i) c = cj_apply_op(c, jp.order[i], jp, m);
  return c;
}
