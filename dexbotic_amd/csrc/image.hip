// Device-side image preprocessing: uint8 RGB frames -> [expand to square] -> bicubic
// resize -> center crop -> rescale / normalise -> planar fp32 / bf16, bit-exact with what the reference gets from
// Pillow's 8-bit resampler under the CLIP image processor:
//   dexbotic/data/dataset/rgb_preprocess.py:13-44  PreprocessRGB.__call__ / expand2square
//   dexbotic/model/dexbotic_arch.py:498-529        process_images
//   Pillow 12.2.0 src/libImaging/Resample.c        precompute_coeffs, normalize_coeffs_8bpc, ImagingResample*_8bpc
// Byte work, HBM/latency bound: two launches per batch of frames (horizontal pass into a uint8 scratch image that
// holds only the rows and columns the crop needs, then vertical pass fused with crop + normalise + HWC->CHW).
#include <math.h>

#include <vector>

#include "common.h"

namespace {

constexpr int PRECISION_BITS = 32 - 8 - 2;   // Resample.c

double bicubic_filter(double x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

double bilinear_filter(double x) {
  if (x < 0.0) x = -x;
  return x < 1.0 ? 1.0 - x : 0.0;
}

double filter_support(int filter) { return filter == DXA_FILTER_BILINEAR ? 1.0 : 2.0; }

int ksize_for(int in_size, int out_size, int filter = DXA_FILTER_BICUBIC) {
  double filterscale = (double)in_size / out_size;
  if (filterscale < 1.0) filterscale = 1.0;
  return (int)ceil(filter_support(filter) * filterscale) * 2 + 1;
}

__device__ __forceinline__ uint8_t clip8(int v) {
  v >>= PRECISION_BITS;
  return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// clip8 as one byte of a dword that is put together with shifts.  The value goes through an empty asm so that hipcc does not fuse
// two neighbouring clips into v_ashr_pk_u8_i32: on the MI355X that instruction was seen to leave bits 16-31 of its destination
// as they were (here: the accumulator), while the code around it ORs the other two bytes in as if they were zero.
__device__ __forceinline__ uint32_t clip8_word(int v) {
  uint32_t b = clip8(v);
  asm volatile("" : "+v"(b));
  return b;
}

struct ImgP {
  const uint8_t* src;
  int n, h, w;            // source frames
  int ph, pw, off_y, off_x;   // padded (virtual) frame and where the source sits in it
  uint32_t bg;            // r | g << 8 | b << 16
  int row0, rows;         // padded rows the vertical pass reads: [row0, row0 + rows)
  int crop_top, crop_left, out_h, out_w;
  const int32_t *hb, *hk;
  int hks;
  const int32_t *vb, *vk;
  int vks;
  uint8_t* tmp;           // [n, rows, out_w, 3]
  void* out;              // [n, 3, out_h, out_w]
  uint8_t* out_u8;        // optional [n, out_h, out_w, 3]
  double scale;
  float mean[3], stdv[3];
};

// One workgroup per (needed padded row, frame): the padded row is staged in LDS, then out_w * 3 taps-sums.
__global__ __launch_bounds__(256) void image_hpass_k(const ImgP p) {
  extern __shared__ uint8_t row[];
  const int r = p.row0 + blockIdx.x, img = blockIdx.y;
  const int sy = r - p.off_y;
  const bool in_y = sy >= 0 && sy < p.h;
  const uint8_t* s = p.src + ((size_t)img * p.h + (in_y ? sy : 0)) * p.w * 3;
  const int nb = p.pw * 3;
  for (int e = threadIdx.x; e < nb; e += 256) {
    const int x = e / 3, c = e - 3 * x, sx = x - p.off_x;
    row[e] = (in_y && sx >= 0 && sx < p.w) ? s[sx * 3 + c] : (uint8_t)(p.bg >> (8 * c));
  }
  __syncthreads();
  uint8_t* d = p.tmp + ((size_t)img * p.rows + blockIdx.x) * p.out_w * 3;
  for (int e = threadIdx.x; e < p.out_w * 3; e += 256) {
    const int xo = e / 3, c = e - 3 * xo, x = xo + p.crop_left;
    if (p.hb == nullptr) {
      d[e] = row[x * 3 + c];
      continue;
    }
    const int xmin = p.hb[2 * x], cnt = p.hb[2 * x + 1];
    const int32_t* k = p.hk + (size_t)x * p.hks;
    int acc = 1 << (PRECISION_BITS - 1);
    for (int i = 0; i < cnt; ++i) acc += (int)row[(xmin + i) * 3 + c] * k[i];
    d[e] = clip8(acc);
  }
}

// One workgroup per (output row, frame); threads run over (channel, x) so the planar stores are contiguous.
template <typename TO>
__global__ __launch_bounds__(256) void image_vpass_k(const ImgP p) {
  const int yo = blockIdx.x, img = blockIdx.y, y = yo + p.crop_top;
  const uint8_t* t = p.tmp + (size_t)img * p.rows * p.out_w * 3;
  int ymin = y, cnt = 1;
  const int32_t* k = nullptr;
  if (p.vb) {
    ymin = p.vb[2 * y];
    cnt = p.vb[2 * y + 1];
    k = p.vk + (size_t)y * p.vks;
  }
  for (int e = threadIdx.x; e < 3 * p.out_w; e += 256) {
    const int c = e / p.out_w, x = e - c * p.out_w;
    const uint8_t* col = t + (size_t)(ymin - p.row0) * p.out_w * 3 + x * 3 + c;
    uint8_t v;
    if (k) {
      int acc = 1 << (PRECISION_BITS - 1);
      for (int i = 0; i < cnt; ++i) acc += (int)col[(size_t)i * p.out_w * 3] * k[i];
      v = clip8(acc);
    } else {
      v = col[0];
    }
    if (p.out_u8) p.out_u8[(((size_t)img * p.out_h + yo) * p.out_w + x) * 3 + c] = v;
    // transformers rescale(): uint8 -> float64 * scale -> float32; normalize(): (x - mean) / std in float32
    const float f = (float)((double)v * p.scale);
    const float o = __fdiv_rn(__fsub_rn(f, p.mean[c]), p.stdv[c]);
    stf<TO>(reinterpret_cast<TO*>(p.out) + (((size_t)img * 3 + c) * p.out_h + yo) * p.out_w + x, o);
  }
}

// ---- crop + bilinear resize of the training augmentations: every frame has its own square box, the tables are per side
struct CropP {
  const uint8_t* src;
  int h, w, off_y, off_x;   // source frames and where they sit in the padded (virtual) frame
  uint32_t bg;
  const int32_t* boxes;     // [n][4] = x0, y0, c, table
  int S, ks, tmp_rows;
  const int32_t *bounds, *taps;
  uint8_t* tmp;             // [n, tmp_rows, S, 3]
  uint8_t* out;             // [n, S, S, 3]
};

// One workgroup per (row of the box, frame).  The in-frame bytes of the row come in as aligned dwords (a lane per dword, the
// interleaved RGB bytes as they lie), shifted in LDS so that byte e of the box row sits at row[base + e]; the virtual pad is
// filled around them.  (The first and last dword may hold up to 3 bytes of the neighbouring row, or of the same aligned dword just
// outside the buffer, which an aligned load cannot fault on; they land in LDS slack or under the pad fill.)  Then S * 3 tap sums, four bytes per lane when the rows of tmp are dword-aligned (VEC).
template <bool VEC>
__global__ __launch_bounds__(256) void crop_hpass_k(const CropP p) {
  extern __shared__ __attribute__((aligned(16))) uint8_t row[];
  const int img = blockIdx.y;
  const int32_t* bx = p.boxes + 4 * (size_t)img;
  const int x0 = bx[0], y0 = bx[1], c = bx[2], table = bx[3];
  if ((int)blockIdx.x >= c) return;                      // uniform per workgroup
  const int sy = y0 + (int)blockIdx.x - p.off_y;
  const bool in_y = sy >= 0 && sy < p.h;
  // box columns [xa, xb) lie inside the source frame
  int xa = p.off_x - x0, xb = p.off_x + p.w - x0;
  xa = xa < 0 ? 0 : (xa > c ? c : xa);
  xb = xb < 0 ? 0 : (xb > c ? c : xb);
  if (!in_y || xb < xa) xb = xa;
  const uint8_t* g = p.src + (((size_t)img * p.h + (in_y ? sy : 0)) * p.w + (x0 + xa - p.off_x)) * 3;
  const int lead = (int)((uintptr_t)g & 3);
  const int base = (lead - 3 * xa) & 3;
  if (xb > xa) {
    const uint32_t* g4 = reinterpret_cast<const uint32_t*>(g - lead);
    uint32_t* r4 = reinterpret_cast<uint32_t*>(row + base + 3 * xa - lead);
    const int nd = (lead + 3 * (xb - xa) + 3) >> 2;
    for (int i = threadIdx.x; i < nd; i += 256) r4[i] = g4[i];
  }
  __syncthreads();                                        // the edge dwords overlap up to 3 pad bytes on either side
  for (int e = threadIdx.x; e < 3 * c; e += 256) {
    const int x = e / 3;
    if (x < xa || x >= xb) row[base + e] = (uint8_t)(p.bg >> (8 * (e - 3 * x)));
  }
  __syncthreads();
  const uint8_t* r = row + base;
  const int32_t* b = p.bounds + (size_t)table * p.S * 2;
  const int32_t* kk = p.taps + (size_t)table * p.S * p.ks;
  uint8_t* d = p.tmp + ((size_t)img * p.tmp_rows + blockIdx.x) * p.S * 3;
  auto tap_sum = [&](int e) {
    const int xo = e / 3, ch = e - 3 * xo;
    const int xmin = b[2 * xo], cnt = b[2 * xo + 1];
    const int32_t* k = kk + (size_t)xo * p.ks;
    int acc = 1 << (PRECISION_BITS - 1);
    for (int i = 0; i < cnt; ++i) acc += (int)r[(xmin + i) * 3 + ch] * k[i];
    return clip8_word(acc);
  };
  if (VEC) {
    for (int e = 4 * threadIdx.x; e < 3 * p.S; e += 4 * 256)
      *reinterpret_cast<uint32_t*>(d + e) = tap_sum(e) | (tap_sum(e + 1) << 8) | (tap_sum(e + 2) << 16) | (tap_sum(e + 3) << 24);
  } else {
    for (int e = threadIdx.x; e < 3 * p.S; e += 256) d[e] = (uint8_t)tap_sum(e);
  }
}

// One workgroup per (output row, frame); a lane owns four consecutive bytes of the row (VEC) and reads a dword of tmp per tap.
template <bool VEC>
__global__ __launch_bounds__(256) void crop_vpass_k(const CropP p) {
  const int yo = blockIdx.x, img = blockIdx.y;
  const int table = p.boxes[4 * (size_t)img + 3];
  const int ymin = p.bounds[((size_t)table * p.S + yo) * 2], cnt = p.bounds[((size_t)table * p.S + yo) * 2 + 1];
  const int32_t* k = p.taps + ((size_t)table * p.S + yo) * p.ks;
  const size_t stride = (size_t)p.S * 3;
  const uint8_t* t = p.tmp + ((size_t)img * p.tmp_rows + ymin) * stride;
  uint8_t* o = p.out + ((size_t)img * p.S + yo) * stride;
  if (VEC) {
    for (int e = 4 * threadIdx.x; e < 3 * p.S; e += 4 * 256) {
      int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0, a3 = a0;
      for (int i = 0; i < cnt; ++i) {
        const uint32_t v = *reinterpret_cast<const uint32_t*>(t + (size_t)i * stride + e);
        const int w = k[i];
        a0 += (int)(v & 255) * w; a1 += (int)((v >> 8) & 255) * w; a2 += (int)((v >> 16) & 255) * w; a3 += (int)(v >> 24) * w;
      }
      *reinterpret_cast<uint32_t*>(o + e) =
          clip8_word(a0) | (clip8_word(a1) << 8) | (clip8_word(a2) << 16) | (clip8_word(a3) << 24);
    }
  } else {
    for (int e = threadIdx.x; e < 3 * p.S; e += 256) {
      int acc = 1 << (PRECISION_BITS - 1);
      for (int i = 0; i < cnt; ++i) acc += (int)t[(size_t)i * stride + e] * k[i];
      o[e] = clip8(acc);
    }
  }
}

}  // namespace

extern "C" int dxa_resample_ksize(int in_size, int out_size) {
  if (in_size <= 0 || out_size <= 0) return 0;
  return ksize_for(in_size, out_size);
}

extern "C" int dxa_resample_ksize_filter(int in_size, int out_size, int filter) {
  if (in_size <= 0 || out_size <= 0 || (filter != DXA_FILTER_BICUBIC && filter != DXA_FILTER_BILINEAR)) return 0;
  return ksize_for(in_size, out_size, filter);
}

extern "C" int dxa_resample_coeffs(int in_size, int out_size, int filter, int32_t* bounds, int32_t* kk) {
  DXA_CHECK_ARG(in_size > 0 && out_size > 0, "dxa_resample_coeffs: sizes must be positive");
  DXA_CHECK_ARG(filter == DXA_FILTER_BICUBIC || filter == DXA_FILTER_BILINEAR,
                "dxa_resample_coeffs: only DXA_FILTER_BICUBIC and DXA_FILTER_BILINEAR are implemented");
  DXA_CHECK_ARG(bounds && kk, "dxa_resample_coeffs: null table");
  // Resample.c precompute_coeffs (in0 = 0, in1 = in_size), then normalize_coeffs_8bpc
  double scale = (double)in_size / out_size, filterscale = scale;
  if (filterscale < 1.0) filterscale = 1.0;
  const double support = filter_support(filter) * filterscale;
  const int ksize = (int)ceil(support) * 2 + 1;
  const double ss = 1.0 / filterscale;
  std::vector<double> k(ksize);
  for (int xx = 0; xx < out_size; ++xx) {
    const double center = (xx + 0.5) * scale;
    double ww = 0.0;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    for (int x = 0; x < xmax; ++x) {
      const double arg = (x + xmin - center + 0.5) * ss;
      const double w = filter == DXA_FILTER_BILINEAR ? bilinear_filter(arg) : bicubic_filter(arg);
      k[x] = w;
      ww += w;
    }
    for (int x = 0; x < xmax; ++x)
      if (ww != 0.0) k[x] /= ww;
    int32_t* o = kk + (size_t)xx * ksize;
    for (int x = 0; x < ksize; ++x) {
      const double v = x < xmax ? k[x] : 0.0;
      o[x] = v < 0 ? (int32_t)(-0.5 + v * (1 << PRECISION_BITS)) : (int32_t)(0.5 + v * (1 << PRECISION_BITS));
    }
    bounds[2 * xx] = xmin;
    bounds[2 * xx + 1] = xmax;
  }
  return DXA_OK;
}

extern "C" int dxa_image_preprocess(const dxa_image_desc* d, dxa_stream_t stream) {
  DXA_CHECK_ARG(d != nullptr, "dxa_image_preprocess: null desc");
  DXA_CHECK_ARG(d->n >= 0 && d->h > 0 && d->w > 0, "dxa_image_preprocess: bad frame size");
  if (d->n == 0) return DXA_OK;
  DXA_CHECK_ARG(d->src && d->tmp && d->out, "dxa_image_preprocess: null buffer");
  DXA_CHECK_ARG(d->out_dtype == DXA_F32 || d->out_dtype == DXA_BF16, "dxa_image_preprocess: bad out_dtype");
  ImgP p;
  memset(&p, 0, sizeof(p));
  p.src = (const uint8_t*)d->src; p.n = d->n; p.h = d->h; p.w = d->w;
  p.ph = d->h; p.pw = d->w;
  if (d->pad) {   // expand2square: the frame is centred along the short side (integer division as the reference)
    p.ph = p.pw = d->h > d->w ? d->h : d->w;
    p.off_y = (p.ph - d->h) / 2;
    p.off_x = (p.pw - d->w) / 2;
  }
  p.bg = (uint32_t)d->bg[0] | ((uint32_t)d->bg[1] << 8) | ((uint32_t)d->bg[2] << 16);
  DXA_CHECK_ARG(d->res_h > 0 && d->res_w > 0, "dxa_image_preprocess: bad resize target");
  DXA_CHECK_ARG((d->hb != nullptr) == (d->res_w != p.pw) && (d->vb != nullptr) == (d->res_h != p.ph),
                "dxa_image_preprocess: a pass has tables exactly when it changes the size (%dx%d -> %dx%d)", p.ph, p.pw,
                d->res_h, d->res_w);
  DXA_CHECK_ARG(!d->hb || d->hks == ksize_for(p.pw, d->res_w), "dxa_image_preprocess: horizontal table stride");
  DXA_CHECK_ARG(!d->vb || d->vks == ksize_for(p.ph, d->res_h), "dxa_image_preprocess: vertical table stride");
  DXA_CHECK_ARG(d->crop_top >= 0 && d->crop_left >= 0 && d->out_h > 0 && d->out_w > 0 &&
                    d->crop_top + d->out_h <= d->res_h && d->crop_left + d->out_w <= d->res_w,
                "dxa_image_preprocess: crop window outside the resized frame");
  DXA_CHECK_ARG(d->row0 >= 0 && d->rows > 0 && d->row0 + d->rows <= p.ph, "dxa_image_preprocess: bad scratch row range");
  DXA_CHECK_ARG((size_t)p.pw * 3 <= 64 * 1024, "dxa_image_preprocess: frames wider than 21845 px are not supported");
  DXA_CHECK_ARG(d->n <= 65535, "dxa_image_preprocess: too many frames per call");
  p.row0 = d->row0; p.rows = d->rows;
  p.crop_top = d->crop_top; p.crop_left = d->crop_left; p.out_h = d->out_h; p.out_w = d->out_w;
  p.hb = d->hb; p.hk = d->hk; p.hks = d->hks;
  p.vb = d->vb; p.vk = d->vk; p.vks = d->vks;
  p.tmp = (uint8_t*)d->tmp; p.out = d->out; p.out_u8 = (uint8_t*)d->out_u8;
  p.scale = d->rescale;
  for (int c = 0; c < 3; ++c) { p.mean[c] = d->mean[c]; p.stdv[c] = d->std[c]; }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(image_hpass_k, dim3(p.rows, p.n), dim3(256), (size_t)p.pw * 3, st, p);
  DXA_CHECK_LAUNCH();
  if (d->out_dtype == DXA_F32) hipLaunchKernelGGL(image_vpass_k<float>, dim3(p.out_h, p.n), dim3(256), 0, st, p);
  else hipLaunchKernelGGL(image_vpass_k<bf16_t>, dim3(p.out_h, p.n), dim3(256), 0, st, p);
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}

extern "C" int dxa_image_crop_resize(const void* src, int n, int h, int w, int pad, uint32_t bg_rgb, const int32_t* boxes,
                                     const int32_t* boxes_host, int S, const int32_t* bounds, const int32_t* taps,
                                     const int32_t* table_sides_host, int n_tables, int ks, void* tmp, int tmp_rows, void* out,
                                     dxa_stream_t stream) {
  DXA_CHECK_ARG(n >= 0 && h > 0 && w > 0, "dxa_image_crop_resize: bad frame size");
  DXA_CHECK_ARG(S > 0, "dxa_image_crop_resize: bad output size");
  if (n == 0) return DXA_OK;
  DXA_CHECK_ARG(src && tmp && out, "dxa_image_crop_resize: null buffer");
  DXA_CHECK_ARG(boxes && boxes_host, "dxa_image_crop_resize: null box table");
  DXA_CHECK_ARG(bounds && taps && table_sides_host && n_tables > 0, "dxa_image_crop_resize: null tap tables");
  DXA_CHECK_ARG(n <= 65535, "dxa_image_crop_resize: too many frames per call");
  CropP p;
  memset(&p, 0, sizeof(p));
  int ph = h, pw = w;
  if (pad) {   // expand2square, as dxa_image_preprocess
    ph = pw = h > w ? h : w;
    p.off_y = (ph - h) / 2;
    p.off_x = (pw - w) / 2;
  }
  int cmax = 0;
  for (int t = 0; t < n_tables; ++t) {
    const int c = table_sides_host[t];
    DXA_CHECK_ARG(c > 0 && ks >= ksize_for(c, S, DXA_FILTER_BILINEAR),
                  "dxa_image_crop_resize: table %d (side %d -> %d) needs a tap stride of %d, got %d", t, c, S,
                  c > 0 ? ksize_for(c, S, DXA_FILTER_BILINEAR) : 0, ks);
  }
  for (int i = 0; i < n; ++i) {
    const int x0 = boxes_host[4 * i], y0 = boxes_host[4 * i + 1], c = boxes_host[4 * i + 2], t = boxes_host[4 * i + 3];
    DXA_CHECK_ARG(c > 0 && x0 >= 0 && y0 >= 0 && (int64_t)x0 + c <= pw && (int64_t)y0 + c <= ph,
                  "dxa_image_crop_resize: box %d (x0 %d, y0 %d, side %d) outside the %dx%d frame", i, x0, y0, c, ph, pw);
    DXA_CHECK_ARG(t >= 0 && t < n_tables && table_sides_host[t] == c,
                  "dxa_image_crop_resize: box %d of side %d names a table built for another side", i, c);
    if (c > cmax) cmax = c;
  }
  DXA_CHECK_ARG(tmp_rows >= cmax, "dxa_image_crop_resize: scratch of %d rows, the largest box has %d", tmp_rows, cmax);
  DXA_CHECK_ARG((size_t)cmax * 3 + 8 <= 64 * 1024, "dxa_image_crop_resize: boxes wider than 21842 px are not supported");
  DXA_CHECK_ARG(S <= 65535 && cmax <= 65535, "dxa_image_crop_resize: side too large");
  p.src = (const uint8_t*)src; p.h = h; p.w = w; p.bg = bg_rgb;
  p.boxes = boxes; p.S = S; p.ks = ks; p.tmp_rows = tmp_rows;
  p.bounds = bounds; p.taps = taps;
  p.tmp = (uint8_t*)tmp; p.out = (uint8_t*)out;
  const bool vec = S % 4 == 0 && (uintptr_t)tmp % 4 == 0 && (uintptr_t)out % 4 == 0;
  const size_t lds = ((size_t)cmax * 3 + 8 + 3) & ~(size_t)3;
  hipStream_t st = (hipStream_t)stream;
  if (vec) hipLaunchKernelGGL(crop_hpass_k<true>, dim3(cmax, n), dim3(256), lds, st, p);
  else hipLaunchKernelGGL(crop_hpass_k<false>, dim3(cmax, n), dim3(256), lds, st, p);
  DXA_CHECK_LAUNCH();
  if (vec) hipLaunchKernelGGL(crop_vpass_k<true>, dim3(S, n), dim3(256), 0, st, p);
  else hipLaunchKernelGGL(crop_vpass_k<false>, dim3(S, n), dim3(256), 0, st, p);
  DXA_CHECK_LAUNCH();
  return DXA_OK;
}
