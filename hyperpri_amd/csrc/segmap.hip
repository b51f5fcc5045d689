// Colour-coded segmentation maps on the device (hyperpri_amd/evaluate.py): the per-pixel arithmetic of eval_color_segmaps
// (src/PLTrainer.py:219-267) without matplotlib -- three bands of the image as a gamma-corrected pseudo-RGB picture
// (:236-240), the prediction / ground-truth classes painted in the colour-blind palette (:243-258), both blended as
// `imshow(img); imshow(overlay, alpha)` blends them (:263-264) -- written as 3 bytes per pixel.
//
//   v_k    = image[n, band_k, y, x], NaN -> 0, clamped to [0, 1]                                  (k = R, G, B)
//   base_k = gamma == 1 ? v_k : powf(v_k, inv_gamma)                                             (:239 `img ** (1 / 2.2)`)
//   p      = is_logits ? 1 / (1 + expf(-pred)) : pred;   s = p > threshold;   g = ((int)mask) != 0      (= seg_counts_kernel)
//   class  = s + 2 g:  0 neither, 1 prediction only, 2 truth only, 3 both    (:255-258: truth overwrites prediction,
//                                                                              agreement overwrites both)
//   over   = class ? palette[class - 1] : (0, 0, 0);   out_k = alpha * over_k + (1 - alpha) * base_k
//   rgb_k  = (uint8)(out_k * 255 + 0.5f)
//
// The clamp and the NaN rule are this library's: the reference hands the raw values to matplotlib, which clips (and warns);
// the two differ only where the reference would hand it a NaN or a value outside [0, 1].
//
// The image is addressed by four element strides, so one kernel reads the zero-padded channels-last views CubeCache /
// CubeStager hand out (band stride 1, pixel stride cs) and a plain contiguous (N, C, h, w) tensor.  Memory-bound and tiny:
// one lane owns four consecutive pixels of a row -- 16-byte loads of its four predictions and mask values where the quad is
// 16-byte aligned, its twelve band loads issued before any arithmetic, 12 contiguous bytes out -- and a per-pixel tail
// covers w % 4.  No LDS, no atomics; the grid is capped at eight workgroups per CU with a grid-stride loop.
#include "tail_helpers.h"

#define SEGMAP_THREADS 256

struct SegmapArgs {
  const float* image;
  long long sn, sc, sy, sx;             // element strides of image[n, band, y, x]
  int band[3];
  const float *pred, *mask;             // (N, h, w) contiguous
  int N, h, w;
  float threshold;
  int is_logits, gamma_is_one;
  float inv_gamma, alpha;
  float palette[9];                     // prediction only, truth only, both
  unsigned char *rgb, *classes;         // (N, h, w, 3); (N, h, w) or nullptr
  int vec;                              // pred / mask / rgb / classes pointers allow the 16- and 4-byte accesses of an aligned quad
};

__device__ __forceinline__ int segmap_class(float x, float m, float thr, int is_logits) {
  const float p = is_logits ? 1.f / (1.f + expf(-x)) : x;
  const int s = p > thr, g = ((int)m) != 0;
  return s + 2 * g;
}

__device__ __forceinline__ float segmap_base(float v, int gamma_is_one, float inv_gamma) {
  v = v > 0.f ? fminf(v, 1.f) : 0.f;                                 // NaN and negatives -> 0
  return gamma_is_one ? v : powf(v, inv_gamma);
}

__device__ __forceinline__ unsigned segmap_round(float out) { return (unsigned)(out * 255.f + 0.5f); }

__device__ __forceinline__ unsigned segmap_blend(float alpha, float over, float base) {
  const float out = alpha * over + (1.f - alpha) * base;
  return segmap_round(out);
}

// the three bands of `cnt` (compile-time) consecutive pixels of a row, all loads issued before any arithmetic
template <int CNT>
__device__ __forceinline__ void segmap_bands(const float* img, const int (&band)[3], long long sc, long long sx, float (&v)[3][CNT]) {
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int j = 0; j < CNT; ++j) v[k][j] = img[band[k] * sc + j * sx];
}

__device__ __forceinline__ unsigned segmap_level(const SegmapArgs& a, int cls, int k, float base) {
  // (selects, not an indexed read: k is a compile-time constant at every call, the class is per lane)
  const float over = cls == 0 ? 0.f : cls == 1 ? a.palette[k] : cls == 2 ? a.palette[3 + k] : a.palette[6 + k];
  return segmap_blend(a.alpha, over, base);
}

__global__ __launch_bounds__(SEGMAP_THREADS) void segmap_overlay_kernel(const SegmapArgs a) {
  const int wq = (a.w + 3) >> 2;                                      // pixel quads per row, the last one possibly short
  const long long items = (long long)a.N * a.h * wq;
  for (long long it = (long long)blockIdx.x * SEGMAP_THREADS + threadIdx.x; it < items; it += (long long)gridDim.x * SEGMAP_THREADS) {
    const long long r = it / wq;                                      // row (n, y)
    const int x0 = (int)(it - r * wq) * 4;
    const long long n = r / a.h;
    const int y = (int)(r - n * a.h);
    const long long pix = r * a.w + x0;                               // first pixel of the quad in pred / mask / rgb / classes
    const float* img = a.image + n * a.sn + y * a.sy + x0 * a.sx;
    if (x0 + 4 <= a.w) {
      float x[4], m[4], v[3][4];
      if (a.vec && (pix & 3) == 0) {
        const f32x4 xv = *reinterpret_cast<const f32x4*>(a.pred + pix);
        const f32x4 mv = *reinterpret_cast<const f32x4*>(a.mask + pix);
#pragma unroll
        for (int j = 0; j < 4; ++j) { x[j] = xv[j]; m[j] = mv[j]; }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) { x[j] = a.pred[pix + j]; m[j] = a.mask[pix + j]; }
      }
      segmap_bands<4>(img, a.band, a.sc, a.sx, v);
      unsigned char o[12], c[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int cls = segmap_class(x[j], m[j], a.threshold, a.is_logits);
        c[j] = (unsigned char)cls;
#pragma unroll
        for (int k = 0; k < 3; ++k) o[3 * j + k] = (unsigned char)segmap_level(a, cls, k, segmap_base(v[k][j], a.gamma_is_one, a.inv_gamma));
      }
      unsigned char* d = a.rgb + 3 * pix;
      if (a.vec && (pix & 3) == 0) {                                  // 3 * pix is a multiple of 4 as well: three aligned words
        unsigned* dw = reinterpret_cast<unsigned*>(d);
#pragma unroll
        for (int q = 0; q < 3; ++q)
          dw[q] = (unsigned)o[4 * q] | ((unsigned)o[4 * q + 1] << 8) | ((unsigned)o[4 * q + 2] << 16) | ((unsigned)o[4 * q + 3] << 24);
        if (a.classes)
          *reinterpret_cast<unsigned*>(a.classes + pix) = (unsigned)c[0] | ((unsigned)c[1] << 8) | ((unsigned)c[2] << 16) | ((unsigned)c[3] << 24);
      } else {
#pragma unroll
        for (int q = 0; q < 12; ++q) d[q] = o[q];
        if (a.classes) {
#pragma unroll
          for (int j = 0; j < 4; ++j) a.classes[pix + j] = c[j];
        }
      }
    } else {
      for (int j = 0; x0 + j < a.w; ++j) {                            // the row's last w % 4 pixels
        const float x = a.pred[pix + j], m = a.mask[pix + j];
        float v[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = img[a.band[k] * a.sc + j * a.sx];
        const int cls = segmap_class(x, m, a.threshold, a.is_logits);
#pragma unroll
        for (int k = 0; k < 3; ++k)
          a.rgb[3 * (pix + j) + k] = (unsigned char)segmap_level(a, cls, k, segmap_base(v[k], a.gamma_is_one, a.inv_gamma));
        if (a.classes) a.classes[pix + j] = (unsigned char)cls;
      }
    }
  }
}

// image: fp32, element (n, band, y, x) at image[n*sn + band*sc + y*sy + x*sx] (strides in elements, >= 0), C bands.
// pred, mask: contiguous (N, h, w) fp32.  rgb: (N, h, w, 3) uint8.  classes: (N, h, w) uint8 or null.
// gamma > 0 and inv_gamma = 1 / gamma as the caller's language forms it (Python: float(1 / 2.2)); the palette holds
// prediction-only, truth-only and both as R, G, B in [0, 1].
extern "C" int hpri_segmap_overlay(const float* image, long long sn, long long sc, long long sy, long long sx, int C, int band_r,
                                   int band_g, int band_b, const float* pred, const float* mask, int N, int h, int w,
                                   float threshold, int is_logits, float gamma, float inv_gamma, float alpha, float p0r, float p0g,
                                   float p0b, float p1r, float p1g, float p1b, float p2r, float p2g, float p2b,
                                   unsigned char* rgb, unsigned char* classes, hipStream_t stream) {
  HPRI_REQUIRE(image && pred && mask && rgb, "segmap_overlay: null pointer");
  HPRI_REQUIRE(N > 0 && h > 0 && w > 0 && C > 0, "segmap_overlay: bad sizes");
  HPRI_REQUIRE(sn >= 0 && sc >= 0 && sy >= 0 && sx >= 0, "segmap_overlay: negative stride");
  HPRI_REQUIRE(band_r >= 0 && band_r < C && band_g >= 0 && band_g < C && band_b >= 0 && band_b < C,
               "segmap_overlay: band index outside [0, C)");
  HPRI_REQUIRE(gamma > 0.f && inv_gamma > 0.f, "segmap_overlay: gamma must be positive");
  HPRI_REQUIRE(alpha >= 0.f && alpha <= 1.f, "segmap_overlay: alpha must lie in [0, 1]");
  SegmapArgs a;
  const float pal[9] = {p0r, p0g, p0b, p1r, p1g, p1b, p2r, p2g, p2b};
  for (int i = 0; i < 9; ++i) {
    HPRI_REQUIRE(pal[i] >= 0.f && pal[i] <= 1.f, "segmap_overlay: palette entries must lie in [0, 1]");
    a.palette[i] = pal[i];
  }
  a.image = image; a.sn = sn; a.sc = sc; a.sy = sy; a.sx = sx;
  a.band[0] = band_r; a.band[1] = band_g; a.band[2] = band_b;
  a.pred = pred; a.mask = mask; a.N = N; a.h = h; a.w = w;
  a.threshold = threshold; a.is_logits = is_logits; a.gamma_is_one = gamma == 1.f;
  a.inv_gamma = inv_gamma; a.alpha = alpha; a.rgb = rgb; a.classes = classes;
  a.vec = (((uintptr_t)pred | (uintptr_t)mask) & 15) == 0 && (((uintptr_t)rgb | (uintptr_t)classes) & 3) == 0;
  const long long items = (long long)N * h * ((w + 3) / 4);
  // (items >= 1 after the size checks above: the floor of hpri_grid_per_cu never acts)
  hipLaunchKernelGGL(segmap_overlay_kernel, dim3(hpri_grid_per_cu(items, SEGMAP_THREADS, 8)), dim3(SEGMAP_THREADS), 0, stream, a);
  HPRI_CHECK_LAUNCH();
  return HPRI_OK;
}

// ------------------------------------------------------------------------------------------------------------------------
// The multi-class picture: the same base picture under the colours of a uint8 class map (N, h, w), predicted (hpri_seg_confusion's
// `classes`) or true.  K colours; class 0 -- the background -- shows the bare picture, and so does a value >= K:
//   out_k = class == 0 ? base_k : alpha * palette[class][k] + (1 - alpha) * base_k;   rgb_k = (uint8)(out_k * 255 + 0.5f)
// Same quads, same accesses and the same grid as the overlay above; the palette (at most 64 x 3 floats, by value in the kernel's
// arguments) is staged in LDS once per workgroup because the class that indexes it differs from lane to lane.
// ------------------------------------------------------------------------------------------------------------------------
#define SEGMAP_MAX_CLASSES 64

struct ClassmapArgs {
  const float* image;
  long long sn, sc, sy, sx;
  int band[3];
  const unsigned char* classes;         // (N, h, w) contiguous
  int N, h, w, K;
  int gamma_is_one;
  float inv_gamma, alpha;
  unsigned char* rgb;                   // (N, h, w, 3)
  int vec;                              // classes / rgb allow the 4-byte accesses of an aligned quad
  float palette[3 * SEGMAP_MAX_CLASSES];
};

__device__ __forceinline__ unsigned classmap_level(const ClassmapArgs& a, const float* pal, int cls, int k, float base) {
  return cls == 0 ? segmap_round(base) : segmap_blend(a.alpha, pal[3 * cls + k], base);
}

__global__ __launch_bounds__(SEGMAP_THREADS) void segmap_classes_kernel(const ClassmapArgs a) {
  __shared__ float pal[3 * SEGMAP_MAX_CLASSES];
  for (int i = threadIdx.x; i < 3 * a.K; i += SEGMAP_THREADS) pal[i] = a.palette[i];
  __syncthreads();
  const int wq = (a.w + 3) >> 2;
  const long long items = (long long)a.N * a.h * wq;
  for (long long it = (long long)blockIdx.x * SEGMAP_THREADS + threadIdx.x; it < items; it += (long long)gridDim.x * SEGMAP_THREADS) {
    const long long r = it / wq;
    const int x0 = (int)(it - r * wq) * 4;
    const long long n = r / a.h;
    const int y = (int)(r - n * a.h);
    const long long pix = r * a.w + x0;
    const float* img = a.image + n * a.sn + y * a.sy + x0 * a.sx;
    if (x0 + 4 <= a.w) {
      int c[4];
      float v[3][4];
      const bool quad = a.vec && (pix & 3) == 0;
      if (quad) {
        const unsigned cw = *reinterpret_cast<const unsigned*>(a.classes + pix);
#pragma unroll
        for (int j = 0; j < 4; ++j) c[j] = (cw >> (8 * j)) & 255u;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) c[j] = a.classes[pix + j];
      }
      segmap_bands<4>(img, a.band, a.sc, a.sx, v);
      unsigned char o[12];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int cls = c[j] < a.K ? c[j] : 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) o[3 * j + k] = (unsigned char)classmap_level(a, pal, cls, k, segmap_base(v[k][j], a.gamma_is_one, a.inv_gamma));
      }
      unsigned char* d = a.rgb + 3 * pix;
      if (quad) {
        unsigned* dw = reinterpret_cast<unsigned*>(d);
#pragma unroll
        for (int q = 0; q < 3; ++q)
          dw[q] = (unsigned)o[4 * q] | ((unsigned)o[4 * q + 1] << 8) | ((unsigned)o[4 * q + 2] << 16) | ((unsigned)o[4 * q + 3] << 24);
      } else {
#pragma unroll
        for (int q = 0; q < 12; ++q) d[q] = o[q];
      }
    } else {
      for (int j = 0; x0 + j < a.w; ++j) {
        float v[3][1];
        segmap_bands<1>(img + j * a.sx, a.band, a.sc, a.sx, v);
        const int cj = a.classes[pix + j], cls = cj < a.K ? cj : 0;
#pragma unroll
        for (int k = 0; k < 3; ++k)
          a.rgb[3 * (pix + j) + k] = (unsigned char)classmap_level(a, pal, cls, k, segmap_base(v[k][0], a.gamma_is_one, a.inv_gamma));
      }
    }
  }
}

// image, strides, C, bands, gamma / inv_gamma, alpha: as hpri_segmap_overlay.  classes: contiguous (N, h, w) uint8.
// palette: K x 3 HOST floats in [0, 1] (row 0 is never shown), 2 <= K <= 64.  rgb: (N, h, w, 3) uint8.
extern "C" int hpri_segmap_classes(const float* image, long long sn, long long sc, long long sy, long long sx, int C, int band_r,
                                   int band_g, int band_b, const unsigned char* classes, int N, int h, int w, float gamma,
                                   float inv_gamma, float alpha, const float* palette, int K, unsigned char* rgb,
                                   hipStream_t stream) {
  HPRI_REQUIRE(image && classes && palette && rgb, "segmap_classes: null pointer");
  HPRI_REQUIRE(K >= 2 && K <= SEGMAP_MAX_CLASSES, "segmap_classes: the number of classes must lie in [2, 64]");
  HPRI_REQUIRE(N > 0 && h > 0 && w > 0 && C > 0, "segmap_classes: bad sizes");
  HPRI_REQUIRE(sn >= 0 && sc >= 0 && sy >= 0 && sx >= 0, "segmap_classes: negative stride");
  HPRI_REQUIRE(band_r >= 0 && band_r < C && band_g >= 0 && band_g < C && band_b >= 0 && band_b < C,
               "segmap_classes: band index outside [0, C)");
  HPRI_REQUIRE(gamma > 0.f && inv_gamma > 0.f, "segmap_classes: gamma must be positive");
  HPRI_REQUIRE(alpha >= 0.f && alpha <= 1.f, "segmap_classes: alpha must lie in [0, 1]");
  ClassmapArgs a;
  for (int i = 0; i < 3 * SEGMAP_MAX_CLASSES; ++i) {
    if (i < 3 * K) HPRI_REQUIRE(palette[i] >= 0.f && palette[i] <= 1.f, "segmap_classes: palette entries must lie in [0, 1]");
    a.palette[i] = i < 3 * K ? palette[i] : 0.f;
  }
  a.image = image; a.sn = sn; a.sc = sc; a.sy = sy; a.sx = sx;
  a.band[0] = band_r; a.band[1] = band_g; a.band[2] = band_b;
  a.classes = classes; a.N = N; a.h = h; a.w = w; a.K = K;
  a.gamma_is_one = gamma == 1.f; a.inv_gamma = inv_gamma; a.alpha = alpha; a.rgb = rgb;
  a.vec = (((uintptr_t)classes | (uintptr_t)rgb) & 3) == 0;
  const long long items = (long long)N * h * ((w + 3) / 4);
  hipLaunchKernelGGL(segmap_classes_kernel, dim3(hpri_grid_per_cu(items, SEGMAP_THREADS, 8)), dim3(SEGMAP_THREADS), 0, stream, a);
  HPRI_CHECK_LAUNCH();
  return HPRI_OK;
}
