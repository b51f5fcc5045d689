// Cube cache, augmenting gather (hyperpri_amd/cache.py: CubeAugment, plan_epoch_augmented): the batch is resampled from the
// cached slots through one affine map per sample -- rotation, zoom, sub-pixel shift and the flips -- with a photometric gain /
// offset and a run of dropped bands, in the same kind of memory-bound pass as cache.hip's gather: four pixel records read, one
// written.  The mask follows through the same map with nearest-neighbour sampling (class ids survive).
//
// Warp entry: 64 bytes = 16 32-bit words per sample, 16-byte aligned, in DEVICE memory:
//     word  0      int32  slot                      (clamped into [0, slots))
//     word  1      int32  drop_lo                   (clamped into [0, cs])
//     word  2      int32  drop_n                    (clamped into [0, cs]; channels [drop_lo, drop_lo + drop_n) are written as 0)
//     word  3      reserved, 0
//     words 4..9   fp32   a00, a01, cx, a10, a11, cy
//     words 10,11  fp32   gain, offset
//     words 12..15 reserved, 0
//
// Output pixel (y, x) of an h x w window:   u = x - (w-1)/2,  v = y - (h-1)/2            (exact in fp32: h, w <= 4096)
//     sx = fma(a00, u, fma(a01, v, cx))     sy = fma(a10, u, fma(a11, v, cy))            (source column / row, centres at integers)
//   image  dst[n, y, x, c] = gain * bilinear(slot, sy, sx, c) + offset for c < C: neighbours (floor sy, floor sx), (+0, +1), (+1, +0),
//          (+1, +1), weights (1-fy)(1-fx), (1-fy) fx, fy (1-fx), fy fx, all fp32 (fp16 slots convert on load).  A neighbour outside
//          the frame counts as 0 and is NOT loaded, and neither is one whose weight is exactly 0: at integer sx, sy one weight is 1,
//          one record is read, and with gain 1 / offset 0 the stored bits come out.  Dropped channels are exactly 0 (after gain and
//          offset); pad channels [C, cs) are exactly 0 whatever the offset (the networks consume the buffer in place).
//   mask   dst[n, 0, y, x] = (float)mask[slot, floor(sy + 0.5), floor(sx + 0.5)], 0 outside the frame; gain / offset / drop do not
//          touch it.
//
// The launchers cannot see the entries, so the kernels clamp: the slot into the cache, sx / sy IN FLOATING POINT to [-1, Ws] /
// [-1, Hs] before any conversion to integer (fmaxf first: a NaN leaves it as -1), the drop run into [0, cs].  A bad entry gives a
// wrong picture (anything further out than one pixel is zero fill anyway), never an access outside the allocation.
#include "cache_warp.h"

// Work items as in cube_gather_kernel: a workgroup takes WARP_ITEM consecutive channel quads of one window row (n, y), so the
// entry and v are uniform per item, consecutive lanes walk the quads of consecutive output pixels, and the source records of
// neighbouring outputs are neighbours too (one source step of (a00, a10) pixels per output pixel).  Every lane issues the
// 4 * WARP_UNROLL neighbour loads of its quads before the first multiply.
template <typename T>
__global__ __launch_bounds__(WARP_THREADS) __attribute__((amdgpu_waves_per_eu(8, 8))) void cube_warp_kernel(const T* __restrict__ cache, int slots, int Hs, int Ws, int q, int C,
                                                                   const int* __restrict__ entries, int N, int h, int w,
                                                                   float* __restrict__ dst) {
  const int rowq = w * q;                                             // quads per window row (< 2^30: checked by the launcher)
  const int pieces = (rowq + WARP_ITEM - 1) / WARP_ITEM;
  const long long items = (long long)N * h * pieces;
  const float uc = 0.5f * (float)(w - 1), vc = 0.5f * (float)(h - 1);
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    const int r = (int)(it / pieces), piece = (int)(it - (long long)r * pieces);
    const int n = r / h, y = r - n * h;
    const WarpEntry g = warp_entry(entries, n, slots, 4 * q);
    const T* s = cache + (long long)g.slot * Hs * Ws * (4LL * q);
    float* d = dst + (long long)r * rowq * 4LL;
    const float v = (float)y - vc;
    const int j0 = piece * WARP_ITEM + threadIdx.x;
    typedef typename WarpRaw<T>::type raw_t;
    raw_t t[WARP_UNROLL][4];
    float wt[WARP_UNROLL][4];
    int ch[WARP_UNROLL];
    // (only the loads and the store depend on j < rowq: the arithmetic below runs in every lane, so that no path round it leaves
    // a load pending at the head of the next unroll step or item -- the compiler would wait there for everything in flight)
#pragma unroll
    for (int k = 0; k < WARP_UNROLL; ++k) {
      const int j = j0 + k * WARP_THREADS;
      const bool live = j < rowq;
      const int x = j / q, c0 = 4 * (j - x * q);
      const float u = (float)x - uc;
      const float sx = warp_coord(g.a00, g.a01, g.cx, u, v, Ws), sy = warp_coord(g.a10, g.a11, g.cy, u, v, Hs);
      const float fx0 = floorf(sx), fy0 = floorf(sy);
      const float fx = sx - fx0, fy = sy - fy0;
      const int x0 = (int)fx0, y0 = (int)fy0;                        // in [-1, Ws] x [-1, Hs]
      ch[k] = c0;
      wt[k][0] = (1.f - fy) * (1.f - fx); wt[k][1] = (1.f - fy) * fx; wt[k][2] = fy * (1.f - fx); wt[k][3] = fy * fx;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int xi = x0 + (b & 1), yi = y0 + (b >> 1);
        t[k][b] = raw_t{0, 0, 0, 0};
        // (an outside neighbour is zero fill; a zero weight is skipped, not multiplied)
        if (live && wt[k][b] != 0.f && xi >= 0 && xi < Ws && yi >= 0 && yi < Hs) t[k][b] = *reinterpret_cast<const raw_t*>(s + ((long long)yi * Ws + xi) * (4LL * q) + c0);
      }
    }
#pragma unroll
    for (int k = 0; k < WARP_UNROLL; ++k) {
      const int j = j0 + k * WARP_THREADS;
      const f32x4 t0 = warp_widen(t[k][0]), t1 = warp_widen(t[k][1]), t2 = warp_widen(t[k][2]), t3 = warp_widen(t[k][3]);
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float acc = wt[k][0] * t0[e];
        acc = fmaf(wt[k][1], t1[e], acc);
        acc = fmaf(wt[k][2], t2[e], acc);
        acc = fmaf(wt[k][3], t3[e], acc);
        const int c = ch[k] + e;
        o[e] = (c >= C || (c >= g.drop_lo && c < g.drop_hi)) ? 0.f : fmaf(g.gain, acc, g.offset);
      }
      if (j < rowq) *reinterpret_cast<f32x4*>(d + 4LL * j) = o;
    }
  }
}

// cache_dtype: 0 = float32, 1 = float16.  cache: (slots, Hs, Ws, cs); entries: N warp entries of 64 bytes on the device;
// dst: (N, h, w, cs) fp32.  The window may be larger than the frame (everything outside is zero fill).
extern "C" int hpri_cube_warp(const void* cache, int cache_dtype, int slots, int Hs, int Ws, int cs, int C, const int* entries,
                              int N, int h, int w, float* dst, hipStream_t stream) {
  HPRI_REQUIRE(cache && entries && dst, "cube_warp: null pointer");
  HPRI_REQUIRE(cache_dtype == 0 || cache_dtype == 1, "cube_warp: cache_dtype must be 0 (f32) or 1 (f16)");
  HPRI_REQUIRE(slots > 0 && Hs > 0 && Ws > 0 && N > 0, "cube_warp: bad sizes");
  HPRI_REQUIRE(cs > 0 && cs % 8 == 0, "cube_warp: the channel stride must be a multiple of 8");
  HPRI_REQUIRE(C > 0 && C <= cs, "cube_warp: the band count must lie in (0, cs]");
  HPRI_REQUIRE(h > 0 && w > 0 && h <= 4096 && w <= 4096, "cube_warp: the window must be 1 .. 4096 pixels a side");
  HPRI_REQUIRE((long long)w * (cs / 4) < 0x40000000LL && (long long)N * h < 0x7FFFFFFFLL, "cube_warp: window too large");
  HPRI_REQUIRE(((uintptr_t)cache & 15) == 0 && ((uintptr_t)dst & 15) == 0 && ((uintptr_t)entries & 15) == 0,
               "cube_warp: buffers must be 16-byte aligned");
  const int q = cs / 4;
  const long long pieces = ((long long)w * q + WARP_ITEM - 1) / WARP_ITEM;
  long long blocks = (long long)N * h * pieces;
  const long long cap = 8LL * hpri_cu_count();                      // eight workgroups per CU, grid-stride over the rest
  if (blocks > cap) blocks = cap;
  if (cache_dtype == 0)
    hipLaunchKernelGGL(cube_warp_kernel<float>, dim3((unsigned)blocks), dim3(WARP_THREADS), 0, stream, (const float*)cache, slots,
                       Hs, Ws, q, C, entries, N, h, w, dst);
  else
    hipLaunchKernelGGL(cube_warp_kernel<_Float16>, dim3((unsigned)blocks), dim3(WARP_THREADS), 0, stream, (const _Float16*)cache,
                       slots, Hs, Ws, q, C, entries, N, h, w, dst);
  HPRI_CHECK_LAUNCH();
  return HPRI_OK;
}

// ---- mask warp: one output pixel per thread, the image's coordinates, nearest neighbour ------------------------------
__global__ void mask_warp_kernel(const unsigned char* __restrict__ masks, int slots, int Hs, int Ws, const int* __restrict__ entries,
                                 int N, int h, int w, float* __restrict__ dst) {
  const long long total = (long long)N * h * w;
  const float uc = 0.5f * (float)(w - 1), vc = 0.5f * (float)(h - 1);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int r = (int)(i / w), x = (int)(i - (long long)r * w);
    const int n = r / h, y = r - n * h;
    const WarpEntry g = warp_entry(entries, n, slots, 8);
    const float u = (float)x - uc, v = (float)y - vc;
    const float sx = warp_coord(g.a00, g.a01, g.cx, u, v, Ws), sy = warp_coord(g.a10, g.a11, g.cy, u, v, Hs);
    const int xs = (int)floorf(sx + 0.5f), ys = (int)floorf(sy + 0.5f);       // in [-1, Ws] x [-1, Hs]
    float o = 0.f;
    if (xs >= 0 && xs < Ws && ys >= 0 && ys < Hs) o = (float)masks[((long long)g.slot * Hs + ys) * Ws + xs];
    dst[i] = o;
  }
}

// masks: uint8 (slots, Hs, Ws); dst: fp32 (N, 1, h, w); the entries of hpri_cube_warp.
extern "C" int hpri_mask_warp(const unsigned char* masks, int slots, int Hs, int Ws, const int* entries, int N, int h, int w,
                              float* dst, hipStream_t stream) {
  HPRI_REQUIRE(masks && entries && dst, "mask_warp: null pointer");
  HPRI_REQUIRE(slots > 0 && Hs > 0 && Ws > 0 && N > 0, "mask_warp: bad sizes");
  HPRI_REQUIRE(h > 0 && w > 0 && h <= 4096 && w <= 4096, "mask_warp: the window must be 1 .. 4096 pixels a side");
  HPRI_REQUIRE((long long)N * h < 0x7FFFFFFFLL, "mask_warp: window too large");
  HPRI_REQUIRE(((uintptr_t)entries & 15) == 0, "mask_warp: the entries must be 16-byte aligned");
  long long blocks = ((long long)N * h * w + 255) / 256;
  const long long cap = 8LL * hpri_cu_count();
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(mask_warp_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, masks, slots, Hs, Ws, entries, N, h, w, dst);
  HPRI_CHECK_LAUNCH();
  return HPRI_OK;
}
