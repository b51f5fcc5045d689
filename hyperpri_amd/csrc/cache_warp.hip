// Cube cache, resampling gather (hyperpri_amd/cache.py: CubeAugment, plan_epoch_augmented; CubeDeform, plan_epoch_deformed): the
// batch is resampled from the cached slots through one affine map per sample -- rotation, zoom, sub-pixel shift and the flips --
// with a photometric gain / offset and a run of dropped bands, in the same kind of memory-bound pass as cache.hip's gather: four
// pixel records read, one written.  The mask follows through the same map with nearest-neighbour sampling (class ids survive).
// The deforming kernels are the same pass with one more input to the coordinate -- an elastic displacement field
// (cache_deform.hip builds it) --, one more term in the value -- Gaussian noise from a counter-based generator -- and one choice
// of which sample a pixel belongs to -- a CutMix rectangle.  The entry readers, the clamped coordinate and the quad forms below
// serve both kernel pairs, and each pair has one launcher.  The kernel BODIES are still two: folding cube_warp_kernel and
// cube_deform_kernel into one template made the fp16 warp instantiation 1 - 2 % slower, and the folded mask kernels 6 %
// (profiles/cube_resample_refactor.json), so a change to the sampling rule is still made in both.
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
// Deform entry: 64 bytes = 16 32-bit words per sample, 16-byte aligned, in DEVICE memory, parallel to the warp entries:
//     word  0      int32  mix_from     batch index in [0, N) of the sample that owns the rectangle's pixels; anything else, or the
//                                      sample's own index: no CutMix
//     words 1..4   int32  ry0, ry1, rx0, rx1   the rectangle [ry0, ry1) x [rx0, rx1) in window coordinates, clamped into the window
//                                      by the kernels; empty: none
//     word  5      int32  nodes_off    offset in floats of this sample's lattice in the node table; negative: no elastic field
//     words 6, 7   int32  gy, gx       lattice rows and columns
//     word  8      fp32   inv_pitch    1 / node spacing in output pixels (both axes)
//     word  9      fp32   noise_sigma  noise is applied only when sigma > 0 (a NaN or a negative value: none)
//     words 10,11  uint32 k0, k1       the Philox key of this sample's noise
//     words 12..15 reserved, 0
//
// Output pixel (y, x) of sample s of an h x w window (the warp kernels: o = s, no field, no noise):
//     owner   o = mix_from[s] when CutMix is on for s and (y, x) lies in its rectangle, else s (o's own CutMix words are ignored)
//     u = (x + field[o, y, x, 0]) - (w-1)/2,  v = (y + field[o, y, x, 1]) - (h-1)/2     (a null field counts as zeros; without
//                                                                                       one exact in fp32: h, w <= 4096)
//     with o's WARP entry:
//     sx = fma(a00, u, fma(a01, v, cx))     sy = fma(a10, u, fma(a11, v, cy))            (source column / row, centres at integers)
//   image  base = gain * bilinear(slot, sy, sx, c) + offset for c < C: neighbours (floor sy, floor sx), (+0, +1), (+1, +0),
//          (+1, +1), weights (1-fy)(1-fx), (1-fy) fx, fy (1-fx), fy fx, all fp32 (fp16 slots convert on load).  A neighbour outside
//          the frame counts as 0 and is NOT loaded, and neither is one whose weight is exactly 0: at integer sx, sy one weight is 1,
//          one record is read, and with gain 1 / offset 0 the stored bits come out.
//          dst[s, y, x, c] = base, or fmaf(sigma[s], z, base) when sigma[s] > 0: the noise and its key are ALWAYS those of s.
//          Dropped channels are exactly 0 (after gain, offset and noise); pad channels [C, cs) are exactly 0 whatever the offset
//          (the networks consume the buffer in place).
//   mask   dst[s, 0, y, x] = (float)mask[slot, floor(sy + 0.5), floor(sx + 0.5)], 0 outside the frame; gain / offset / drop / noise
//          do not touch it.
// Noise: z from Philox4x32-10 (deform_math.h) under the key (k0, k1) at the counter (lo32 e, hi32 e, 0, 0),
// e = (y * w + x) * (cs / 4) + c0 / 4: one call per channel quad, words r0..r3 for channels c0..c0+3, (r0, r1) and (r2, r3) through
// Box-Muller.  No fast intrinsics, and this file must not be built with -ffast-math: the stream is documented bit for bit.
//
// The launchers cannot see the entries, so the kernels clamp: the slot into the cache, sx / sy IN FLOATING POINT to [-1, Ws] /
// [-1, Hs] before any conversion to integer (fmaxf first: a NaN leaves it as -1), the drop run into [0, cs], the rectangle into
// the window.  A bad entry gives a wrong picture (anything further out than one pixel is zero fill anyway), never an access
// outside the allocation.
#include "cache_launch.h"
#include "deform_math.h"

#define WARP_THREADS 256
#define WARP_UNROLL 2
#define WARP_ITEM (WARP_THREADS * WARP_UNROLL)

struct WarpEntry { int slot, drop_lo, drop_hi; float a00, a01, cx, a10, a11, cy, gain, offset; };

__device__ __forceinline__ WarpEntry warp_entry(const int* __restrict__ entries, int n, int slots, int cs) {
  const int4* e = reinterpret_cast<const int4*>(entries + 16 * (size_t)n);
  const int4 a = e[0], b = e[1], c = e[2];
  WarpEntry g;
  g.slot = min(max(a.x, 0), slots - 1);
  g.drop_lo = min(max(a.y, 0), cs);
  g.drop_hi = min(g.drop_lo + min(max(a.z, 0), cs), cs);
  g.a00 = __int_as_float(b.x); g.a01 = __int_as_float(b.y); g.cx = __int_as_float(b.z);
  g.a10 = __int_as_float(b.w); g.a11 = __int_as_float(c.x); g.cy = __int_as_float(c.y);
  g.gain = __int_as_float(c.z); g.offset = __int_as_float(c.w);
  return g;
}

struct DeformEntry { int mix_from, ry0, ry1, rx0, rx1; float sigma; unsigned k0, k1; };

// s's deform words as the cube / mask kernels use them: mix_from = -1 when there is no CutMix, the rectangle inside the window,
// sigma = 0 when there is no noise
__device__ __forceinline__ DeformEntry deform_entry(const int* __restrict__ deform, int s, int N, int h, int w) {
  const int4* e = reinterpret_cast<const int4*>(deform + 16 * (size_t)s);
  const int4 a = e[0], b = e[1], c = e[2];
  DeformEntry d;
  d.ry0 = max(a.y, 0); d.ry1 = min(a.z, h); d.rx0 = max(a.w, 0); d.rx1 = min(b.x, w);
  d.mix_from = (a.x >= 0 && a.x < N && a.x != s && d.ry0 < d.ry1 && d.rx0 < d.rx1) ? a.x : -1;
  const float sg = __int_as_float(c.y);
  d.sigma = sg > 0.f ? sg : 0.f;                                       // (a NaN compares false)
  d.k0 = (unsigned)c.z; d.k1 = (unsigned)c.w;
  return d;
}

// the source coordinate of one axis, clamped into [-1, extent] (a NaN becomes -1: fmaxf returns its other operand)
__device__ __forceinline__ float warp_coord(float au, float av, float c0, float u, float v, int extent) {
  return fminf(fmaxf(fmaf(au, u, fmaf(av, v, c0)), -1.f), (float)extent);
}

// a quad as it is loaded (fp16 slots: two registers) and as it enters the arithmetic: the conversion waits for the load, so it
// belongs to the arithmetic, behind ALL the loads of the item
template <typename T> struct WarpRaw;
template <> struct WarpRaw<float> { typedef f32x4 type; };
template <> struct WarpRaw<_Float16> { typedef f16x4 type; };
__device__ __forceinline__ f32x4 warp_widen(f32x4 v) { return v; }
__device__ __forceinline__ f32x4 warp_widen(f16x4 v) {
  f32x4 r;
  r[0] = (float)v[0]; r[1] = (float)v[1]; r[2] = (float)v[2]; r[3] = (float)v[3];
  return r;
}

// ---- the cube: the warp kernel -------------------------------------------------------------------------------------------
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

// ---- the cube: cube_warp_kernel's work items ---------------------------------------------------------------------------
// A workgroup takes WARP_ITEM consecutive channel quads of one window row (s, y).  The row's deform entry is uniform, and so are
// the two warp entries a lane can belong to -- s's own and its CutMix partner's --: the choice between them is per lane (a row
// that crosses a rectangle edge), made by selects, not by branches.  Order inside an item: the field loads of both unroll steps,
// the coordinates and all 4 * WARP_UNROLL neighbour loads, then -- while those are in flight -- Philox and Box-Muller for a noisy
// sample (a uniform branch), then the conversion, the bilinear sum and the store.  Only loads and the store depend on the row tail.
// Registers: the per-lane owner choice and the four normals per unroll step do not fit cube_warp_kernel's 64 (eight waves per
// SIMD); this kernel is built for six waves per SIMD (80 registers): the compiler's report shows 77 for fp32 slots, 71 for fp16, no spill.
template <typename T>
__global__ __launch_bounds__(WARP_THREADS) __attribute__((amdgpu_waves_per_eu(6, 6))) void cube_deform_kernel(
    const T* __restrict__ cache, int slots, int Hs, int Ws, int q, int C, const int* __restrict__ entries, const int* __restrict__ deform,
    const float* __restrict__ field, int N, int h, int w, float* __restrict__ dst) {
  const int rowq = w * q;                                             // quads per window row (< 2^30: checked by the launcher)
  const int pieces = (rowq + WARP_ITEM - 1) / WARP_ITEM;
  const long long items = (long long)N * h * pieces;
  const long long slot_elems = (long long)Hs * Ws * (4LL * q);
  const float uc = 0.5f * (float)(w - 1), vc = 0.5f * (float)(h - 1);
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    const int r = (int)(it / pieces), piece = (int)(it - (long long)r * pieces);
    const int n = r / h, y = r - n * h;
    const DeformEntry de = deform_entry(deform, n, N, h, w);
    const bool rowin = de.mix_from >= 0 && y >= de.ry0 && y < de.ry1;
    const int p = rowin ? de.mix_from : n;                            // the only other owner this row can have
    const WarpEntry gs = warp_entry(entries, n, slots, 4 * q), gp = warp_entry(entries, p, slots, 4 * q);
    const long long row_s = ((long long)n * h + y) * w, row_p = ((long long)p * h + y) * w;   // pixels before this row, per owner
    float* d = dst + (long long)r * rowq * 4LL;
    const int j0 = piece * WARP_ITEM + threadIdx.x;
    typedef typename WarpRaw<T>::type raw_t;
    raw_t t[WARP_UNROLL][4];
    float wt[WARP_UNROLL][4];
    float2 disp[WARP_UNROLL];
    float z[WARP_UNROLL][4];
    // the displacement of every lane's pixel, from its owner's field
#pragma unroll
    for (int k = 0; k < WARP_UNROLL; ++k) {
      const int j = j0 + k * WARP_THREADS;
      const int x = j / q;
      const bool mine = rowin && x >= de.rx0 && x < de.rx1;
      disp[k] = make_float2(0.f, 0.f);
      if (field != nullptr && j < rowq) disp[k] = reinterpret_cast<const float2*>(field)[(mine ? row_p : row_s) + x];
    }
#pragma unroll
    for (int k = 0; k < WARP_UNROLL; ++k) {
      const int j = j0 + k * WARP_THREADS;
      const bool live = j < rowq;
      const int x = j / q, c0 = 4 * (j - x * q);
      const bool mine = rowin && x >= de.rx0 && x < de.rx1;
      const float a00 = mine ? gp.a00 : gs.a00, a01 = mine ? gp.a01 : gs.a01, cx = mine ? gp.cx : gs.cx;
      const float a10 = mine ? gp.a10 : gs.a10, a11 = mine ? gp.a11 : gs.a11, cy = mine ? gp.cy : gs.cy;
      const T* s = cache + (mine ? gp.slot : gs.slot) * slot_elems;
      const float u = ((float)x + disp[k].x) - uc, v = ((float)y + disp[k].y) - vc;
      const float sx = warp_coord(a00, a01, cx, u, v, Ws), sy = warp_coord(a10, a11, cy, u, v, Hs);
      const float fx0 = floorf(sx), fy0 = floorf(sy);
      const float fx = sx - fx0, fy = sy - fy0;
      const int x0 = (int)fx0, y0 = (int)fy0;                        // in [-1, Ws] x [-1, Hs]
      wt[k][0] = (1.f - fy) * (1.f - fx); wt[k][1] = (1.f - fy) * fx; wt[k][2] = fy * (1.f - fx); wt[k][3] = fy * fx;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int xi = x0 + (b & 1), yi = y0 + (b >> 1);
        t[k][b] = raw_t{0, 0, 0, 0};
        if (live && wt[k][b] != 0.f && xi >= 0 && xi < Ws && yi >= 0 && yi < Hs) t[k][b] = *reinterpret_cast<const raw_t*>(s + ((long long)yi * Ws + xi) * (4LL * q) + c0);
      }
    }
    // the noise of s, while the loads are in flight: e = (y * w + x) * q + c0 / 4 = y * rowq + j
    const bool noisy = de.sigma > 0.f;
#pragma unroll
    for (int k = 0; k < WARP_UNROLL; ++k) {
      z[k][0] = z[k][1] = z[k][2] = z[k][3] = 0.f;
      if (noisy) {
        uint32_t bits[4];
        hpri_deform_bits(de.k0, de.k1, (uint64_t)((long long)y * rowq + (j0 + k * WARP_THREADS)), bits);
        hpri_deform_normals(bits, z[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < WARP_UNROLL; ++k) {
      const int j = j0 + k * WARP_THREADS;
      const int x = j / q, c0 = 4 * (j - x * q);
      const bool mine = rowin && x >= de.rx0 && x < de.rx1;
      const float gain = mine ? gp.gain : gs.gain, offset = mine ? gp.offset : gs.offset;
      const int drop_lo = mine ? gp.drop_lo : gs.drop_lo, drop_hi = mine ? gp.drop_hi : gs.drop_hi;
      const f32x4 t0 = warp_widen(t[k][0]), t1 = warp_widen(t[k][1]), t2 = warp_widen(t[k][2]), t3 = warp_widen(t[k][3]);
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float acc = wt[k][0] * t0[e];
        acc = fmaf(wt[k][1], t1[e], acc);
        acc = fmaf(wt[k][2], t2[e], acc);
        acc = fmaf(wt[k][3], t3[e], acc);
        const int c = c0 + e;
        const float base = fmaf(gain, acc, offset);
        const float val = noisy ? fmaf(de.sigma, z[k][e], base) : base;
        o[e] = (c >= C || (c >= drop_lo && c < drop_hi)) ? 0.f : val;
      }
      if (j < rowq) *reinterpret_cast<f32x4*>(d + 4LL * j) = o;
    }
  }
}

// hpri_cube_warp (deformed == false: deform and field are null, the kernel without the deformation) and hpri_cube_deform.  The
// grid is one workgroup per CU for every wave per SIMD the kernel is built for, grid-stride over the rest.
static int cube_resample_launch(const CachePass& p, bool deformed, const void* cache, int cache_dtype, int cs, int C, const int* entries,
                                const int* deform, const float* field, float* dst, hipStream_t stream) {
  CACHE_REQUIRE(p.who, cache && entries && dst && (deform || !deformed), "null pointer");
  const CacheSlots c = {cache_dtype, cs, C};
  if (int e = cache_check(p, &c)) return e;
  CACHE_REQUIRE(p.who, hpri_aligned16(cache, dst, entries, deform, field), "buffers must be 16-byte aligned");
  const int q = cs / 4;
  const dim3 grid = cache_grid(cache_row_items(p, q, WARP_ITEM), deformed ? 6 : 8), block(WARP_THREADS);
  const float* c32 = (const float*)cache;
  const _Float16* c16 = (const _Float16*)cache;
  if (!deformed && cache_dtype == 0)
    hipLaunchKernelGGL(cube_warp_kernel<float>, grid, block, 0, stream, c32, p.slots, p.Hs, p.Ws, q, C, entries, p.N, p.h, p.w, dst);
  else if (!deformed)
    hipLaunchKernelGGL(cube_warp_kernel<_Float16>, grid, block, 0, stream, c16, p.slots, p.Hs, p.Ws, q, C, entries, p.N, p.h, p.w, dst);
  else if (cache_dtype == 0)
    hipLaunchKernelGGL(cube_deform_kernel<float>, grid, block, 0, stream, c32, p.slots, p.Hs, p.Ws, q, C, entries, deform, field, p.N, p.h,
                       p.w, dst);
  else
    hipLaunchKernelGGL(cube_deform_kernel<_Float16>, grid, block, 0, stream, c16, p.slots, p.Hs, p.Ws, q, C, entries, deform, field, p.N,
                       p.h, p.w, dst);
  HPRI_CHECK_LAUNCH();
  return HPRI_OK;
}

// cache_dtype: 0 = float32, 1 = float16.  cache: (slots, Hs, Ws, cs); entries: N warp entries of 64 bytes on the device;
// dst: (N, h, w, cs) fp32.  The window may be larger than the frame (everything outside is zero fill).
extern "C" int hpri_cube_warp(const void* cache, int cache_dtype, int slots, int Hs, int Ws, int cs, int C, const int* entries,
                              int N, int h, int w, float* dst, hipStream_t stream) {
  return cube_resample_launch({"cube_warp", slots, Hs, Ws, N, h, w, false}, false, cache, cache_dtype, cs, C, entries, nullptr, nullptr,
                              dst, stream);
}

// hpri_cube_warp's arguments plus deform (N deform entries on the device) and field ((N, h, w, 2) fp32 from hpri_elastic_field,
// or null: no displacement).
extern "C" int hpri_cube_deform(const void* cache, int cache_dtype, int slots, int Hs, int Ws, int cs, int C, const int* entries,
                                const int* deform, const float* field, int N, int h, int w, float* dst, hipStream_t stream) {
  return cube_resample_launch({"cube_deform", slots, Hs, Ws, N, h, w, false}, true, cache, cache_dtype, cs, C, entries, deform, field,
                              dst, stream);
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

// (the deforming mask: the image's owner and coordinates)
__global__ __launch_bounds__(256) void mask_deform_kernel(const unsigned char* __restrict__ masks, int slots, int Hs, int Ws,
                                                           const int* __restrict__ entries, const int* __restrict__ deform,
                                                           const float* __restrict__ field, int N, int h, int w, float* __restrict__ dst) {
  const long long total = (long long)N * h * w;
  const float uc = 0.5f * (float)(w - 1), vc = 0.5f * (float)(h - 1);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int r = (int)(i / w), x = (int)(i - (long long)r * w);
    const int n = r / h, y = r - n * h;
    const DeformEntry de = deform_entry(deform, n, N, h, w);
    const bool mine = de.mix_from >= 0 && y >= de.ry0 && y < de.ry1 && x >= de.rx0 && x < de.rx1;
    const int o = mine ? de.mix_from : n;
    const WarpEntry g = warp_entry(entries, o, slots, 8);
    float2 disp = make_float2(0.f, 0.f);
    if (field != nullptr) disp = reinterpret_cast<const float2*>(field)[((long long)o * h + y) * w + x];
    const float u = ((float)x + disp.x) - uc, v = ((float)y + disp.y) - vc;
    const float sx = warp_coord(g.a00, g.a01, g.cx, u, v, Ws), sy = warp_coord(g.a10, g.a11, g.cy, u, v, Hs);
    const int xs = (int)floorf(sx + 0.5f), ys = (int)floorf(sy + 0.5f);       // in [-1, Ws] x [-1, Hs]
    float out = 0.f;
    if (xs >= 0 && xs < Ws && ys >= 0 && ys < Hs) out = (float)masks[((long long)g.slot * Hs + ys) * Ws + xs];
    dst[i] = out;
  }
}

static int mask_resample_launch(const CachePass& p, bool deformed, const unsigned char* masks, const int* entries, const int* deform,
                                const float* field, float* dst, hipStream_t stream) {
  CACHE_REQUIRE(p.who, masks && entries && dst && (deform || !deformed), "null pointer");
  if (int e = cache_check(p)) return e;
  CACHE_REQUIRE(p.who, hpri_aligned16(entries, deform, field),
                deformed ? "the entries and the field must be 16-byte aligned" : "the entries must be 16-byte aligned");
  const dim3 grid = cache_grid(cache_pixel_blocks(p), 8), block(256);
  if (!deformed) hipLaunchKernelGGL(mask_warp_kernel, grid, block, 0, stream, masks, p.slots, p.Hs, p.Ws, entries, p.N, p.h, p.w, dst);
  else hipLaunchKernelGGL(mask_deform_kernel, grid, block, 0, stream, masks, p.slots, p.Hs, p.Ws, entries, deform, field, p.N, p.h, p.w, dst);
  HPRI_CHECK_LAUNCH();
  return HPRI_OK;
}

// masks: uint8 (slots, Hs, Ws); dst: fp32 (N, 1, h, w); the entries of hpri_cube_warp.
extern "C" int hpri_mask_warp(const unsigned char* masks, int slots, int Hs, int Ws, const int* entries, int N, int h, int w,
                              float* dst, hipStream_t stream) {
  return mask_resample_launch({"mask_warp", slots, Hs, Ws, N, h, w, false}, false, masks, entries, nullptr, nullptr, dst, stream);
}

// masks: uint8 (slots, Hs, Ws); dst: fp32 (N, 1, h, w); entries, deform and field of hpri_cube_deform.
extern "C" int hpri_mask_deform(const unsigned char* masks, int slots, int Hs, int Ws, const int* entries, const int* deform,
                                const float* field, int N, int h, int w, float* dst, hipStream_t stream) {
  return mask_resample_launch({"mask_deform", slots, Hs, Ws, N, h, w, false}, true, masks, entries, deform, field, dst, stream);
}
