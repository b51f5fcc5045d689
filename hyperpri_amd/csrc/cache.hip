// Device-resident cube cache (hyperpri_amd/cache.py): a training split is stored once in HBM, band-sliced and zero-padded
// per pixel, and every batch is ASSEMBLED from it by one gather pass that crops and flips on the way -- the reference's
// only augmentation is RandomCrop with one RNG state for image and mask (params_HyperPRI.py:201-203, dataset.py:283-293).
//
//   store   (P, B) fp32 / fp16 pixel-major cube  ->  cache slot (P, cs), cs = roundup(C, 8): bands [lo, lo+C) at channels
//           [0, C), zeros at [C, cs); element type fp32 or fp16 (fp16: half the HBM, NOT the reference's numerics).
//   gather  dst[i, y, x, 0:cs] = cache[slot_i, top_i + (flip_h ? h-1-y : y), left_i + (flip_w ? w-1-x : x), 0:cs] as fp32:
//           the (N, h, w, cs) zero-padded channels-last buffer the networks consume in place (Act.from_tensor).
//   mask    the same table, crop and flips over uint8 (slots, Hs, Ws) masks -> fp32 (N, 1, h, w).
//
// The table lives on the device: {slot, top, left, flags} per sample, four int32 (flags bit 0: flip rows, bit 1: flip
// columns).  The launchers cannot see it, so the kernels clamp slot / top / left into the cache: a bad table reads the wrong
// window, never outside the allocation (hyperpri_amd/cache.py validates on the host before it uploads).
#include "cache_launch.h"

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

extern "C" int hpri_hwb_ingest(const void* src, int src_dtype, float* dst, long long P, int B, int lo, int C, int dst_cs,
                               int dst_cw, hipStream_t stream);

// ---- store: fp16 destination (the fp32 destination is hpri_hwb_ingest's pass) ---------------------------------------
// dst[p][c] = c < C ? (half)src[p*B + lo + c] : 0     (c < cs; cs % 8 == 0; one thread per channel octet = 16 bytes)
template <typename T>
__global__ void hwb_store_f16_kernel(const T* __restrict__ src, _Float16* __restrict__ dst, long long P, int B, int lo, int C,
                                     int cs) {
  const int o = cs >> 3;
  const long long total = P * o;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long p = i / o;
    const int c = (int)(i - p * o) * 8;
    const T* s = src + p * B + lo + c;
    f16x8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = c + j < C ? (_Float16)s[j] : (_Float16)0.f;      // fp32 -> half: round to nearest even, once
    *reinterpret_cast<f16x8*>(dst + p * cs + c) = v;
  }
}

// src_dtype / dst_dtype: 0 = float32, 1 = float16
extern "C" int hpri_hwb_store(const void* src, int src_dtype, void* dst, int dst_dtype, long long P, int B, int lo, int C,
                              int cs, hipStream_t stream) {
  HPRI_REQUIRE(src && dst, "hwb_store: null pointer");
  HPRI_REQUIRE(P > 0 && B > 0 && lo >= 0 && C > 0 && lo + C <= B, "hwb_store: bad band range");
  HPRI_REQUIRE(cs % 8 == 0 && cs >= C, "hwb_store: the slot's channel stride must be a multiple of 8 that holds the bands");
  HPRI_REQUIRE((src_dtype == 0 || src_dtype == 1) && (dst_dtype == 0 || dst_dtype == 1), "hwb_store: dtypes must be 0 (f32) or 1 (f16)");
  HPRI_REQUIRE(((uintptr_t)dst & 15) == 0, "hwb_store: the slot must be 16-byte aligned");
  if (dst_dtype == 0) return hpri_hwb_ingest(src, src_dtype, (float*)dst, P, B, lo, C, cs, cs, stream);
  long long blocks = (P * (cs / 8) + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  if (src_dtype == 0)
    hipLaunchKernelGGL(hwb_store_f16_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, stream, (const float*)src,
                       (_Float16*)dst, P, B, lo, C, cs);
  else
    hipLaunchKernelGGL(hwb_store_f16_kernel<_Float16>, dim3((unsigned)blocks), dim3(256), 0, stream, (const _Float16*)src,
                       (_Float16*)dst, P, B, lo, C, cs);
  HPRI_CHECK_LAUNCH();
  return HPRI_OK;
}

// ---- batch gather ----------------------------------------------------------------------------------------------------
// Memory-bound: 16 bytes per lane both ways (8-byte loads from fp16 slots), nothing but index arithmetic in between, no LDS,
// no atomics.  The unit of work is a channel QUAD; a window row (n, y) holds w * cs/4 of them, contiguous in the destination
// and -- without a column flip -- in the source too.  A workgroup takes items of GATHER_ITEM quads of one row (grid-stride
// over (row, piece)), so slot / row / flip are uniform per item and only the column flip costs a per-lane division; every
// lane issues its GATHER_UNROLL loads before the first store.  Slot offsets are 64-bit (45 slots hold 6.4 G elements).
#define GATHER_THREADS 256
#define GATHER_UNROLL 4
#define GATHER_ITEM (GATHER_THREADS * GATHER_UNROLL)

struct GatherEntry { int slot, top, left, flags; };

__device__ __forceinline__ GatherEntry gather_entry(const int* __restrict__ table, int n, int slots, int Hs, int Ws, int h, int w) {
  const int4 e = *reinterpret_cast<const int4*>(table + 4 * (size_t)n);
  GatherEntry g;
  g.slot = min(max(e.x, 0), slots - 1);
  g.top = min(max(e.y, 0), Hs - h);
  g.left = min(max(e.z, 0), Ws - w);
  g.flags = e.w;
  return g;
}

__device__ __forceinline__ f32x4 gather_load(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ f32x4 gather_load(const _Float16* p) {
  const f16x4 v = *reinterpret_cast<const f16x4*>(p);
  f32x4 r;
  r[0] = (float)v[0]; r[1] = (float)v[1]; r[2] = (float)v[2]; r[3] = (float)v[3];
  return r;
}

template <typename T>
__global__ __launch_bounds__(GATHER_THREADS) void cube_gather_kernel(const T* __restrict__ cache, int slots, int Hs, int Ws, int q,
                                                                     const int* __restrict__ table, int N, int h, int w,
                                                                     float* __restrict__ dst) {
  const int rowq = w * q;                                             // quads per window row (< 2^31: checked by the launcher)
  const int pieces = (rowq + GATHER_ITEM - 1) / GATHER_ITEM;
  const long long items = (long long)N * h * pieces;
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    const int r = (int)(it / pieces), piece = (int)(it - (long long)r * pieces);
    const int n = r / h, y = r - n * h;
    const GatherEntry g = gather_entry(table, n, slots, Hs, Ws, h, w);
    const int ys = g.top + ((g.flags & 1) ? h - 1 - y : y);
    const T* s = cache + (((long long)g.slot * Hs + ys) * Ws + g.left) * (4LL * q);
    float* d = dst + (long long)r * rowq * 4LL;
    const bool fw = (g.flags & 2) != 0;
    f32x4 v[GATHER_UNROLL];
    const int j0 = piece * GATHER_ITEM + threadIdx.x;
#pragma unroll
    for (int u = 0; u < GATHER_UNROLL; ++u) {
      const int j = j0 + u * GATHER_THREADS;
      if (j < rowq) {
        int sj = j;
        if (fw) {                                                     // pixel x comes from pixel w-1-x: the quad keeps its channel
          const int x = j / q;
          sj = (w - 1 - x) * q + (j - x * q);
        }
        v[u] = gather_load(s + 4LL * sj);
      }
    }
#pragma unroll
    for (int u = 0; u < GATHER_UNROLL; ++u) {
      const int j = j0 + u * GATHER_THREADS;
      if (j < rowq) *reinterpret_cast<f32x4*>(d + 4LL * j) = v[u];
    }
  }
}

// cache_dtype: 0 = float32, 1 = float16.  cache: (slots, Hs, Ws, cs); table: N entries of 4 int32 on the device; dst: (N, h, w, cs) fp32.
extern "C" int hpri_cube_gather(const void* cache, int cache_dtype, int slots, int Hs, int Ws, int cs, const int* table, int N,
                                int h, int w, float* dst, hipStream_t stream) {
  const CachePass p = {"cube_gather", slots, Hs, Ws, N, h, w, true};
  CACHE_REQUIRE(p.who, cache && table && dst, "null pointer");
  const CacheSlots c = {cache_dtype, cs, cs};
  if (int e = cache_check(p, &c)) return e;
  CACHE_REQUIRE(p.who, hpri_aligned16(cache, dst, table), "buffers must be 16-byte aligned");
  const int q = cs / 4;
  const dim3 grid = cache_grid(cache_row_items(p, q, GATHER_ITEM), 8);  // eight workgroups per CU, grid-stride over the rest
  if (cache_dtype == 0)
    hipLaunchKernelGGL(cube_gather_kernel<float>, grid, dim3(GATHER_THREADS), 0, stream, (const float*)cache, slots, Hs, Ws, q, table, N,
                       h, w, dst);
  else
    hipLaunchKernelGGL(cube_gather_kernel<_Float16>, grid, dim3(GATHER_THREADS), 0, stream, (const _Float16*)cache, slots, Hs, Ws, q,
                       table, N, h, w, dst);
  HPRI_CHECK_LAUNCH();
  return HPRI_OK;
}

// ---- mask gather: 0.4 % of the cube's bytes; one output pixel per thread, coalesced fp32 stores ----------------------
__global__ void mask_gather_kernel(const unsigned char* __restrict__ masks, int slots, int Hs, int Ws, const int* __restrict__ table,
                                   int N, int h, int w, float* __restrict__ dst) {
  const long long total = (long long)N * h * w;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int r = (int)(i / w), x = (int)(i - (long long)r * w);
    const int n = r / h, y = r - n * h;
    const GatherEntry g = gather_entry(table, n, slots, Hs, Ws, h, w);
    const int ys = g.top + ((g.flags & 1) ? h - 1 - y : y);
    const int xs = g.left + ((g.flags & 2) ? w - 1 - x : x);
    dst[i] = (float)masks[((long long)g.slot * Hs + ys) * Ws + xs];
  }
}

// masks: uint8 (slots, Hs, Ws); dst: fp32 (N, 1, h, w); the table of hpri_cube_gather.
extern "C" int hpri_mask_gather(const unsigned char* masks, int slots, int Hs, int Ws, const int* table, int N, int h, int w,
                                float* dst, hipStream_t stream) {
  const CachePass p = {"mask_gather", slots, Hs, Ws, N, h, w, true};
  CACHE_REQUIRE(p.who, masks && table && dst, "null pointer");
  if (int e = cache_check(p)) return e;
  CACHE_REQUIRE(p.who, hpri_aligned16(table), "the table must be 16-byte aligned");
  hipLaunchKernelGGL(mask_gather_kernel, cache_grid(cache_pixel_blocks(p), 8), dim3(256), 0, stream, masks, slots, Hs, Ws, table, N, h, w,
                     dst);
  HPRI_CHECK_LAUNCH();
  return HPRI_OK;
}
