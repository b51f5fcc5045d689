// What the passes over the band axis of the cube cache's slots share (spectral.hip: moments, Gram; cluster.hip: k-means sums): the
// constants of the summation rule, the widening loads, the selection, the cut of a slot list into runs and the argument checks.
// Each once; spectral.hip states the rule itself.
#pragma once
#include "cache_launch.h"

#define BAND_FP32_RUN 2048              // pixels a sum spends in fp32 before it is promoted (documented: <= 4096)
#define BAND_MAX_CS 320                 // ten 32-band blocks: 55 block pairs, at most 14 per wave
#define BAND_THREADS 256
#define BAND_LDS_BYTES (160 * 1024)

#ifdef __HIPCC__
__device__ __forceinline__ f32x4 band_load(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ f32x4 band_load(const _Float16* p) {
  const f16x4 v = *reinterpret_cast<const f16x4*>(p);
  f32x4 r;
  r[0] = (float)v[0]; r[1] = (float)v[1]; r[2] = (float)v[2]; r[3] = (float)v[3];
  return r;
}

// the same 16 (8) bytes as they come, widened later: a load whose value is not touched does not stall the wave that issued it
__device__ __forceinline__ f32x4 band_raw(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ f16x4 band_raw(const _Float16* p) { return *reinterpret_cast<const f16x4*>(p); }
__device__ __forceinline__ f32x4 band_widen(f32x4 v) { return v; }
__device__ __forceinline__ f32x4 band_widen(f16x4 v) {
  f32x4 r;
  r[0] = (float)v[0]; r[1] = (float)v[1]; r[2] = (float)v[2]; r[3] = (float)v[3];
  return r;
}

__device__ __forceinline__ bool band_selected(const unsigned char* __restrict__ masks, long long pixel, int select) {
  if (select == 0) return true;
  return (masks[pixel] != 0) == (select == 1);
}

struct BandRun { long long base; int len; };     // first pixel (slot * P + offset inside the slot) and length of a run

__device__ __forceinline__ BandRun band_run(const int* __restrict__ table, int slots, long long P, int runs_per_slot, long long r) {
  const int e = (int)(r / runs_per_slot), k = (int)(r - (long long)e * runs_per_slot);
  const int slot = min(max(table[e], 0), slots - 1);
  const long long p0 = (long long)k * BAND_FP32_RUN;
  BandRun b;
  b.base = (long long)slot * P + p0;
  b.len = (int)min((long long)BAND_FP32_RUN, P - p0);
  return b;
}
#endif

// a pixel row of a tile in LDS (band_project_kernel, band_detect_kernel, cluster.hip): cs + 2 words rounded up to 2 (mod 32), so the
// 32 lanes of a ds_read_b32 group (2 i + k) hit 32 banks; even, the rows are written as 8-byte pairs; at least roundup(cs, 32) + 2
static inline __host__ __device__ int band_tile_stride(int cs) { return cs + 2 + ((32 - (cs & 31)) & 31); }

// ---- host: what a pass over the slots requires of its arguments, in the order it is reported -----------------------------------
struct BandPass { const char* who; const void* cache; int dtype, slots, Hs, Ws, cs; const unsigned char* masks; const int* table; int n, select; };

static inline int band_check(const BandPass& p, const void* workspace, size_t workspace_bytes, size_t need) {
  CACHE_REQUIRE(p.who, p.cache && p.table && workspace, "null pointer");
  CACHE_REQUIRE(p.who, p.dtype == 0 || p.dtype == 1, "cache_dtype must be 0 (f32) or 1 (f16)");
  CACHE_REQUIRE(p.who, p.slots > 0 && p.Hs > 0 && p.Ws > 0 && p.n > 0, "bad sizes");
  CACHE_REQUIRE(p.who, p.cs > 0 && p.cs % 8 == 0 && p.cs <= BAND_MAX_CS, "the channel stride must be a multiple of 8 up to hpri_band_max_cs");
  CACHE_REQUIRE(p.who, p.select >= 0 && p.select <= 2, "select must be 0 (all), 1 (foreground) or 2 (background)");
  CACHE_REQUIRE(p.who, p.select == 0 || p.masks, "a selection needs the masks");
  CACHE_REQUIRE(p.who, workspace_bytes >= need, "the workspace is smaller than hpri_band_workspace_bytes");
  CACHE_REQUIRE(p.who, hpri_aligned16(p.cache, workspace) && ((uintptr_t)p.table & 3) == 0, "buffers must be 16-byte aligned");
  return HPRI_OK;
}
