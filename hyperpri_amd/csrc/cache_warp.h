// What the warp kernels (cache_warp.hip) and the deforming ones (cache_deform.hip) share: the 64-byte warp entry as the kernels
// read and clamp it, the clamped source coordinate, and the load / arithmetic forms of a channel quad.
#pragma once
#include "common.h"

typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

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
