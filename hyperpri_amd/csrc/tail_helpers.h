// The rules the kernels of a step's tail share (step.hip, segmap.hip, multiclass.hip, segloss.hip, components.hip, distance.hip,
// skeleton.hip, sort.hip, guided.hip, ridge.hip, the band family and the cube cache's launchers): every rule once.  They carry the reproducibility promise -- fp64 sums
// in a fixed order, fixed butterflies, integer atomics only -- so a new tail kernel takes them from here and restates none of them.
#pragma once
#include "common.h"

// ---- host: grids and alignment ---------------------------------------------------------------------------------------------------
#define HPRI_MAX_BLOCKS 1024             // the cap of the passes whose per-block partial sums a one-block finish adds up

// blocks = min(ceil(items / per_block), per_cu x CUs), at least 1: the kernels stride over the rest.  (The floor matters only to a
// launcher that admits items == 0; segmap.hip and the cube cache had none and check their sizes first, so it changes nothing there.)
static inline int hpri_grid_per_cu(long long items, int per_block, int per_cu) {
  long long blocks = (items + per_block - 1) / per_block;
  const long long cap = (long long)per_cu * hpri_cu_count();
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  return (int)blocks;
}

// blocks = min(ceil(items / per_block), HPRI_MAX_BLOCKS), at least 1
static inline int hpri_grid_capped(long long items, int per_block) {
  long long blocks = (items + per_block - 1) / per_block;
  if (blocks > HPRI_MAX_BLOCKS) blocks = HPRI_MAX_BLOCKS;
  if (blocks < 1) blocks = 1;
  return (int)blocks;
}

// every pointer 16-byte aligned (a null pointer is)
template <typename... P> static inline bool hpri_aligned16(P... ptr) { return ((((uintptr_t)ptr) | ...) & 15) == 0; }

// ---- host: a launch with more than 64 KB of dynamic LDS -------------------------------------------------------------------------
// More than 64 KB has to be asked for, per kernel and device; a runtime that needs no such request may refuse it, and the refusal is
// forgotten: the launch reports what matters.
template <class K> static inline void hpri_ask_dynamic_lds(K kernel, size_t bytes) {
  if (bytes > 64 * 1024 && hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess)
    (void)hipGetLastError();
}

#ifdef __HIPCC__
// ---- the logit of a score in [0, 1], clamped to [2^-24, 1 - 2^-24]: finite for every input, NaN aside -------------------------------
#define HPRI_P_LO 5.9604644775390625e-08f    // 2^-24
#define HPRI_P_HI 0.99999994039535522f       // 1 - 2^-24
__device__ __forceinline__ float hpri_clamped_logit(float s) {
  const float p = fminf(fmaxf(s, HPRI_P_LO), HPRI_P_HI);
  return logf(p) - log1pf(-p);
}

// ---- a wave's 64 lanes: xor butterfly 32 .. 1, the result in every lane ------------------------------------------------------------
template <typename T> __device__ __forceinline__ T hpri_wave_sum(T v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ int hpri_wave_max(int v) {
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
  return v;
}

// ---- a workgroup's R fp64 sums: the halving tree red[r][t] += red[r][t + w], w = THREADS/2 .. 1, a barrier after each level --------
// Every thread calls it; red[r][0] holds the sums afterwards.  (A caller that comes back with the next sums puts a barrier between.)
template <int R, int THREADS>
__device__ __forceinline__ void hpri_block_sum(double (*red)[THREADS], const double (&s)[R]) {
#pragma unroll
  for (int r = 0; r < R; ++r) red[r][threadIdx.x] = s[r];
  __syncthreads();
  for (int w = THREADS / 2; w > 0; w >>= 1) {
    if (threadIdx.x < w) {
#pragma unroll
      for (int r = 0; r < R; ++r) red[r][threadIdx.x] += red[r][threadIdx.x + w];
    }
    __syncthreads();
  }
}

// ---- four counters of a workgroup: wave sums, LDS atomics, then one 64-bit atomic per counter that is not zero ----------------------
// count(c) adds this thread's share to c[0..3]; every thread of the workgroup calls the helper.
template <class Count>
__device__ __forceinline__ void hpri_block_count4(unsigned long long* __restrict__ out, Count&& count) {
  __shared__ unsigned int red[4];
  if (threadIdx.x < 4) red[threadIdx.x] = 0;
  __syncthreads();
  unsigned int c[4] = {0, 0, 0, 0};
  count(c);
  for (int k = 0; k < 4; ++k) {
    const unsigned int v = hpri_wave_sum(c[k]);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(&red[k], v);
  }
  __syncthreads();
  if (threadIdx.x < 4 && red[threadIdx.x]) atomicAdd(&out[threadIdx.x], (unsigned long long)red[threadIdx.x]);
}

// ---- four adjacent floats: one 16-byte access (vec), else the first cnt elements; a load leaves zeros past cnt ---------------------
__device__ __forceinline__ void hpri_load4(const float* __restrict__ p, int cnt, int vec, float (&x)[4]) {
  if (vec) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = v[j];
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = j < cnt ? p[j] : 0.f;
  }
}

__device__ __forceinline__ void hpri_store4(float* __restrict__ p, int cnt, int vec, const float (&x)[4]) {
  if (vec) {
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = x[j];
    *reinterpret_cast<f32x4*>(p) = v;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < cnt) p[j] = x[j];
  }
}

// ---- sp = sigmoid(x), sn = sigmoid(-x) and (WITH_LOG) lg = log1p(exp(-|x|)) from one exponential -----------------------------------
// Neither sigmoid is formed as 1 - the other: a confident pixel keeps its relative accuracy on both sides.
template <int WITH_LOG>
__device__ __forceinline__ void hpri_sigmoids(float x, float& sp, float& sn, float& lg) {
  const float e = expf(-fabsf(x)), r = 1.f / (1.f + e);
  sp = x >= 0.f ? r : e * r;
  sn = x >= 0.f ? e * r : r;
  lg = WITH_LOG ? log1pf(e) : 0.f;
}

__device__ __forceinline__ void hpri_sigmoids(float x, float& sp, float& sn) {
  float lg;
  hpri_sigmoids<0>(x, sp, sn, lg);
}
#endif
