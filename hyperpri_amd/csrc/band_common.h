// What the kernels over the band axis share, each once.
// The passes over the cube cache's slots (spectral.hip: moments, Gram; cluster.hip: k-means sums; unmix.hip: the ATGP step): the
// constants of the summation rule, the widening loads, the selection, the cut of a slot list into runs and the argument checks;
// spectral.hip states the rule itself.
// The batch-tile pipeline (band_project_kernel, band_detect_kernel, band_assign_kernel, band_cluster_kernel, band_unmix_kernel,
// band_extreme_kernel): the row stride of a tile in LDS, the tile load and stage, the score rows in LDS and the MFMA chain over them.
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

// ---- the batch-tile pipeline ------------------------------------------------------------------------------------------------------
// a pixel row of a tile in LDS: cs + 2 words rounded up to 2 (mod 32), so the 32 lanes of a ds_read_b32 group (2 i + k) hit 32 banks;
// even, the rows are written as 8-byte pairs; at least roundup(cs, 32) + 2
static inline __host__ __device__ int band_tile_stride(int cs) { return cs + 2 + ((32 - (cs & 31)) & 31); }

// words of a row of the score rows in LDS: NKB blocks of 16 rows, rounded up to 32
static inline __host__ __device__ int band_kp(int nkb) { return (nkb * 16 + 31) & ~31; }

// the channel strides the family takes
static inline bool band_cs_ok(int cs) { return cs > 0 && cs % 8 == 0 && cs <= BAND_MAX_CS; }

#ifdef __HIPCC__
// Tile load: quad lt + u THREADS of the tile that starts at src, global -> registers as it comes (band_raw), zeros from quad `left`
// on (left = the tile's pixels inside the batch or the slot, times the quads of a pixel).
template <int LOADS, int THREADS, typename T, typename V>
__device__ __forceinline__ void band_tile_load(V (&v)[LOADS], const T* __restrict__ src, int lt, int left) {
#pragma unroll
  for (int u = 0; u < LOADS; ++u) {
    const int idx = lt + u * THREADS;
    v[u] = V{};
    if (idx < left) v[u] = band_raw(src + 4 * idx);
  }
}

// Tile stage: the first `total` quads held in registers (the tile's pixels times ql, the quads of a pixel) -> pixel rows in LDS at a
// stride of ldx, widened, through f (the identity, or (quad, cq) -> what is stored for channel quad cq), as 8-byte pairs.  The caller
// hides ql from the optimiser per tile (asm volatile("" : "+s"(ql))): the quotients idx / ql and the addresses made of them would
// otherwise be computed once and held in registers across the k loops.
template <int LOADS, int THREADS, typename V, class F>
__device__ __forceinline__ void band_tile_stage(float* __restrict__ xl, const V (&v)[LOADS], int lt, int total, int ql, int ldx, F&& f) {
#pragma unroll
  for (int u = 0; u < LOADS; ++u) {
    const int idx = lt + u * THREADS;
    if (idx < total) {
      const int px = idx / ql, cq = idx - px * ql;
      const f32x4 w = f(band_widen(v[u]), cq);
      float2* d = reinterpret_cast<float2*>(xl + px * ldx + 4 * cq);
      d[0] = float2{w[0], w[1]};
      d[1] = float2{w[2], w[3]};
    }
  }
}
struct BandQuadAsIs { __device__ __forceinline__ f32x4 operator()(f32x4 w, int) const { return w; } };

// Score rows.  v_mfma_f32_16x16x4_f32 with i = row, j = pixel, k = band: lane l holds A[i = l & 15][k = l >> 4] = W[i][c + k] and
// B[k][j = l & 15] = d[pixel j][c + k]; D: column (pixel) = l & 15, row = 4 (l >> 4) + reg, so a lane ends with four consecutive rows
// of one pixel.  W sits transposed in LDS for the workgroup's lifetime: wl[c][kp], kp = band_kp(NKB), column n of row c at
// n ^ 16 (c & 1), so that the two k of a 32-lane group fall into different halves of the banks.
template <int NKB> struct BandRows { f32x4 b4[NKB]; int woff[NKB]; };   // this lane's bias quads and column offsets (rows c + kq: their parity is kq's)

template <int NKB>
__device__ __forceinline__ void band_stage_rows(float* __restrict__ wl, const float* __restrict__ W, const float* __restrict__ bias, int cs,
                                                int ks, int t, int col, int kq, BandRows<NKB>& rows) {
  const int kp = band_kp(NKB);
  for (int i = t; i < cs * kp; i += BAND_THREADS) {
    const int c = i / kp, n = i - c * kp;
    wl[c * kp + (n ^ ((c & 1) << 4))] = n < ks ? W[(long long)n * cs + c] : 0.f;
  }
#pragma unroll
  for (int kb = 0; kb < NKB; ++kb) {
    const int n0 = kb * 16 + kq * 4;
    rows.woff[kb] = (kb * 16 + col) ^ ((kq & 1) << 4);
    rows.b4[kb] = n0 < ks ? *reinterpret_cast<const f32x4*>(bias + n0) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
}

// z of this lane's pixel (xr = its row in LDS + kq, wr = wl + kq kp) against every block of 16 rows: the chain over c ascends, started
// from the bias, bit for bit fmaf(W[k][cs-1], d[cs-1], ... fmaf(W[k][0], d[0], b[k])).  DIAG: also the 16 x 16 products of the wave's
// pixels with themselves, whose diagonal is s = fmaf(d[c], d[c], s).  cs % 8 == 0: two k-steps per iteration, the next iteration's
// operands read from LDS before this one's MFMAs issue (the last iteration reads its own again).
template <int NKB, bool DIAG>
__device__ __forceinline__ void band_scores(const float* __restrict__ xr, const float* __restrict__ wr, const BandRows<NKB>& rows, int cs,
                                            f32x4 (&acc)[NKB], f32x4& accd) {
  const int kp = band_kp(NKB);
#pragma unroll
  for (int kb = 0; kb < NKB; ++kb) acc[kb] = rows.b4[kb];
  accd = f32x4{0.f, 0.f, 0.f, 0.f};
  float x0 = xr[0], x1 = xr[4], w0[NKB], w1[NKB];
#pragma unroll
  for (int kb = 0; kb < NKB; ++kb) { w0[kb] = wr[rows.woff[kb]]; w1[kb] = wr[4 * kp + rows.woff[kb]]; }
  for (int c = 0; c < cs; c += 8) {
    const int cn = min(c + 8, cs - 8);
    const float nx0 = xr[cn], nx1 = xr[cn + 4];
    float nw0[NKB], nw1[NKB];
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) { nw0[kb] = wr[cn * kp + rows.woff[kb]]; nw1[kb] = wr[(cn + 4) * kp + rows.woff[kb]]; }
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) acc[kb] = __builtin_amdgcn_mfma_f32_16x16x4f32(w0[kb], x0, acc[kb], 0, 0, 0);
    if (DIAG) accd = __builtin_amdgcn_mfma_f32_16x16x4f32(x0, x0, accd, 0, 0, 0);
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) acc[kb] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1[kb], x1, acc[kb], 0, 0, 0);
    if (DIAG) accd = __builtin_amdgcn_mfma_f32_16x16x4f32(x1, x1, accd, 0, 0, 0);
    x0 = nx0; x1 = nx1;
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) { w0[kb] = nw0[kb]; w1[kb] = nw1[kb]; }
  }
}
#endif

// ---- host: what a pass over the slots requires of its arguments, in the order it is reported -----------------------------------
struct BandPass { const char* who; const void* cache; int dtype, slots, Hs, Ws, cs; const unsigned char* masks; const int* table; int n, select; };

static inline int band_check(const BandPass& p, const void* workspace, size_t workspace_bytes, size_t need) {
  CACHE_REQUIRE(p.who, p.cache && p.table && workspace, "null pointer");
  CACHE_REQUIRE(p.who, p.dtype == 0 || p.dtype == 1, "cache_dtype must be 0 (f32) or 1 (f16)");
  CACHE_REQUIRE(p.who, p.slots > 0 && p.Hs > 0 && p.Ws > 0 && p.n > 0, "bad sizes");
  CACHE_REQUIRE(p.who, band_cs_ok(p.cs), "the channel stride must be a multiple of 8 up to hpri_band_max_cs");
  CACHE_REQUIRE(p.who, p.select >= 0 && p.select <= 2, "select must be 0 (all), 1 (foreground) or 2 (background)");
  CACHE_REQUIRE(p.who, p.select == 0 || p.masks, "a selection needs the masks");
  CACHE_REQUIRE(p.who, workspace_bytes >= need, "the workspace is smaller than hpri_band_workspace_bytes");
  CACHE_REQUIRE(p.who, hpri_aligned16(p.cache, workspace) && ((uintptr_t)p.table & 3) == 0, "buffers must be 16-byte aligned");
  return HPRI_OK;
}
