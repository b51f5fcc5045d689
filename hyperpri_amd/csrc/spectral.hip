// Spectral statistics and projection (hyperpri_amd/spectral.py): the band axis of the cube cache's slots.
//
//   moments  count and per-band sums of the selected pixels of a list of slots (optionally the sums of squares about a pivot)
//   gram     G[i][j] = sum over the selected pixels of (x[i] - pivot[i]) * (x[j] - pivot[j]), on the exact fp32 MFMA
//   project  y[p][k] = b[k] + sum_c W[k][c] * x[p][c] over a zero-padded channels-last fp32 batch, on the exact fp32 MFMA
//   affine   y[p][c] = fmaf(x[p][c], s[c], t[c]): the diagonal case
//
// The slots are read exactly as cache.hip reads them: (slots, Hs, Ws, cs) fp32 or fp16, cs % 8 == 0, zeros above the bands; masks
// (slots, Hs, Ws) uint8.  The list of slots is a device table of int32; the kernels clamp its entries into the cache (a bad table
// reads the wrong slot, never outside the allocation; spectral.py validates on the host).
//
// Determinism of moments and gram.  The pixels of list entry e are cut into RUNS of BAND_FP32_RUN pixels (the last one shorter); run
// r of the launch is run r % runs_per_slot of entry r / runs_per_slot.  A sum stays in fp32 inside one run and is then added into an
// fp64 PARTIAL accumulator; partial a owns the runs a, a + NPART, a + 2 NPART, ... in that order (NPART = BAND_MOMENT_PARTS or
// BAND_GRAM_PARTS: constants, not the CU count), one workgroup per partial.  A finishing kernel adds the partials 0, 1, 2, ... in
// fp64.  No floating-point atomic anywhere: the bits depend on the arguments and on these constants only.  The partials live in the
// caller's workspace, whose size (hpri_band_workspace_bytes) depends on cs alone.
#include "band_common.h"                // BAND_FP32_RUN, BAND_MAX_CS, the loads, the selection, the runs, band_check; the batch-tile pipeline

#define BAND_MOMENT_PARTS 2048          // partial accumulators of the moments pass (memory-bound: eight workgroups per CU)
#define BAND_GRAM_PARTS 256             // partial accumulators of the Gram pass (MFMA-bound: one wave per SIMD)
#define GRAM_CHUNK 16                   // pixels staged in LDS at a time
#define GRAM_MAXP 14                    // block pairs per wave
#define GRAM_LOADS ((GRAM_CHUNK * (BAND_MAX_CS / 4) + BAND_THREADS - 1) / BAND_THREADS)
#define PROJ_TILE 64                    // pixels per workgroup tile: 16 per wave
#define PROJ_MAX_K 64
#define PROJ_LOADS ((PROJ_TILE * (BAND_MAX_CS / 4) + BAND_THREADS - 1) / BAND_THREADS)

// ---- moments ---------------------------------------------------------------------------------------------------------
// One workgroup per partial.  Thread t holds channel quad t % q of the pixels t / q, t / q + npl, ... of a run (q = cs / 4,
// npl = 256 / q pixel lanes): a row of the slot is q consecutive 16-byte (fp16: 8-byte) loads.  Per run an fp32 sum, then fp64.
template <typename T>
__global__ __launch_bounds__(BAND_THREADS) void band_moments_kernel(const T* __restrict__ cache, const unsigned char* __restrict__ masks,
                                                                    const int* __restrict__ table, int slots, long long P, int q,
                                                                    int runs_per_slot, long long runs, int select,
                                                                    const float* __restrict__ pivot, double* __restrict__ part_sum,
                                                                    double* __restrict__ part_sq, long long* __restrict__ part_cnt) {
  __shared__ double red[BAND_THREADS * 4];
  __shared__ long long redc[BAND_THREADS];
  const int t = threadIdx.x, npl = BAND_THREADS / q;
  const int pl = t / q, cq = t - pl * q;
  const bool live = pl < npl;
  const int cs = 4 * q;
  f32x4 pv = {0.f, 0.f, 0.f, 0.f};
  if (pivot != nullptr && live) pv = *reinterpret_cast<const f32x4*>(pivot + 4 * cq);
  double s[4] = {0., 0., 0., 0.}, s2[4] = {0., 0., 0., 0.};
  long long cnt = 0;
  for (long long r = blockIdx.x; r < runs; r += BAND_MOMENT_PARTS) {
    const BandRun run = band_run(table, slots, P, runs_per_slot, r);
    f32x4 a = {0.f, 0.f, 0.f, 0.f}, a2 = {0.f, 0.f, 0.f, 0.f};
    int c = 0;
    if (live) {
#pragma unroll 4
      for (int i = pl; i < run.len; i += npl) {
        const long long pix = run.base + i;
        if (band_selected(masks, pix, select)) {
          const f32x4 x = band_load(cache + pix * cs + 4 * cq);
          ++c;
          if (pivot != nullptr) {
            const f32x4 d = x - pv;
            a += d;
#pragma unroll
            for (int j = 0; j < 4; ++j) a2[j] = fmaf(d[j], d[j], a2[j]);
          } else {
            a += x;
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) { s[j] += (double)a[j]; s2[j] += (double)a2[j]; }
    cnt += c;
  }
  // the pixel lanes of a quad, added in ascending order by the thread of pixel lane 0
  const int passes = part_sq != nullptr ? 2 : 1;
  for (int pass = 0; pass < passes; ++pass) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) red[4 * t + j] = pass == 0 ? s[j] : s2[j];
    if (pass == 0) redc[t] = cnt;
    __syncthreads();
    if (t < q) {
      double o[4] = {0., 0., 0., 0.};
      for (int l = 0; l < npl; ++l)
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] += red[4 * (l * q + t) + j];
      double* dst = (pass == 0 ? part_sum : part_sq) + (long long)blockIdx.x * cs + 4 * t;
#pragma unroll
      for (int j = 0; j < 4; ++j) dst[j] = o[j];
    }
    if (pass == 0 && t == 0) {
      long long n = 0;
      for (int l = 0; l < npl; ++l) n += redc[l * q];
      part_cnt[blockIdx.x] = n;
    }
  }
}

__global__ void band_moments_finish_kernel(const double* __restrict__ part_sum, const double* __restrict__ part_sq,
                                           const long long* __restrict__ part_cnt, int parts, int cs, long long* __restrict__ count,
                                           double* __restrict__ sums, double* __restrict__ sumsq) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < cs) {
    double a = 0., b = 0.;
    for (int p = 0; p < parts; ++p) a += part_sum[(long long)p * cs + c];
    sums[c] = a;
    if (sumsq != nullptr) {
      for (int p = 0; p < parts; ++p) b += part_sq[(long long)p * cs + c];
      sumsq[c] = b;
    }
  }
  if (c == 0) {
    long long n = 0;
    for (int p = 0; p < parts; ++p) n += part_cnt[p];
    *count = n;
  }
}

// ---- Gram matrix -----------------------------------------------------------------------------------------------------
// v_mfma_f32_32x32x2_f32: D (32 x 32) += A (32 x 2) B (2 x 32); lane l holds A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31].
// With k a PIXEL and i, j bands, the operand of band block b is the same register for both sides: d[pixel k][32 b + (l & 31)].  A
// workgroup stages GRAM_CHUNK pixels x all bands in LDS as d = x - pivot (zeros for pixels that are not selected or past the run,
// and for the columns between cs and the next multiple of 32), and its four waves share the upper-triangle block pairs (pair t
// goes to wave t % 4; the kernel is instantiated for 1, 2, 4, 7, 9 and 14 pairs per wave, so that every accumulator index is a
// constant and no MFMA sits under a branch).  A step is two pixels: one MFMA per pair, two ds_read_b32 per MFMA (rows of 32
// consecutive words: no bank conflict).  The next chunk travels global -> registers untouched while this one is multiplied; it is
// widened, pivoted and selected when it is stored to LDS, so no wave waits for a load it has just issued.  D: column = l & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (l >> 5).  After a run the fp32 tiles are added into the fp64
// tiles of the workgroup's partial in the workspace (32 x 32 doubles per pair, L2-resident).
__device__ __forceinline__ int gram_pairs(int nb) { return nb * (nb + 1) / 2; }
__host__ __device__ __forceinline__ int gram_pair_index(int nb, int bi, int bj) { return bi * nb - bi * (bi - 1) / 2 + (bj - bi); }

template <typename T, int NP>
__global__ __launch_bounds__(BAND_THREADS) void band_gram_kernel(const T* __restrict__ cache, const unsigned char* __restrict__ masks,
                                                                 const int* __restrict__ table, int slots, long long P, int q,
                                                                 int runs_per_slot, long long runs, int select,
                                                                 const float* __restrict__ pivot, double* __restrict__ part) {
  extern __shared__ float gl[];                        // [GRAM_CHUNK][ldw] staged pixels, then [cs] pivot
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int cs = 4 * q, nb = (cs + 31) >> 5, ldw = nb * 32, npairs = nb * (nb + 1) / 2;
  float* pl = gl + GRAM_CHUNK * ldw;
  for (int i = t; i < GRAM_CHUNK * ldw; i += BAND_THREADS) gl[i] = 0.f;        // (the columns [cs, ldw) stay zero)
  for (int i = t; i < cs; i += BAND_THREADS) pl[i] = pivot[i];
  // this wave's pairs: t = wave, wave + 4, ...
  // packed, one byte per slot (bi | bj << 4), four slots per word: as 28 words the block indices and the LDS offsets made of
  // them outgrow the scalar registers.  (A slot beyond the wave's pairs repeats pair (0, 0) and is never written back.)
  unsigned pk[4] = {0u, 0u, 0u, 0u};
  int cnt = 0;
  {
    int bi = 0, bj = 0;
    for (int p = 0; p < npairs; ++p) {
      if ((p & 3) == wave) {
#pragma unroll
        for (int w = 0; w < 4; ++w)
          if (w == (cnt >> 2)) pk[w] |= (unsigned)(bi | (bj << 4)) << (8 * (cnt & 3));
        ++cnt;
      }
      if (++bj == nb) { ++bi; bj = bi; }
    }
  }
  const int total = GRAM_CHUNK * q;                    // quads of a chunk: one contiguous span of the slot
  const int row = lane & 31, half = lane >> 5;
  // the workgroup's partial starts from zero (the barriers of the first chunk order these stores before the first promotion)
  for (int i = t; i < npairs * 1024; i += BAND_THREADS) part[(long long)blockIdx.x * npairs * 1024 + i] = 0.;
  for (long long r = blockIdx.x; r < runs; r += BAND_GRAM_PARTS) {
    const BandRun run = band_run(table, slots, P, runs_per_slot, r);
    f32x16 acc[NP];
#pragma unroll
    for (int s = 0; s < NP; ++s)
#pragma unroll
      for (int j = 0; j < 16; ++j) acc[s][j] = 0.f;
    // a chunk's quads as loaded (widened, pivoted and selected when they are stored into LDS, one chunk later) and their pixel's mask
    // byte (-1: past the run)
    decltype(band_raw(cache)) v[GRAM_LOADS];
    int keep[GRAM_LOADS];
    auto load = [&](int c0, int ql) {
#pragma unroll
      for (int u = 0; u < GRAM_LOADS; ++u) {
        const int idx = t + u * BAND_THREADS;
        keep[u] = -1;
        if (idx < total) {
          const int px = idx / ql, cq = idx - px * ql;
          if (c0 + px < run.len) {
            const long long pix = run.base + c0 + px;
            v[u] = band_raw(cache + pix * cs + 4 * cq);
            keep[u] = select == 0 ? 1 : (int)masks[pix];
          }
        }
      }
    };
    __syncthreads();                                   // (the pivot is in LDS; the previous run's last chunk has been consumed)
    // (q is hidden from the optimiser per chunk: the ten quotients idx / q would otherwise be computed once, held in registers
    // for the kernel's lifetime and spilled beside the fourteen accumulator tiles)
    int ql = q;
    asm volatile("" : "+s"(ql));
    load(0, ql);
    for (int c0 = 0; c0 < run.len; c0 += GRAM_CHUNK) {
      __syncthreads();
      asm volatile("" : "+s"(ql));
#pragma unroll
      for (int u = 0; u < GRAM_LOADS; ++u) {
        const int idx = t + u * BAND_THREADS;
        if (idx < total) {
          const int px = idx / ql, cq = idx - px * ql;
          const bool on = keep[u] >= 0 && (select == 0 || (keep[u] != 0) == (select == 1));
          f32x4 d = {0.f, 0.f, 0.f, 0.f};
          if (on) d = band_widen(v[u]) - *reinterpret_cast<const f32x4*>(pl + 4 * cq);
          *reinterpret_cast<f32x4*>(gl + px * ldw + 4 * cq) = d;
        }
      }
      __syncthreads();
      if (c0 + GRAM_CHUNK < run.len) load(c0 + GRAM_CHUNK, ql);
#pragma unroll 2
      for (int k = 0; k < GRAM_CHUNK; k += 2) {
        const float* base = gl + (k + half) * ldw + row;
        // (unpacked again at every step, in vector registers: a few VALU instructions beside every MFMA, which leaves them idle)
        unsigned w0 = pk[0], w1 = pk[1], w2 = pk[2], w3 = pk[3];
        asm volatile("" : "+v"(w0), "+v"(w1), "+v"(w2), "+v"(w3));
#pragma unroll
        for (int s = 0; s < NP; ++s) {
          const unsigned e = ((s >> 2) == 0 ? w0 : (s >> 2) == 1 ? w1 : (s >> 2) == 2 ? w2 : w3) >> (8 * (s & 3));
          acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(base[(e & 15u) * 32], base[((e >> 4) & 15u) * 32], acc[s], 0, 0, 0);
        }
      }
    }
    // promote: fp32 tiles -> the fp64 tiles of this partial.  (The empty asm keeps the 224 tile addresses from being computed once
    // before the run loop and held in registers: they are rebuilt here from one pointer.)
    double* pb = part + (long long)blockIdx.x * npairs * 1024 + (4 * half) * 32 + row;
    asm volatile("" : "+v"(pb));
    int live = cnt;                                    // (likewise: not fourteen comparison results kept across the run loop)
    asm volatile("" : "+s"(live));
#pragma unroll
    for (int s = 0; s < NP; ++s) {
      if (s < live) {
        double* tile = pb + (wave + 4 * s) * 1024;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          double* d = tile + ((j & 3) + 8 * (j >> 2)) * 32;
          *d += (double)acc[s][j];
        }
      }
      __builtin_amdgcn_sched_barrier(0);               // (one tile's sixteen doubles in flight at a time, not all of them)
    }
  }
}

// G[i][j] for all (i, j) of cs x cs: the partials of the upper-triangle element (min, max) in ascending order -- the mirror is exact.
__global__ void band_gram_finish_kernel(const double* __restrict__ part, int parts, int cs, double* __restrict__ gram) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= cs * cs) return;
  const int i = e / cs, j = e - i * cs;
  const int a = min(i, j), b = max(i, j), nb = (cs + 31) >> 5;
  const int npairs = nb * (nb + 1) / 2;
  const long long off = (long long)gram_pair_index(nb, a >> 5, b >> 5) * 1024 + (a & 31) * 32 + (b & 31);
  double g = 0.;
  for (int p = 0; p < parts; ++p) g += part[(long long)p * npairs * 1024 + off];
  gram[e] = g;
}

// ---- projection ------------------------------------------------------------------------------------------------------
// The batch-tile pipeline of band_common.h with nothing added: W and the bias as the score rows (band_stage_rows), PROJ_TILE pixel
// rows per tile (band_tile_load, band_tile_stage: the next tile's rows travel global -> registers before the current tile is
// multiplied), each wave 16 pixels of the tile against every block of output channels (band_scores).  A lane ends with four
// consecutive output channels of one pixel: one 16-byte store.
template <int NKB>
__global__ __launch_bounds__(BAND_THREADS) void band_project_kernel(const float* __restrict__ x, long long P, int q,
                                                                    const float* __restrict__ W, const float* __restrict__ bias,
                                                                    int ks, float* __restrict__ y) {
  extern __shared__ float pl[];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int cs = 4 * q, kp = band_kp(NKB), ldx = band_tile_stride(cs);
  float* wl = pl;                                      // [cs][kp]
  float* xl = pl + cs * kp;                            // [PROJ_TILE][ldx]
  const int col = lane & 15, kq = lane >> 4;
  BandRows<NKB> rows;
  band_stage_rows<NKB>(wl, W, bias, cs, ks, t, col, kq, rows);
  const long long tiles = (P + PROJ_TILE - 1) / PROJ_TILE;
  f32x4 v[PROJ_LOADS];
  auto load = [&](long long tile) {
    const long long p0 = tile * PROJ_TILE;             // (left: the quads of the tile that lie inside the batch)
    band_tile_load<PROJ_LOADS, BAND_THREADS>(v, x + p0 * cs, t, (int)min((long long)PROJ_TILE, P - p0) * q);
  };
  if (blockIdx.x < tiles) load(blockIdx.x);
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    __syncthreads();
    band_tile_stage<PROJ_LOADS, BAND_THREADS>(xl, v, t, PROJ_TILE * q, q, ldx, BandQuadAsIs());
    __syncthreads();
    if (tile + gridDim.x < tiles) load(tile + gridDim.x);
    f32x4 acc[NKB], accd;
    band_scores<NKB, false>(xl + (wave * 16 + col) * ldx + kq, wl + kq * kp, rows, cs, acc, accd);
    const long long pix = tile * PROJ_TILE + wave * 16 + col;
    if (pix < P) {
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb) {
        const int n0 = kb * 16 + kq * 4;
        if (n0 < ks) *reinterpret_cast<f32x4*>(y + pix * ks + n0) = acc[kb];
      }
    }
  }
}

// ---- affine: y = fmaf(x, s, t) on the bands, zeros above; one channel quad per thread, 16 bytes both ways -----------------------
__global__ void band_affine_kernel(const float* __restrict__ x, long long quads, int q, int C, const float* __restrict__ s,
                                   const float* __restrict__ tt, float* __restrict__ y) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < quads; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % q) * 4;
    const f32x4 v = *reinterpret_cast<const f32x4*>(x + 4 * i);
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = c + j < C ? fmaf(v[j], s[c + j], tt[c + j]) : 0.f;
    *reinterpret_cast<f32x4*>(y + 4 * i) = o;
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------
static inline size_t band_moment_bytes(int cs) { return (size_t)BAND_MOMENT_PARTS * (2 * (size_t)cs + 1) * 8; }
static inline size_t band_gram_bytes(int cs) {
  const size_t nb = ((size_t)cs + 31) / 32;
  return (size_t)BAND_GRAM_PARTS * (nb * (nb + 1) / 2) * 1024 * 8;
}
static inline size_t band_project_lds(int cs, int ks) {
  return ((size_t)cs * band_kp((ks + 15) / 16) + (size_t)PROJ_TILE * band_tile_stride(cs)) * 4;
}

extern "C" int hpri_band_fp32_run(void) { return BAND_FP32_RUN; }
extern "C" int hpri_band_max_cs(void) { return BAND_MAX_CS; }
extern "C" int hpri_band_project_max_k(void) { return PROJ_MAX_K; }

// 0 for a channel stride the family does not take
extern "C" size_t hpri_band_workspace_bytes(int cs) {
  if (!band_cs_ok(cs)) return 0;
  const size_t a = band_moment_bytes(cs), b = band_gram_bytes(cs);
  return a > b ? a : b;
}

extern "C" int hpri_band_moments(const void* cache, int cache_dtype, int slots, int Hs, int Ws, int cs, const unsigned char* masks,
                                 const int* slot_table, int n, int select, const float* pivot, void* workspace, size_t workspace_bytes,
                                 long long* count, double* sums, double* sumsq, hipStream_t stream) {
  const BandPass p = {"band_moments", cache, cache_dtype, slots, Hs, Ws, cs, masks, slot_table, n, select};
  CACHE_REQUIRE(p.who, count && sums, "null pointer");
  if (int e = band_check(p, workspace, workspace_bytes, hpri_band_workspace_bytes(cs))) return e;
  CACHE_REQUIRE(p.who, (pivot == nullptr) == (sumsq == nullptr), "pivot and sumsq come together");
  CACHE_REQUIRE(p.who, ((uintptr_t)pivot & 15) == 0 && (((uintptr_t)count | (uintptr_t)sums | (uintptr_t)sumsq) & 7) == 0, "misaligned pointer");
  const long long P = (long long)Hs * Ws;
  const int rps = (int)((P + BAND_FP32_RUN - 1) / BAND_FP32_RUN);
  const long long runs = (long long)n * rps;
  const int parts = (int)(runs < BAND_MOMENT_PARTS ? runs : BAND_MOMENT_PARTS);
  double* part_sum = (double*)workspace;
  double* part_sq = part_sum + (size_t)BAND_MOMENT_PARTS * cs;
  long long* part_cnt = (long long*)(part_sq + (size_t)BAND_MOMENT_PARTS * cs);
  double* psq = sumsq ? part_sq : nullptr;
  if (cache_dtype == 0)
    hipLaunchKernelGGL(band_moments_kernel<float>, dim3(parts), dim3(BAND_THREADS), 0, stream, (const float*)cache, masks, slot_table, slots,
                       P, cs / 4, rps, runs, select, pivot, part_sum, psq, part_cnt);
  else
    hipLaunchKernelGGL(band_moments_kernel<_Float16>, dim3(parts), dim3(BAND_THREADS), 0, stream, (const _Float16*)cache, masks, slot_table,
                       slots, P, cs / 4, rps, runs, select, pivot, part_sum, psq, part_cnt);
  HPRI_CHECK_LAUNCH();
  hipLaunchKernelGGL(band_moments_finish_kernel, dim3((cs + 63) / 64), dim3(64), 0, stream, part_sum, psq, part_cnt, parts, cs, count, sums,
                     sumsq);
  HPRI_CHECK_LAUNCH();
  return HPRI_OK;
}

extern "C" int hpri_band_gram(const void* cache, int cache_dtype, int slots, int Hs, int Ws, int cs, const unsigned char* masks,
                              const int* slot_table, int n, int select, const float* pivot, void* workspace, size_t workspace_bytes,
                              double* gram, hipStream_t stream) {
  const BandPass p = {"band_gram", cache, cache_dtype, slots, Hs, Ws, cs, masks, slot_table, n, select};
  CACHE_REQUIRE(p.who, pivot && gram, "null pointer");
  if (int e = band_check(p, workspace, workspace_bytes, hpri_band_workspace_bytes(cs))) return e;
  CACHE_REQUIRE(p.who, ((uintptr_t)pivot & 15) == 0 && ((uintptr_t)gram & 7) == 0, "misaligned pointer");
  const long long P = (long long)Hs * Ws;
  const int rps = (int)((P + BAND_FP32_RUN - 1) / BAND_FP32_RUN);
  const long long runs = (long long)n * rps;
  const int parts = (int)(runs < BAND_GRAM_PARTS ? runs : BAND_GRAM_PARTS);
  const int nb = (cs + 31) / 32;
  const size_t lds = ((size_t)GRAM_CHUNK * nb * 32 + cs) * 4;
  const int need = (nb * (nb + 1) / 2 + 3) / 4;        // block pairs per wave
#define BAND_GRAM_LAUNCH(NP_)                                                                                                      \
  do {                                                                                                                             \
    if (cache_dtype == 0)                                                                                                          \
      hipLaunchKernelGGL((band_gram_kernel<float, NP_>), dim3(parts), dim3(BAND_THREADS), lds, stream, (const float*)cache, masks,   \
                         slot_table, slots, P, cs / 4, rps, runs, select, pivot, (double*)workspace);                              \
    else                                                                                                                           \
      hipLaunchKernelGGL((band_gram_kernel<_Float16, NP_>), dim3(parts), dim3(BAND_THREADS), lds, stream, (const _Float16*)cache,   \
                         masks, slot_table, slots, P, cs / 4, rps, runs, select, pivot, (double*)workspace);                       \
  } while (0)
  if (need <= 1) BAND_GRAM_LAUNCH(1);
  else if (need <= 2) BAND_GRAM_LAUNCH(2);
  else if (need <= 4) BAND_GRAM_LAUNCH(4);
  else if (need <= 7) BAND_GRAM_LAUNCH(7);
  else if (need <= 9) BAND_GRAM_LAUNCH(9);
  else BAND_GRAM_LAUNCH(GRAM_MAXP);
#undef BAND_GRAM_LAUNCH
  HPRI_CHECK_LAUNCH();
  hipLaunchKernelGGL(band_gram_finish_kernel, dim3((cs * cs + 255) / 256), dim3(256), 0, stream, (const double*)workspace, parts, cs, gram);
  HPRI_CHECK_LAUNCH();
  return HPRI_OK;
}

extern "C" int hpri_band_project(const float* x, long long pixels, int cs, const float* weight, const float* bias, int K, float* y,
                                 hipStream_t stream) {
  HPRI_REQUIRE(x && weight && bias && y, "band_project: null pointer");
  HPRI_REQUIRE(pixels > 0 && K > 0, "band_project: bad sizes");
  HPRI_REQUIRE(band_cs_ok(cs), "band_project: the channel stride must be a multiple of 8 up to hpri_band_max_cs");
  HPRI_REQUIRE(K <= PROJ_MAX_K, "band_project: K exceeds hpri_band_project_max_k");
  const int ks = (K + 7) & ~7;
  const size_t lds = band_project_lds(cs, ks);
  HPRI_REQUIRE(lds <= BAND_LDS_BYTES, "band_project: weights and a tile of this cs and K do not fit the LDS");
  HPRI_REQUIRE(hpri_aligned16(x, weight, bias, y), "band_project: buffers must be 16-byte aligned");
  const long long tiles = (pixels + PROJ_TILE - 1) / PROJ_TILE;
  const long long per_cu = BAND_LDS_BYTES / (long long)lds;
  const dim3 grid = cache_grid(tiles, (int)(per_cu < 1 ? 1 : per_cu > 4 ? 4 : per_cu));
#define BAND_PROJECT_LAUNCH(NKB_)                                                                                                  \
  do {                                                                                                                             \
    hpri_ask_dynamic_lds(band_project_kernel<NKB_>, lds);                                                                          \
    hipLaunchKernelGGL(band_project_kernel<NKB_>, grid, dim3(BAND_THREADS), lds, stream, x, pixels, cs / 4, weight, bias, ks, y);  \
  } while (0)
  switch ((ks + 15) / 16) {                            // blocks of 16 output channels
    case 1: BAND_PROJECT_LAUNCH(1); break;
    case 2: BAND_PROJECT_LAUNCH(2); break;
    case 3: BAND_PROJECT_LAUNCH(3); break;
    default: BAND_PROJECT_LAUNCH(4); break;
  }
#undef BAND_PROJECT_LAUNCH
  HPRI_CHECK_LAUNCH();
  return HPRI_OK;
}

extern "C" int hpri_band_affine(const float* x, long long pixels, int cs, int C, const float* scale, const float* shift, float* y,
                                hipStream_t stream) {
  HPRI_REQUIRE(x && scale && shift && y, "band_affine: null pointer");
  HPRI_REQUIRE(pixels > 0, "band_affine: bad sizes");
  HPRI_REQUIRE(cs > 0 && cs % 8 == 0 && C > 0 && C <= cs, "band_affine: the channel stride must be a multiple of 8 that holds the bands");
  HPRI_REQUIRE(hpri_aligned16(x, y), "band_affine: buffers must be 16-byte aligned");
  const long long quads = pixels * (cs / 4);
  hipLaunchKernelGGL(band_affine_kernel, cache_grid((quads + 255) / 256, 8), dim3(256), 0, stream, x, quads, cs / 4, C, scale, shift, y);
  HPRI_CHECK_LAUNCH();
  return HPRI_OK;
}
