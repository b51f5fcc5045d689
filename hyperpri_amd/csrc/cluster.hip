// Spectral k-means (hyperpri_amd/cluster.py): the argmin of K affine scores of a centred pixel, for a batch (assign) and as the
// fitting pass over the cube cache's slots (cluster sums).
//
//   d[c]  = fp32(x[c] - pivot[c])                                              (x itself without a pivot)
//   z[k]  = fmaf(W[k][cs-1], d[cs-1], ... fmaf(W[k][0], d[0], b[k]))           k < K: bitwise the chain of hpri_band_project
//   label = the lowest k < K with z[k] == min z,   zmin = z[label],   s = fmaf(d[c], d[c], s) from 0, ascending c
//
// For a centroid g the caller passes W[k] = -g and b[k] = |g|^2 / 2: z is half the squared distance minus |d|^2 / 2, and
// max(0, 2 zmin + s) is the squared distance to the nearest centroid.  The kernels know nothing of that.
//
// Scores.  The batch-tile pipeline of band_common.h: W transposed in LDS for the workgroup's lifetime (band_stage_rows), a tile of
// CL_TILE = 64 pixels as d at a row stride of band_tile_stride(cs), each wave 16 pixels against every block of 16 rows (band_scores).
// Where W at ks = 64 and 64 pixels do not fit the LDS together (cs > 304) the tile is 32 pixels and two waves score.  s is the diagonal
// of the same product with the pixel on both sides (A == B == the register that holds d): D[i][i] of the 16 x 16 tile is the chain
// above, bit for bit.
// Argmin.  A lane holds the rows 16 kb + 4 (l >> 4) + j, j < 4, of its pixel; it scans them in ascending k (a later row wins only when
// it is strictly smaller), then the four lanes of a pixel exchange (z, k) over xor 16 and xor 32 and keep the smaller z, the lower k
// between equal z.  Rows >= K never enter.  A lane without a row starts at k = -1 and takes whatever comes: label < K for every
// input, NaN included (what a NaN pixel is labelled depends on the exchange; it is a valid index).
//
// Cluster sums.  One workgroup per partial (CL_PARTS = 256, a constant), runs as band_gram_kernel cuts them (band_run).  Per chunk of
// a run: stage d (exact zeros for a pixel that is not selected or past the run), score and label it as above -- the same functions,
// so the labels are those of hpri_band_assign -- then the update on v_mfma_f32_32x32x2_f32 with k = PIXEL: A[i][k] = (label of pixel k
// == cluster i) ? 1 : 0, B[k][j] = d[pixel k][band j].  A pixel of another cluster adds fmaf(0, d, acc) = acc, so sums[i][j] of a run is
// the fp32 chain acc = fmaf(1, d[p][j], acc) over the run's pixels p in ASCENDING order, from 0: fixed by the run alone.  The (cluster
// block, band block) tiles are dealt to the four waves (tile t to wave t % 4).  After the run the fp32 tiles are added into the fp64
// tiles of the workgroup's partial (L2-resident), partial a owning the runs a, a + CL_PARTS, ... in that order.  zmin and s of a
// selected pixel are added in fp64 at once by the lane that owns pixel slot (wave, column) of every chunk; at the end of the kernel
// one thread adds the 64 lane sums in ascending slot order.  Counts: 64-bit integer atomics in LDS, then the partial scheme.  A
// finishing kernel adds the partials 0, 1, 2, ... .  No floating-point atomic anywhere.
#include "band_common.h"

#define CL_MAX_K 64
#define CL_TILE 64
#define CL_PARTS 256
#define CL_LOADS ((CL_TILE * (BAND_MAX_CS / 4) + BAND_THREADS - 1) / BAND_THREADS)

// LDS of either kernel, in words: wl [cs][kp], xl [tile][ldx], the pivot [cs], the labels [CL_TILE], then 64 counters and 2 x 64
// doubles of 8 bytes
static inline size_t cl_lds_bytes(int cs, int ks, int tile) {
  const int kp = band_kp((ks + 15) / 16);
  return ((size_t)cs * kp + (size_t)tile * band_tile_stride(cs) + cs + CL_TILE) * 4 + (size_t)CL_MAX_K * 8 + 2 * (size_t)CL_TILE * 8;
}
static inline int cl_tile(int cs, int ks) { return cl_lds_bytes(cs, ks, CL_TILE) <= BAND_LDS_BYTES ? CL_TILE : CL_TILE / 2; }

// the label and its score, in every lane of the pixel (see the head of the file)
template <int NKB>
__device__ __forceinline__ void cl_argmin(const f32x4 (&acc)[NKB], int K, int kq, int& label, float& zmin) {
  int bk = -1;
  float bz = 0.f;
#pragma unroll
  for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = kb * 16 + kq * 4 + j;
      const float z = acc[kb][j];
      const bool take = k < K && (bk < 0 || z < bz);
      bk = take ? k : bk;
      bz = take ? z : bz;
    }
#pragma unroll
  for (int o = 16; o <= 32; o <<= 1) {
    const int ok = __shfl_xor(bk, o);
    const float oz = __shfl_xor(bz, o);
    const bool take = ok >= 0 && (bk < 0 || oz < bz || (oz == bz && ok < bk));
    bk = take ? ok : bk;
    bz = take ? oz : bz;
  }
  label = bk;
  zmin = bz;
}

// s of pixel column col, in the lanes of that column: D[col][col] sits in lane col + 16 (col >> 2), register col & 3
__device__ __forceinline__ float cl_diagonal(const f32x4& accd, int col) {
  const int j = col & 3;
  const float mine = j == 0 ? accd[0] : j == 1 ? accd[1] : j == 2 ? accd[2] : accd[3];
  return __shfl(mine, col + 16 * (col >> 2));
}

// ---- assign ----------------------------------------------------------------------------------------------------------
template <int NKB, bool DIAG>
__global__ __launch_bounds__(BAND_THREADS) void band_assign_kernel(const float* __restrict__ x, long long P, int q,
                                                                   const float* __restrict__ pivot, const float* __restrict__ W,
                                                                   const float* __restrict__ bias, int ks, int K, int tile,
                                                                   const float* __restrict__ lut, unsigned char* __restrict__ labels,
                                                                   float* __restrict__ zout, float* __restrict__ dist2,
                                                                   float* __restrict__ value) {
  extern __shared__ float cl[];
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int cs = 4 * q, kp = band_kp(NKB), ldx = band_tile_stride(cs);
  float* wl = cl;                                      // [cs][kp]
  float* xl = wl + cs * kp;                            // [tile][ldx]
  float* pvl = xl + tile * ldx;                        // [cs]
  const int col = lane & 15, kq = lane >> 4;
  BandRows<NKB> rows;
  band_stage_rows<NKB>(wl, W, bias, cs, ks, t, col, kq, rows);
  for (int i = t; i < cs; i += BAND_THREADS) pvl[i] = pivot != nullptr ? pivot[i] : 0.f;
  const long long tiles = (P + tile - 1) / tile;
  f32x4 v[CL_LOADS];
  // (q is hidden from the optimiser per tile, as band_gram_kernel hides it: the quotients idx / q and the addresses made of them would
  // otherwise be computed once and held in registers across the k loop)
  int ql = q;
  auto load = [&](long long tl) {
    const long long p0 = tl * tile;
    const int left = (int)min((long long)tile, P - p0) * ql;       // quads of the tile that lie inside the batch
    // (band_tile_load with its 64-bit addresses: on 32-bit offsets from the tile's first quad the label map at K = 2 and 8 measured
    // 2 % slower, profiles/band_pipeline_refactor.json)
#pragma unroll
    for (int u = 0; u < CL_LOADS; ++u) {
      const int idx = t + u * BAND_THREADS;
      v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (idx < left) v[u] = *reinterpret_cast<const f32x4*>(x + p0 * cs + 4LL * idx);
    }
  };
  const auto centre = [pvl](f32x4 w, int cq) { return w - *reinterpret_cast<const f32x4*>(pvl + 4 * cq); };
  if (blockIdx.x < tiles) load(blockIdx.x);
  for (long long tl = blockIdx.x; tl < tiles; tl += gridDim.x) {
    __syncthreads();                                   // (the rows and the pivot are in LDS; the previous tile has been consumed)
    asm volatile("" : "+s"(ql));
    band_tile_stage<CL_LOADS, BAND_THREADS>(xl, v, t, tile * q, ql, ldx, centre);
    __syncthreads();
    if (tl + gridDim.x < tiles) load(tl + gridDim.x);
    if (wave * 16 < tile) {
      f32x4 acc[NKB], accd;
      band_scores<NKB, DIAG>(xl + (wave * 16 + col) * ldx + kq, wl + kq * kp, rows, cs, acc, accd);
      int label;
      float zmin;
      cl_argmin<NKB>(acc, K, kq, label, zmin);
      const float s = DIAG ? cl_diagonal(accd, col) : 0.f;
      const long long pix = tl * tile + wave * 16 + col;
      if (kq == 0 && pix < P) {
        if (labels != nullptr) labels[pix] = (unsigned char)label;
        if (zout != nullptr) zout[pix] = zmin;
        if (DIAG) dist2[pix] = fmaxf(0.f, fmaf(2.f, zmin, s));
        if (value != nullptr) value[pix] = lut[label];
      }
    }
  }
}

// ---- cluster sums ----------------------------------------------------------------------------------------------------
// NKB blocks of 16 score rows are KB32 = ceil(NKB / 2) blocks of 32 clusters; with up to ten band blocks that is at most NT tiles a wave
template <typename T, int NKB>
__global__ __launch_bounds__(BAND_THREADS) void band_cluster_kernel(const T* __restrict__ cache, const unsigned char* __restrict__ masks,
                                                                    const int* __restrict__ table, int slots, long long P, int q,
                                                                    int runs_per_slot, long long runs, int select,
                                                                    const float* __restrict__ pivot, const float* __restrict__ W,
                                                                    const float* __restrict__ bias, int ks, int K, int tile,
                                                                    double* __restrict__ part, unsigned long long* __restrict__ part_cnt,
                                                                    double* __restrict__ part_tot) {
  constexpr int KB32 = (NKB + 1) / 2, NT = (KB32 * (BAND_MAX_CS / 32) + 3) / 4;
  extern __shared__ float cl[];
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int cs = 4 * q, kp = band_kp(NKB), ldx = band_tile_stride(cs), nb = (cs + 31) >> 5;
  const int ntiles = ((K + 31) >> 5) * nb;
  float* wl = cl;                                      // [cs][kp]
  float* xl = wl + cs * kp;                            // [tile][ldx]
  float* pvl = xl + tile * ldx;                        // [cs]
  int* lab = reinterpret_cast<int*>(pvl + cs);         // [CL_TILE]: the label of a staged pixel, -1: it does not count
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(lab + CL_TILE);       // [CL_MAX_K]
  double* tot = reinterpret_cast<double*>(cnt + CL_MAX_K);                              // [2][CL_TILE]
  const int col = lane & 15, kq = lane >> 4;
  BandRows<NKB> rows;
  band_stage_rows<NKB>(wl, W, bias, cs, ks, t, col, kq, rows);
  for (int i = t; i < cs; i += BAND_THREADS) pvl[i] = pivot != nullptr ? pivot[i] : 0.f;
  for (int i = t; i < tile * ldx; i += BAND_THREADS) xl[i] = 0.f;          // (the columns [cs, ldx) stay zero)
  if (t < CL_MAX_K) cnt[t] = 0ull;
  // this wave's tiles t = wave, wave + 4, ...: 32 x (cluster block, band block); a slot beyond them repeats tile 0 and is never used
  int boff[NT], cbase[NT];
#pragma unroll
  for (int s = 0; s < NT; ++s) {
    const int ti = wave + 4 * s;
    const int cb = ti < ntiles ? ti / nb : 0, bb = ti < ntiles ? ti - cb * nb : 0;
    boff[s] = 32 * bb;
    cbase[s] = 32 * cb;
  }
  const int live = (ntiles - wave + 3) >> 2;           // tiles of this wave
  const int row = lane & 31, half = lane >> 5;
  const long long pstride = (long long)ntiles * 1024;
  // the workgroup's partial starts from zero (the barriers of the first chunk order these stores before the first promotion)
  for (int i = t; i < ntiles * 1024; i += BAND_THREADS) part[(long long)blockIdx.x * pstride + i] = 0.;
  double az = 0., as = 0.;
  const int total = tile * q;
  const int px0 = t / q, cq0 = t - px0 * q, dq = BAND_THREADS / q, dr = BAND_THREADS - dq * q;
  for (long long r = blockIdx.x; r < runs; r += CL_PARTS) {
    const BandRun run = band_run(table, slots, P, runs_per_slot, r);
    f32x16 acc[NT];
#pragma unroll
    for (int s = 0; s < NT; ++s)
#pragma unroll
      for (int j = 0; j < 16; ++j) acc[s][j] = 0.f;
    // a chunk's quads as loaded (widened, pivoted and selected when they are stored into LDS, one chunk later) and their pixel's mask
    // byte (-1: past the run)
    decltype(band_raw(cache)) v[CL_LOADS];
    int keep[CL_LOADS];
    // quad t + 256 u of a chunk is (pixel, channel quad) = (px0, cq0) + u (dq, dr) with a carry: no division per quad.  (The start is
    // hidden from the optimiser per chunk, as band_gram_kernel hides q: the pairs would otherwise be computed once, held in
    // registers for the kernel's lifetime and spilled beside the accumulator tiles.)
    auto load = [&](int c0, int px, int cq) {
#pragma unroll
      for (int u = 0; u < CL_LOADS; ++u) {
        const int idx = t + u * BAND_THREADS;
        keep[u] = -1;
        if (idx < total && c0 + px < run.len) {
          const long long pix = run.base + c0 + px;
          v[u] = band_raw(cache + pix * cs + 4 * cq);
          keep[u] = select == 0 ? 1 : (int)masks[pix];
        }
        cq += dr;
        px += dq;
        if (cq >= q) { cq -= q; ++px; }
      }
    };
    int pxs = px0, cqs = cq0;
    asm volatile("" : "+v"(pxs), "+v"(cqs));
    load(0, pxs, cqs);
    for (int c0 = 0; c0 < run.len; c0 += tile) {
      __syncthreads();                                 // (the rows are in LDS; the previous chunk and its labels have been consumed)
      asm volatile("" : "+v"(pxs), "+v"(cqs));
      int px = pxs, cq = cqs;
#pragma unroll
      for (int u = 0; u < CL_LOADS; ++u, cq += dr, px += dq) {
        const int idx = t + u * BAND_THREADS;
        if (cq >= q) { cq -= q; ++px; }
        if (idx < total) {
          const bool on = keep[u] >= 0 && (select == 0 || (keep[u] != 0) == (select == 1));
          f32x4 d = {0.f, 0.f, 0.f, 0.f};
          if (on) d = band_widen(v[u]) - *reinterpret_cast<const f32x4*>(pvl + 4 * cq);
          float2* dst = reinterpret_cast<float2*>(xl + px * ldx + 4 * cq);
          dst[0] = float2{d[0], d[1]};
          dst[1] = float2{d[2], d[3]};
          if (cq == 0) lab[px] = on ? 0 : -1;
        }
      }
      __syncthreads();
      if (c0 + tile < run.len) load(c0 + tile, pxs, cqs);
      if (wave * 16 < tile) {
        f32x4 sc[NKB], accd;
        band_scores<NKB, true>(xl + (wave * 16 + col) * ldx + kq, wl + kq * kp, rows, cs, sc, accd);
        int label;
        float zmin;
        cl_argmin<NKB>(sc, K, kq, label, zmin);
        const float s = cl_diagonal(accd, col);
        const int px = wave * 16 + col;
        if (kq == 0 && lab[px] >= 0) {
          lab[px] = label;
          az += (double)zmin;
          as += (double)s;
          atomicAdd(&cnt[label], 1ull);
        }
      }
      __syncthreads();
      // two pixels a step, ascending: the one-hot column of the pixel against its staged d
      // (the operands of the next step are read from LDS before this step's MFMAs issue; the last step reads its own again)
      const float* base = xl + half * ldx + row;
      int l = lab[half] - row;
      float b[NT];
#pragma unroll
      for (int s = 0; s < NT; ++s) b[s] = base[boff[s]];
      for (int k = 0; k < tile; k += 2) {
        const int kn = min(k + 2, tile - 2);
        const int nl = lab[kn + half] - row;
        float nb[NT];
#pragma unroll
        for (int s = 0; s < NT; ++s) nb[s] = base[kn * ldx + boff[s]];
#pragma unroll
        for (int s = 0; s < NT; ++s)
          if (s < live) acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(l == cbase[s] ? 1.f : 0.f, b[s], acc[s], 0, 0, 0);
        l = nl;
#pragma unroll
        for (int s = 0; s < NT; ++s) b[s] = nb[s];
      }
    }
    // promote: fp32 tiles -> the fp64 tiles of this partial; D: column (band) = l & 31, row (cluster) = (reg & 3) + 8 (reg >> 2) + 4 (l >> 5)
    // (the empty asm keeps the tile addresses from being computed once before the run loop and held in registers)
    double* pb = part + (long long)blockIdx.x * pstride + (4 * half) * 32 + row;
    asm volatile("" : "+v"(pb));
    int lv = live;
    asm volatile("" : "+s"(lv));
#pragma unroll
    for (int s = 0; s < NT; ++s) {
      if (s < lv) {
        double* tp = pb + (long long)(wave + 4 * s) * 1024;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          double* d = tp + ((j & 3) + 8 * (j >> 2)) * 32;
          *d += (double)acc[s][j];
        }
      }
      __builtin_amdgcn_sched_barrier(0);               // (one tile's sixteen doubles in flight at a time, not all of them)
    }
  }
  // the lane sums of pixel slot (wave, col), added in ascending slot order by one thread; the counts
  __syncthreads();
  if (kq == 0) {
    tot[wave * 16 + col] = az;
    tot[CL_TILE + wave * 16 + col] = as;
  }
  __syncthreads();
  if (t < 2) {
    double a = 0.;
    for (int i = 0; i < CL_TILE; ++i) a += tot[t * CL_TILE + i];
    part_tot[2 * blockIdx.x + t] = a;
  }
  if (t < CL_MAX_K) part_cnt[(long long)blockIdx.x * CL_MAX_K + t] = cnt[t];
}

// sums[k][c], counts[k] and the totals: the partials in ascending order
__global__ void band_cluster_finish_kernel(const double* __restrict__ part, const unsigned long long* __restrict__ part_cnt,
                                           const double* __restrict__ part_tot, int parts, int cs, int K, long long* __restrict__ counts,
                                           double* __restrict__ sums, double* __restrict__ totals) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  const int nb = (cs + 31) >> 5;
  const long long pstride = (long long)((K + 31) >> 5) * nb * 1024;
  if (e < K * cs) {
    const int k = e / cs, c = e - k * cs;
    const long long off = (long long)((k >> 5) * nb + (c >> 5)) * 1024 + (k & 31) * 32 + (c & 31);
    double a = 0.;
    for (int p = 0; p < parts; ++p) a += part[(long long)p * pstride + off];
    sums[e] = a;
  }
  if (e < K) {
    unsigned long long n = 0ull;
    for (int p = 0; p < parts; ++p) n += part_cnt[(long long)p * CL_MAX_K + e];
    counts[e] = (long long)n;
  }
  if (e < 2) {
    double a = 0.;
    for (int p = 0; p < parts; ++p) a += part_tot[2 * p + e];
    totals[e] = a;
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------
extern "C" int hpri_band_cluster_max_k(void) { return CL_MAX_K; }
extern "C" int hpri_band_cluster_parts(void) { return CL_PARTS; }

static inline size_t cl_part_doubles(int cs, int K) { return (size_t)((K + 31) / 32) * (((size_t)cs + 31) / 32) * 1024; }

// 0 for a channel stride or a K the pass does not take
extern "C" size_t hpri_band_cluster_workspace_bytes(int cs, int K) {
  if (!band_cs_ok(cs) || K <= 0 || K > CL_MAX_K) return 0;
  return (size_t)CL_PARTS * (cl_part_doubles(cs, K) + CL_MAX_K + 2) * 8;
}

extern "C" int hpri_band_assign(const float* x, long long pixels, int cs, const float* pivot, const float* centers, const float* bias,
                                int K, const float* lut, unsigned char* labels, float* zmin, float* dist2, float* value,
                                hipStream_t stream) {
  HPRI_REQUIRE(x && centers && bias, "band_assign: null pointer");
  HPRI_REQUIRE(pixels > 0, "band_assign: bad sizes");
  HPRI_REQUIRE(band_cs_ok(cs), "band_assign: the channel stride must be a multiple of 8 up to hpri_band_max_cs");
  HPRI_REQUIRE(K > 0 && K <= CL_MAX_K, "band_assign: K must lie in [1, hpri_band_cluster_max_k]");
  HPRI_REQUIRE(labels || zmin || dist2 || value, "band_assign: nothing to write");
  HPRI_REQUIRE((value != nullptr) == (lut != nullptr), "band_assign: value and lut come together");
  HPRI_REQUIRE(hpri_aligned16(x, pivot, centers, bias) && (((uintptr_t)lut | (uintptr_t)zmin | (uintptr_t)dist2 | (uintptr_t)value) & 3) == 0,
               "band_assign: misaligned pointer");
  const int ks = (K + 7) & ~7, tile = cl_tile(cs, ks);
  const size_t lds = cl_lds_bytes(cs, ks, tile);
  const long long tiles = (pixels + tile - 1) / tile;
  const long long per_cu = BAND_LDS_BYTES / (long long)lds;
  const dim3 grid = cache_grid(tiles, (int)(per_cu < 1 ? 1 : per_cu > 4 ? 4 : per_cu));
#define CL_ASSIGN_LAUNCH(NKB_, DIAG_)                                                                                              \
  do {                                                                                                                             \
    hpri_ask_dynamic_lds(band_assign_kernel<NKB_, DIAG_>, lds);                                                                    \
    hipLaunchKernelGGL((band_assign_kernel<NKB_, DIAG_>), grid, dim3(BAND_THREADS), lds, stream, x, pixels, cs / 4, pivot, centers, bias, \
                       ks, K, tile, lut, labels, zmin, dist2, value);                                                              \
  } while (0)
#define CL_ASSIGN_DIAG(NKB_)                                                                                                       \
  do {                                                                                                                             \
    if (dist2 != nullptr) CL_ASSIGN_LAUNCH(NKB_, true);                                                                            \
    else CL_ASSIGN_LAUNCH(NKB_, false);                                                                                            \
  } while (0)
  switch ((ks + 15) / 16) {                            // blocks of 16 score rows
    case 1: CL_ASSIGN_DIAG(1); break;
    case 2: CL_ASSIGN_DIAG(2); break;
    case 3: CL_ASSIGN_DIAG(3); break;
    default: CL_ASSIGN_DIAG(4); break;
  }
#undef CL_ASSIGN_DIAG
#undef CL_ASSIGN_LAUNCH
  HPRI_CHECK_LAUNCH();
  return HPRI_OK;
}

extern "C" int hpri_band_cluster_sums(const void* cache, int cache_dtype, int slots, int Hs, int Ws, int cs, const unsigned char* masks,
                                      const int* slot_table, int n, int select, const float* pivot, const float* centers,
                                      const float* bias, int K, void* workspace, size_t workspace_bytes, long long* counts, double* sums,
                                      double* totals, hipStream_t stream) {
  const BandPass p = {"band_cluster_sums", cache, cache_dtype, slots, Hs, Ws, cs, masks, slot_table, n, select};
  CACHE_REQUIRE(p.who, centers && bias && counts && sums && totals, "null pointer");
  if (int e = band_check(p, workspace, 0, 0)) return e;
  CACHE_REQUIRE(p.who, K > 0 && K <= CL_MAX_K, "K must lie in [1, hpri_band_cluster_max_k]");
  CACHE_REQUIRE(p.who, workspace_bytes >= hpri_band_cluster_workspace_bytes(cs, K), "the workspace is smaller than hpri_band_cluster_workspace_bytes");
  CACHE_REQUIRE(p.who, hpri_aligned16(pivot, centers, bias) && (((uintptr_t)counts | (uintptr_t)sums | (uintptr_t)totals) & 7) == 0,
                "misaligned pointer");
  const long long P = (long long)Hs * Ws;
  const int rps = (int)((P + BAND_FP32_RUN - 1) / BAND_FP32_RUN);
  const long long runs = (long long)n * rps;
  const int parts = (int)(runs < CL_PARTS ? runs : CL_PARTS);
  const int ks = (K + 7) & ~7, tile = cl_tile(cs, ks);
  const size_t lds = cl_lds_bytes(cs, ks, tile);
  double* part = (double*)workspace;
  unsigned long long* part_cnt = (unsigned long long*)(part + (size_t)CL_PARTS * cl_part_doubles(cs, K));
  double* part_tot = (double*)(part_cnt + (size_t)CL_PARTS * CL_MAX_K);
#define CL_SUMS_LAUNCH(NKB_)                                                                                                       \
  do {                                                                                                                             \
    if (cache_dtype == 0) {                                                                                                        \
      hpri_ask_dynamic_lds(band_cluster_kernel<float, NKB_>, lds);                                                                 \
      hipLaunchKernelGGL((band_cluster_kernel<float, NKB_>), dim3(parts), dim3(BAND_THREADS), lds, stream, (const float*)cache, masks, \
                         slot_table, slots, P, cs / 4, rps, runs, select, pivot, centers, bias, ks, K, tile, part, part_cnt, part_tot); \
    } else {                                                                                                                       \
      hpri_ask_dynamic_lds(band_cluster_kernel<_Float16, NKB_>, lds);                                                              \
      hipLaunchKernelGGL((band_cluster_kernel<_Float16, NKB_>), dim3(parts), dim3(BAND_THREADS), lds, stream, (const _Float16*)cache, \
                         masks, slot_table, slots, P, cs / 4, rps, runs, select, pivot, centers, bias, ks, K, tile, part, part_cnt,  \
                         part_tot);                                                                                                \
    }                                                                                                                              \
  } while (0)
  switch ((ks + 15) / 16) {
    case 1: CL_SUMS_LAUNCH(1); break;
    case 2: CL_SUMS_LAUNCH(2); break;
    case 3: CL_SUMS_LAUNCH(3); break;
    default: CL_SUMS_LAUNCH(4); break;
  }
#undef CL_SUMS_LAUNCH
  HPRI_CHECK_LAUNCH();
  const int items = K * cs;
  hipLaunchKernelGGL(band_cluster_finish_kernel, dim3((items + 255) / 256), dim3(256), 0, stream, (const double*)part,
                     (const unsigned long long*)part_cnt, (const double*)part_tot, parts, cs, K, counts, sums, totals);
  HPRI_CHECK_LAUNCH();
  return HPRI_OK;
}
