// Spectral Gaussian mixtures (hyperpri_amd/mixture.py): K full-covariance Gaussians in a shared q-dimensional projection of a centred
// pixel, scored for a batch (gmm score) and as the E-step with the M-step's sums over the cube cache's slots (gmm sums).  The contract
// (z, u_k, m_k, l_k, L_c, r_k and the summation rule) is stated in include/hyperpri_hip.h.
//
// Score.  Stage 1 is the batch-tile pipeline of band_common.h with NKB blocks of 16 rows (one for q <= 16, else two): W transposed in
// LDS for the workgroup's lifetime, a tile of 64 pixels as d (32 where the LDS does not hold 64), each wave 16 pixels.  z of the tile
// goes to LDS.  Stage 2 is the same chain again (band_scores) per component, looped: the "bands" are the qp entries of z, the rows
// those of A_k, which sits transposed in LDS as W does, the bias is a_k.  The four lanes of a pixel add the squares of their u.
//
// Sums.  One workgroup per partial, runs as band_gram_kernel cuts them.  Per chunk of a run: stage d (zeros for a pixel that does not
// count), z, l_k, r_k by the functions of the score pass, r_k to LDS, then the update on v_mfma_f32_32x32x2_f32 with k = PIXEL over
// X = (e[0], ..., e[q-1], 1): A[i][p] = fp32(r_k X[i]), B[p][j] = X[j], so Q_k = D[i][j], S_k = D[i][q], N_k = D[q][q].  At q = 32 X has
// 33 entries: a second tile, A = (r, r e[0], ..., r e[30]) against B = (1, e[31], 0, ...), holds N_k = D[0][0], S_k[i] = D[i+1][0] and
// S_k[31] = D[0][1].  Component k belongs to wave k % 4.  After the run the fp32 tiles are added into the fp64 tiles of the workgroup's
// partial; L_all and the count go into the lane that owns the pixel's slot, as zmin does in cluster.hip.
#include "band_common.h"

#define GM_MAX_K 8
#define GM_MAX_Q 32
#define GM_TILE 64
#define GM_PARTS 256
#define GM_LOADS ((GM_TILE * (BAND_MAX_CS / 4) + BAND_THREADS - 1) / BAND_THREADS)
#define GM_ZS 34                        // band_tile_stride(32): the row stride of z in LDS
#define GM_KP 32                        // band_kp(1) == band_kp(2)

// LDS of either kernel, in words: wl [cs][32], al [K][qp][32], a [K][32], c [8], xl [tile][ldx], the pivot [cs], z [64][GM_ZS],
// r [64][8], the selection [64], then 64 doubles and 64 counters of 8 bytes
static inline size_t gm_lds_bytes(int cs, int qp, int K, int tile) {
  return ((size_t)cs * GM_KP + (size_t)K * qp * GM_KP + (size_t)K * 32 + 8 + (size_t)tile * band_tile_stride(cs) + cs + GM_TILE * GM_ZS +
          GM_TILE * GM_MAX_K + GM_TILE) * 4 + 2 * (size_t)GM_TILE * 8;
}
static inline int gm_tile(int cs, int qp, int K) { return gm_lds_bytes(cs, qp, K, GM_TILE) <= BAND_LDS_BYTES ? GM_TILE : GM_TILE / 2; }

#ifdef __HIPCC__
struct GmLds { float *wl, *al, *abl, *ckl, *xl, *pvl, *zl, *rl; int* sel; double* tot; unsigned long long* cnt; };

__device__ __forceinline__ GmLds gm_carve(float* base, int cs, int qp, int K, int tile) {
  GmLds s;
  s.wl = base;
  s.al = s.wl + cs * GM_KP;
  s.abl = s.al + K * qp * GM_KP;
  s.ckl = s.abl + K * 32;
  s.xl = s.ckl + 8;
  s.pvl = s.xl + tile * band_tile_stride(cs);
  s.zl = s.pvl + cs;
  s.rl = s.zl + GM_TILE * GM_ZS;
  s.sel = reinterpret_cast<int*>(s.rl + GM_TILE * GM_MAX_K);
  s.tot = reinterpret_cast<double*>(s.sel + GM_TILE);
  s.cnt = reinterpret_cast<unsigned long long*>(s.tot + GM_TILE);
  return s;
}

// what a workgroup keeps in LDS for its lifetime: W (band_stage_rows; the chain of z starts from 0), A_k transposed as W is, a_k, c_k,
// the pivot; z starts as zeros (its columns from 16 NKB on stay zero)
template <int NKB>
__device__ __forceinline__ void gm_stage(const GmLds& s, const float* __restrict__ W, const float* __restrict__ pivot,
                                         const float* __restrict__ A, const float* __restrict__ a, const float* __restrict__ cst, int cs,
                                         int qp, int K, int t, int col, int kq, BandRows<NKB>& rows) {
  band_stage_rows<NKB>(s.wl, W, W, cs, qp, t, col, kq, rows);          // (the bias quads it reads are replaced by zeros below)
#pragma unroll
  for (int kb = 0; kb < NKB; ++kb) rows.b4[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int i = t; i < K * qp * GM_KP; i += BAND_THREADS) {
    const int kc = i / GM_KP, n = i - kc * GM_KP;                       // kc = k qp + c: column c of A_k
    const int k = kc / qp, c = kc - k * qp;
    s.al[kc * GM_KP + (n ^ ((c & 1) << 4))] = n < qp ? A[((long long)k * qp + n) * qp + c] : 0.f;
  }
  for (int i = t; i < K * 32; i += BAND_THREADS) {
    const int k = i >> 5, n = i & 31;
    s.abl[i] = n < qp ? a[k * qp + n] : 0.f;
  }
  if (t < 8) s.ckl[t] = t < K ? cst[t] : 0.f;
  for (int i = t; i < cs; i += BAND_THREADS) s.pvl[i] = pivot != nullptr ? pivot[i] : 0.f;
  for (int i = t; i < GM_TILE * GM_ZS; i += BAND_THREADS) s.zl[i] = 0.f;
}

// z of this lane's pixel (four consecutive rows per block of 16) -> its row in LDS
template <int NKB>
__device__ __forceinline__ void gm_store_z(float* __restrict__ zrow, const f32x4 (&acc)[NKB], int kq) {
#pragma unroll
  for (int kb = 0; kb < NKB; ++kb) {
    float2* d = reinterpret_cast<float2*>(zrow + kb * 16 + kq * 4);
    d[0] = float2{acc[kb][0], acc[kb][1]};
    d[1] = float2{acc[kb][2], acc[kb][3]};
  }
}

// l_k of this lane's pixel for every k < K, in every lane of the pixel (see the head of the file); l[k] = -inf for k >= K
template <int NKB>
__device__ __forceinline__ void gm_logdens(const GmLds& s, const float* __restrict__ zrow, const BandRows<NKB>& rows, int qp, int K, int kq,
                                           float (&l)[GM_MAX_K]) {
#pragma unroll
  for (int j = 0; j < GM_MAX_K; ++j) l[j] = -__builtin_inff();
  for (int k = 0; k < K; ++k) {
    BandRows<NKB> r2;
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
      r2.woff[kb] = rows.woff[kb];
      r2.b4[kb] = *reinterpret_cast<const f32x4*>(s.abl + k * 32 + kb * 16 + kq * 4);
    }
    f32x4 u[NKB], unused;
    band_scores<NKB, false>(zrow + kq, s.al + (k * qp + kq) * GM_KP, r2, qp, u, unused);
    float m = 0.f;
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
      for (int j = 0; j < 4; ++j) m = fmaf(u[kb][j], u[kb][j], m);
    m += __shfl_xor(m, 16);
    m += __shfl_xor(m, 32);
    const float lk = fmaf(-0.5f, m, s.ckl[k]);
#pragma unroll
    for (int j = 0; j < GM_MAX_K; ++j) l[j] = j == k ? lk : l[j];
  }
}

// L over all components and r_k = expf(l_k - mx) / sum (0 for k >= K)
__device__ __forceinline__ float gm_mix_all(const float (&l)[GM_MAX_K], int K, float (&r)[GM_MAX_K]) {
  float mx = -__builtin_inff();
#pragma unroll
  for (int k = 0; k < GM_MAX_K; ++k)
    if (k < K) mx = fmaxf(mx, l[k]);
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < GM_MAX_K; ++k) {
    r[k] = k < K ? expf(l[k] - mx) : 0.f;
    sum += r[k];
  }
#pragma unroll
  for (int k = 0; k < GM_MAX_K; ++k) r[k] = r[k] / sum;
  return mx + logf(sum);
}

// L_c of every class c < GM_MAX_K (a class without a component: -inf); cls: 4 bits per component
__device__ __forceinline__ void gm_lse_classes(const float (&l)[GM_MAX_K], int K, unsigned cls, float (&Lc)[GM_MAX_K]) {
  float mx[GM_MAX_K], sum[GM_MAX_K];
#pragma unroll
  for (int c = 0; c < GM_MAX_K; ++c) { mx[c] = -__builtin_inff(); sum[c] = 0.f; }
#pragma unroll
  for (int k = 0; k < GM_MAX_K; ++k)
    if (k < K) {
      const int ck = (cls >> (4 * k)) & 15;
#pragma unroll
      for (int c = 0; c < GM_MAX_K; ++c) mx[c] = ck == c ? fmaxf(mx[c], l[k]) : mx[c];
    }
#pragma unroll
  for (int k = 0; k < GM_MAX_K; ++k)
    if (k < K) {
      const int ck = (cls >> (4 * k)) & 15;
      float m = mx[0];
#pragma unroll
      for (int c = 1; c < GM_MAX_K; ++c) m = ck == c ? mx[c] : m;
      const float e = expf(l[k] - m);
#pragma unroll
      for (int c = 0; c < GM_MAX_K; ++c) sum[c] = ck == c ? sum[c] + e : sum[c];
    }
#pragma unroll
  for (int c = 0; c < GM_MAX_K; ++c) Lc[c] = mx[c] + logf(sum[c]);
}

// ---- score -----------------------------------------------------------------------------------------------------------
template <int NKB>
__global__ __launch_bounds__(BAND_THREADS) void band_gmm_score_kernel(const float* __restrict__ x, long long P, long long plane, int q4,
                                                                      const float* __restrict__ pivot, const float* __restrict__ W, int qp,
                                                                      const float* __restrict__ A, const float* __restrict__ a,
                                                                      const float* __restrict__ cst, unsigned cls, int K, int C, int tile,
                                                                      float* __restrict__ loglik, float* __restrict__ logit,
                                                                      unsigned char* __restrict__ labels, float* __restrict__ resp,
                                                                      float* __restrict__ nll) {
  extern __shared__ float gm[];
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int cs = 4 * q4, ldx = band_tile_stride(cs);
  const GmLds s = gm_carve(gm, cs, qp, K, tile);
  const int col = lane & 15, kq = lane >> 4;
  BandRows<NKB> rows;
  gm_stage<NKB>(s, W, pivot, A, a, cst, cs, qp, K, t, col, kq, rows);
  const long long tiles = (P + tile - 1) / tile;
  f32x4 v[GM_LOADS];
  int ql = q4;
  auto load = [&](long long tl) {
    const long long p0 = tl * tile;
    const int left = (int)min((long long)tile, P - p0) * ql;         // quads of the tile that lie inside the batch
#pragma unroll
    for (int u = 0; u < GM_LOADS; ++u) {
      const int idx = t + u * BAND_THREADS;
      v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (idx < left) v[u] = *reinterpret_cast<const f32x4*>(x + p0 * cs + 4LL * idx);
    }
  };
  float* pvl = s.pvl;
  const auto centre = [pvl](f32x4 w, int cq) { return w - *reinterpret_cast<const f32x4*>(pvl + 4 * cq); };
  const bool active = wave * 16 < tile;
  const int px = wave * 16 + col;
  const bool by_class = loglik != nullptr || logit != nullptr || labels != nullptr;
  const bool by_all = resp != nullptr || nll != nullptr;
  if (blockIdx.x < tiles) load(blockIdx.x);
  for (long long tl = blockIdx.x; tl < tiles; tl += gridDim.x) {
    __syncthreads();                                   // (the rows are in LDS; the previous tile and its z have been consumed)
    asm volatile("" : "+s"(ql));
    band_tile_stage<GM_LOADS, BAND_THREADS>(s.xl, v, t, tile * q4, ql, ldx, centre);
    __syncthreads();
    if (tl + gridDim.x < tiles) load(tl + gridDim.x);
    if (active) {
      f32x4 acc[NKB], unused;
      band_scores<NKB, false>(s.xl + px * ldx + kq, s.wl + kq * GM_KP, rows, cs, acc, unused);
      gm_store_z<NKB>(s.zl + px * GM_ZS, acc, kq);
    }
    __syncthreads();
    if (active) {
      float l[GM_MAX_K];
      gm_logdens<NKB>(s, s.zl + px * GM_ZS, rows, qp, K, kq, l);
      const long long pix = tl * tile + px;
      if (pix < P) {
        const long long img = pix / plane, off = pix - img * plane;
        if (by_class) {
          float Lc[GM_MAX_K];
          gm_lse_classes(l, K, cls, Lc);
          if (kq == 0 && loglik != nullptr) {
#pragma unroll
            for (int c = 0; c < GM_MAX_K; ++c)
              if (c < C) loglik[(img * C + c) * plane + off] = Lc[c];
          }
          if (kq == 1 && logit != nullptr) logit[pix] = Lc[1] - Lc[0];
          if (kq == 2 && labels != nullptr) {
            int best = -1;
            float bl = 0.f;
#pragma unroll
            for (int c = 0; c < GM_MAX_K; ++c) {
              const bool take = c < C && (best < 0 || Lc[c] > bl);
              best = take ? c : best;
              bl = take ? Lc[c] : bl;
            }
            labels[pix] = (unsigned char)best;
          }
        }
        if (by_all) {
          float rk[GM_MAX_K];
          const float La = gm_mix_all(l, K, rk);
          if (kq == 3 && nll != nullptr) nll[pix] = -La;
          if (kq == 0 && resp != nullptr) {
#pragma unroll
            for (int k = 0; k < GM_MAX_K; ++k)
              if (k < K) resp[(img * K + k) * plane + off] = rk[k];
          }
        }
      }
    }
  }
}

// ---- sums ------------------------------------------------------------------------------------------------------------
template <typename T, int NKB, bool Q32>
__global__ __launch_bounds__(BAND_THREADS) void band_gmm_sums_kernel(const T* __restrict__ cache, const unsigned char* __restrict__ masks,
                                                                     const int* __restrict__ table, int slots, long long P, int q4,
                                                                     int runs_per_slot, long long runs, int select,
                                                                     const float* __restrict__ pivot, const float* __restrict__ W, int q,
                                                                     int qp, const float* __restrict__ A, const float* __restrict__ a,
                                                                     const float* __restrict__ cst, const float* __restrict__ means, int K,
                                                                     int tile, double* __restrict__ part, double* __restrict__ part_ll,
                                                                     unsigned long long* __restrict__ part_cnt) {
  constexpr int NTQ = Q32 ? 2 : 1;                     // fp32 tiles of a component
  extern __shared__ float gm[];
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int cs = 4 * q4, ldx = band_tile_stride(cs);
  const GmLds s = gm_carve(gm, cs, qp, K, tile);
  const int col = lane & 15, kq = lane >> 4;
  BandRows<NKB> rows;
  gm_stage<NKB>(s, W, pivot, A, a, cst, cs, qp, K, t, col, kq, rows);
  for (int i = t; i < tile * ldx; i += BAND_THREADS) s.xl[i] = 0.f;            // (the columns [cs, ldx) stay zero)
  // this wave's components k = wave, wave + 4 and, per lane, the entry `row` of their means: -1 at row q (e = 0 - -1 = 1, the
  // constant of X), 0 beyond
  const int row = lane & 31, half = lane >> 5;
  const int live = K > wave ? (K - wave + 3) >> 2 : 0;
  float mk[2], m31[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int k = wave + 4 * c;
    mk[c] = row == q ? -1.f : 0.f;
    m31[c] = 0.f;
    if (c < live && row < q) mk[c] = means[k * qp + row];
    if (Q32 && c < live) m31[c] = means[k * qp + 31];
  }
  const long long pstride = (long long)K * NTQ * 1024;
  // the workgroup's partial starts from zero (the barriers of the first chunk order these stores before the first promotion)
  for (int i = t; i < K * NTQ * 1024; i += BAND_THREADS) part[(long long)blockIdx.x * pstride + i] = 0.;
  double all = 0.;
  unsigned long long counted = 0ull;
  const int total = tile * q4;
  const int px0 = t / q4, cq0 = t - px0 * q4, dq = BAND_THREADS / q4, dr = BAND_THREADS - dq * q4;
  const bool active = wave * 16 < tile;
  const int mypx = wave * 16 + col;
  for (long long r = blockIdx.x; r < runs; r += GM_PARTS) {
    const BandRun run = band_run(table, slots, P, runs_per_slot, r);
    f32x16 acc[2][NTQ];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int y = 0; y < NTQ; ++y)
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[c][y][j] = 0.f;
    // a chunk's quads as loaded (widened, pivoted and selected when they are stored into LDS, one chunk later) and their pixel's mask
    // byte (-1: past the run); quad t + 256 u of a chunk is (pixel, channel quad) = (px0, cq0) + u (dq, dr) with a carry
    decltype(band_raw(cache)) v[GM_LOADS];
    int keep[GM_LOADS];
    auto load = [&](int c0, int px, int cq) {
#pragma unroll
      for (int u = 0; u < GM_LOADS; ++u) {
        const int idx = t + u * BAND_THREADS;
        keep[u] = -1;
        if (idx < total && c0 + px < run.len) {
          const long long pix = run.base + c0 + px;
          v[u] = band_raw(cache + pix * cs + 4 * cq);
          keep[u] = select == 0 ? 1 : (int)masks[pix];
        }
        cq += dr;
        px += dq;
        if (cq >= q4) { cq -= q4; ++px; }
      }
    };
    int pxs = px0, cqs = cq0;
    asm volatile("" : "+v"(pxs), "+v"(cqs));
    load(0, pxs, cqs);
    for (int c0 = 0; c0 < run.len; c0 += tile) {
      __syncthreads();                                 // (the rows are in LDS; the previous chunk, its z and r have been consumed)
      asm volatile("" : "+v"(pxs), "+v"(cqs));
      int px = pxs, cq = cqs;
#pragma unroll
      for (int u = 0; u < GM_LOADS; ++u, cq += dr, px += dq) {
        const int idx = t + u * BAND_THREADS;
        if (cq >= q4) { cq -= q4; ++px; }
        if (idx < total) {
          const bool on = keep[u] >= 0 && (select == 0 || (keep[u] != 0) == (select == 1));
          f32x4 d = {0.f, 0.f, 0.f, 0.f};
          if (on) d = band_widen(v[u]) - *reinterpret_cast<const f32x4*>(s.pvl + 4 * cq);
          float2* dst = reinterpret_cast<float2*>(s.xl + px * ldx + 4 * cq);
          dst[0] = float2{d[0], d[1]};
          dst[1] = float2{d[2], d[3]};
          if (cq == 0) s.sel[px] = on ? 1 : 0;
        }
      }
      __syncthreads();
      if (c0 + tile < run.len) load(c0 + tile, pxs, cqs);
      if (active) {
        f32x4 sc[NKB], unused;
        band_scores<NKB, false>(s.xl + mypx * ldx + kq, s.wl + kq * GM_KP, rows, cs, sc, unused);
        gm_store_z<NKB>(s.zl + mypx * GM_ZS, sc, kq);
      }
      __syncthreads();
      if (active) {
        float l[GM_MAX_K];
        gm_logdens<NKB>(s, s.zl + mypx * GM_ZS, rows, qp, K, kq, l);
        float rk[GM_MAX_K];
        const float La = gm_mix_all(l, K, rk);
        if (kq == 0) {
          const bool on = s.sel[mypx] != 0;
#pragma unroll
          for (int k = 0; k < GM_MAX_K; ++k)
            if (k < K) s.rl[mypx * GM_MAX_K + k] = on ? rk[k] : 0.f;
          if (on) {
            all += (double)La;
            ++counted;
          }
        }
      }
      __syncthreads();
      // two pixels a step, ascending: r X of the pixel against its X
      for (int p = 0; p < tile; p += 2) {
        const float* zp = s.zl + (p + half) * GM_ZS;
        const float* rp = s.rl + (p + half) * GM_MAX_K + wave;
        const float z = zp[row];
#pragma unroll
        for (int c = 0; c < 2; ++c)
          if (c < live) {
            const float rk = rp[4 * c];
            const float e = z - mk[c];
            const float re = rk * e;
            acc[c][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(re, e, acc[c][0], 0, 0, 0);
            if (Q32) {
              const float up = __shfl_up(re, 1, 32);
              const float e31 = zp[31] - m31[c];
              const float ay = row == 0 ? rk : up;
              const float by = row == 0 ? 1.f : row == 1 ? e31 : 0.f;
              acc[c][NTQ - 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(ay, by, acc[c][NTQ - 1], 0, 0, 0);
            }
          }
      }
    }
    // promote: fp32 tiles -> the fp64 tiles of this partial; D: column = l & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (l >> 5)
    // (the empty asm keeps the tile addresses from being computed once before the run loop and held in registers)
    double* pb = part + (long long)blockIdx.x * pstride + (4 * half) * 32 + row;
    asm volatile("" : "+v"(pb));
    int lv = live;
    asm volatile("" : "+s"(lv));
#pragma unroll
    for (int c = 0; c < 2; ++c) {
#pragma unroll
      for (int y = 0; y < NTQ; ++y) {
        if (c < lv) {
          double* tp = pb + (long long)((wave + 4 * c) * NTQ + y) * 1024;
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            double* d = tp + ((j & 3) + 8 * (j >> 2)) * 32;
            *d += (double)acc[c][y][j];
          }
        }
        __builtin_amdgcn_sched_barrier(0);             // (one tile's sixteen doubles in flight at a time, not all of them)
      }
    }
  }
  // the lane sums of pixel slot (wave, col), added in ascending slot order by one thread
  __syncthreads();
  if (kq == 0) {
    s.tot[wave * 16 + col] = all;
    s.cnt[wave * 16 + col] = counted;
  }
  __syncthreads();
  if (t == 0) {
    double ll = 0.;
    unsigned long long n = 0ull;
    for (int i = 0; i < GM_TILE; ++i) { ll += s.tot[i]; n += s.cnt[i]; }
    part_ll[blockIdx.x] = ll;
    part_cnt[blockIdx.x] = n;
  }
}

// N[k], S[k][i], Q[k][i][j] (strides of qp; zeros from q on), LL and the count: the partials in ascending order
__global__ void band_gmm_finish_kernel(const double* __restrict__ part, const double* __restrict__ part_ll,
                                       const unsigned long long* __restrict__ part_cnt, int parts, int q, int qp, int K,
                                       long long* __restrict__ count, double* __restrict__ N, double* __restrict__ S, double* __restrict__ Q,
                                       double* __restrict__ LL) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  const int ntq = q == 32 ? 2 : 1;
  const long long pstride = (long long)K * ntq * 1024;
  const auto total = [&](int k, int y, int i, int j) {
    const long long off = (long long)(k * ntq + y) * 1024 + i * 32 + j;
    double a = 0.;
    for (int p = 0; p < parts; ++p) a += part[(long long)p * pstride + off];
    return a;
  };
  if (e < K * qp * qp) {
    const int k = e / (qp * qp), ij = e - k * qp * qp, i = ij / qp, j = ij - i * qp;
    Q[e] = i < q && j < q ? total(k, 0, i, j) : 0.;
  }
  if (e < K * qp) {
    const int k = e / qp, i = e - k * qp;
    S[e] = i >= q ? 0. : q < 32 ? total(k, 0, i, q) : i < 31 ? total(k, 1, i + 1, 0) : total(k, 1, 0, 1);
  }
  if (e < K) N[e] = q < 32 ? total(e, 0, q, q) : total(e, 1, 0, 0);
  if (e == 0) {
    double ll = 0.;
    unsigned long long n = 0ull;
    for (int p = 0; p < parts; ++p) { ll += part_ll[p]; n += part_cnt[p]; }
    *LL = ll;
    *count = (long long)n;
  }
}
#endif

// ---- host ------------------------------------------------------------------------------------------------------------
extern "C" int hpri_band_gmm_max_components(void) { return GM_MAX_K; }
extern "C" int hpri_band_gmm_max_dims(void) { return GM_MAX_Q; }
extern "C" int hpri_band_gmm_parts(void) { return GM_PARTS; }

static inline bool gm_model_ok(int q, int K) { return q > 0 && q <= GM_MAX_Q && K > 0 && K <= GM_MAX_K; }
static inline size_t gm_part_doubles(int q, int K) { return (size_t)K * (q == 32 ? 2 : 1) * 1024; }

// 0 for a channel stride, a q or a K the pass does not take
extern "C" size_t hpri_band_gmm_workspace_bytes(int cs, int q, int K) {
  if (!band_cs_ok(cs) || !gm_model_ok(q, K)) return 0;
  return (size_t)GM_PARTS * (gm_part_doubles(q, K) + 2) * 8;
}

extern "C" int hpri_band_gmm_score(const float* x, long long pixels, long long plane, int cs, const float* pivot, const float* weight,
                                   int q, const float* A, const float* a, const float* c, const int* classes, int K, int C, float* loglik,
                                   float* logit, unsigned char* labels, float* resp, float* nll, hipStream_t stream) {
  HPRI_REQUIRE(x && weight && A && a && c && classes, "band_gmm_score: null pointer");
  HPRI_REQUIRE(pixels > 0 && plane > 0 && pixels % plane == 0, "band_gmm_score: bad sizes");
  HPRI_REQUIRE(band_cs_ok(cs), "band_gmm_score: the channel stride must be a multiple of 8 up to hpri_band_max_cs");
  HPRI_REQUIRE(gm_model_ok(q, K), "band_gmm_score: q must lie in [1, hpri_band_gmm_max_dims], K in [1, hpri_band_gmm_max_components]");
  HPRI_REQUIRE(C > 0 && C <= GM_MAX_K, "band_gmm_score: the classes must number 1 to hpri_band_gmm_max_components");
  unsigned cls = 0;
  for (int k = 0; k < K; ++k) {
    HPRI_REQUIRE(classes[k] >= 0 && classes[k] < C, "band_gmm_score: a component's class must lie in [0, C)");
    cls |= (unsigned)classes[k] << (4 * k);
  }
  HPRI_REQUIRE(loglik || logit || labels || resp || nll, "band_gmm_score: nothing to write");
  HPRI_REQUIRE(logit == nullptr || C == 2, "band_gmm_score: the logit needs exactly two classes");
  HPRI_REQUIRE(hpri_aligned16(x, pivot, weight, A, a) &&
               (((uintptr_t)c | (uintptr_t)loglik | (uintptr_t)logit | (uintptr_t)resp | (uintptr_t)nll) & 3) == 0,
               "band_gmm_score: misaligned pointer");
  const int qp = (q + 7) & ~7, tile = gm_tile(cs, qp, K);
  const size_t lds = gm_lds_bytes(cs, qp, K, tile);
  const long long tiles = (pixels + tile - 1) / tile;
  const long long per_cu = BAND_LDS_BYTES / (long long)lds;
  const dim3 grid = cache_grid(tiles, (int)(per_cu < 1 ? 1 : per_cu > 4 ? 4 : per_cu));
#define GM_SCORE_LAUNCH(NKB_)                                                                                                      \
  do {                                                                                                                             \
    hpri_ask_dynamic_lds(band_gmm_score_kernel<NKB_>, lds);                                                                        \
    hipLaunchKernelGGL((band_gmm_score_kernel<NKB_>), grid, dim3(BAND_THREADS), lds, stream, x, pixels, plane, cs / 4, pivot, weight, qp, \
                       A, a, c, cls, K, C, tile, loglik, logit, labels, resp, nll);                                                \
  } while (0)
  if (qp <= 16) GM_SCORE_LAUNCH(1);
  else GM_SCORE_LAUNCH(2);
#undef GM_SCORE_LAUNCH
  HPRI_CHECK_LAUNCH();
  return HPRI_OK;
}

extern "C" int hpri_band_gmm_sums(const void* cache, int cache_dtype, int slots, int Hs, int Ws, int cs, const unsigned char* masks,
                                  const int* slot_table, int n, int select, const float* pivot, const float* weight, int q, const float* A,
                                  const float* a, const float* c, const float* means, int K, void* workspace, size_t workspace_bytes,
                                  long long* count, double* N, double* S, double* Q, double* LL, hipStream_t stream) {
  const BandPass p = {"band_gmm_sums", cache, cache_dtype, slots, Hs, Ws, cs, masks, slot_table, n, select};
  CACHE_REQUIRE(p.who, weight && A && a && c && means && count && N && S && Q && LL, "null pointer");
  if (int e = band_check(p, workspace, 0, 0)) return e;
  CACHE_REQUIRE(p.who, gm_model_ok(q, K), "q must lie in [1, hpri_band_gmm_max_dims], K in [1, hpri_band_gmm_max_components]");
  CACHE_REQUIRE(p.who, workspace_bytes >= hpri_band_gmm_workspace_bytes(cs, q, K), "the workspace is smaller than hpri_band_gmm_workspace_bytes");
  CACHE_REQUIRE(p.who, hpri_aligned16(pivot, weight, A, a) && (((uintptr_t)c | (uintptr_t)means) & 3) == 0 &&
                           (((uintptr_t)count | (uintptr_t)N | (uintptr_t)S | (uintptr_t)Q | (uintptr_t)LL) & 7) == 0,
                "misaligned pointer");
  const long long P = (long long)Hs * Ws;
  const int rps = (int)((P + BAND_FP32_RUN - 1) / BAND_FP32_RUN);
  const long long runs = (long long)n * rps;
  const int parts = (int)(runs < GM_PARTS ? runs : GM_PARTS);
  const int qp = (q + 7) & ~7, tile = gm_tile(cs, qp, K);
  const size_t lds = gm_lds_bytes(cs, qp, K, tile);
  double* part = (double*)workspace;
  double* part_ll = part + (size_t)GM_PARTS * gm_part_doubles(q, K);
  unsigned long long* part_cnt = (unsigned long long*)(part_ll + GM_PARTS);
#define GM_SUMS_LAUNCH(T_, NKB_, Q32_)                                                                                             \
  do {                                                                                                                             \
    hpri_ask_dynamic_lds(band_gmm_sums_kernel<T_, NKB_, Q32_>, lds);                                                               \
    hipLaunchKernelGGL((band_gmm_sums_kernel<T_, NKB_, Q32_>), dim3(parts), dim3(BAND_THREADS), lds, stream, (const T_*)cache, masks, \
                       slot_table, slots, P, cs / 4, rps, runs, select, pivot, weight, q, qp, A, a, c, means, K, tile, part, part_ll, \
                       part_cnt);                                                                                                  \
  } while (0)
#define GM_SUMS_DTYPE(NKB_, Q32_)                                                                                                  \
  do {                                                                                                                             \
    if (cache_dtype == 0) GM_SUMS_LAUNCH(float, NKB_, Q32_);                                                                       \
    else GM_SUMS_LAUNCH(_Float16, NKB_, Q32_);                                                                                     \
  } while (0)
  if (qp <= 16) GM_SUMS_DTYPE(1, false);
  else if (q < 32) GM_SUMS_DTYPE(2, false);
  else GM_SUMS_DTYPE(2, true);
#undef GM_SUMS_DTYPE
#undef GM_SUMS_LAUNCH
  HPRI_CHECK_LAUNCH();
  const int items = K * qp * qp;
  hipLaunchKernelGGL(band_gmm_finish_kernel, dim3((items + 255) / 256), dim3(256), 0, stream, (const double*)part, (const double*)part_ll,
                     (const unsigned long long*)part_cnt, parts, q, qp, K, count, N, S, Q, LL);
  HPRI_CHECK_LAUNCH();
  return HPRI_OK;
}
