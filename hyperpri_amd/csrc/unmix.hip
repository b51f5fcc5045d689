// Spectral unmixing (hyperpri_amd/unmix.py): the abundances of a batch under the linear mixing model x ~ E a, in one pass, and one
// ATGP step (the pixel with the largest residual after projecting out the rows found so far) over the cube cache's slots.
//
//   y[m]  = fmaf(Q32[m][cs-1], x[cs-1], ... fmaf(Q32[m][0], x[0], 0))           m < M    (fp32 MFMA chain, ascending c)
//   b     = R^T y,  a = argmin 1/2 a^T G a - b^T a  under the mode                        (fp64; G = R^T R, E = Q R the thin QR)
//   a32   = (float)a, M planes (M, P)
//   r[c]  = fmaf(-E32[M-1][c], a32[M-1], ... fmaf(-E32[0][c], a32[0], x[c]))              (fp32)
//   rmse  = sqrtf(s / C),  s = fmaf(r[c], r[c], s) ascending c over cs, from 0
//   value = logit(clamp(sum over the foreground members of a32[m], 2^-24, 1 - 2^-24))     (fp32, ascending m)
//
// include/hyperpri_hip.h states the modes and the active-set rule in full.
//
// Layout.  A workgroup is four waves and owns one tile of UM_TILE = 64 pixels at a time (a persistent grid of two workgroups per CU
// -- one where two tiles do not fit the LDS).  The tile sits in LDS as band_common.h keeps it (band_tile_load, band_tile_stage: rows at
// band_tile_stride(cs), written as 8-byte pairs); the 16 basis rows (15 KB at cs = 240) are streamed from L2, not staged: a
// lane's consecutive k-steps walk one cache line.  v_mfma_f32_16x16x4_f32: wave w multiplies the 16 rows against its 16 pixels;
// lane l holds A[i = l & 15][k = l >> 4] = Q32[i][c + k] and B[k][j = l & 15] = x[pixel 16 w + j][c + k]; D: column (pixel) = l & 15,
// row = 4 (l >> 4) + reg.  y goes to LDS.
// The waves are specialised: wave 0 solves -- one lane per pixel, fp64, everything in registers -- while the waves 1 .. 3 fetch the
// next tile global -> registers (the solver wave carries no prefetch registers, the loaders no factor).  The loop bodies of the two
// kinds are instances of one function and meet at the same barriers.  The second workgroup of the CU multiplies meanwhile.
// The residuals are then formed by all four waves (thread (pixel, quarter of the bands), in place over the tile) and the 64 lanes of
// wave 0 add the squares in ascending c.
//
// The solver holds no array that is indexed by a run-time value (such an array would live in scratch, see DetExtents in
// detect.hip): the kernel is a template on M, every loop over members is unrolled, the support is a bit mask, and a clamped
// variable's row and column are the identity's with a zero right-hand side, so one M x M Cholesky factorisation serves any support.
//
// No floating-point atomic; the result of a pixel depends neither on P, nor on the grid, nor on its place in a tile.  Capped pixels
// are counted with hpri_block_count4.
//
// hpri_band_extreme: the same tile, projection and residual code over the tiles of the listed slots (both cache dtypes), K <= 8 rows:
//   v = sum fmaf(r[c], r[c], v),  r[c] = fmaf(-Q32[K-1][c], y[K-1], ... fmaf(-Q32[0][c], y[0], x[c]))
// Each lane of wave 0 keeps the best (v, position) of the pixels it saw -- a later one wins only when v is strictly larger or equal
// at a lower position --, the workgroup's best goes to the workspace and a one-thread kernel picks among the partials in ascending
// order by the same rule: the result is the maximum of a total order and does not depend on the grid.
#include "band_common.h"

#define UM_THREADS 256
#define UM_TILE 64
#define UM_MAX_M 8
#define UM_ROWS 16                      // rows of the padded basis: one block of the MFMA
#define UM_LOADERS (UM_THREADS - 64)    // unmix: the waves 1 .. 3 fetch
#define UM_LOADS ((UM_TILE * (BAND_MAX_CS / 4) + UM_LOADERS - 1) / UM_LOADERS)
#define UM_XLOADS ((UM_TILE * (BAND_MAX_CS / 4) + UM_THREADS - 1) / UM_THREADS)
#define UM_TAU 9.094947017729282e-13        // 2^-40
#define UM_PARTIALS HPRI_MAX_BLOCKS         // the most workgroups of the ATGP pass: the workspace holds one (v, position) each

// ---- what the two kernels share ----------------------------------------------------------------------------------------------------
// the 16 basis rows against the 16 pixels of this wave; two k-steps per iteration (cs % 8 == 0), the operands of the next iteration
// read before this one's MFMAs issue (the last iteration reads its own again).  (A queue that keeps the basis operands six
// iterations ahead measured slower, DESIGN.md.)
__device__ __forceinline__ f32x4 um_project(const float* __restrict__ xr, const float* __restrict__ wr, int cs) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  float a0 = wr[0], a1 = wr[4], b0 = xr[0], b1 = xr[4];
  for (int c = 0; c < cs; c += 8) {
    const int cn = min(c + 8, cs - 8);
    const float na0 = wr[cn], na1 = wr[cn + 4], nb0 = xr[cn], nb1 = xr[cn + 4];
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc, 0, 0, 0);
    a0 = na0; a1 = na1; b0 = nb0; b1 = nb1;
  }
  return acc;
}

// rows k < K of the product go to yb[k][pixel] (the lanes l >> 4 < 2 hold the rows 0 .. 7)
__device__ __forceinline__ void um_put_rows(float* __restrict__ yb, const f32x4& acc, int K, int px, int kq) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int k = 4 * kq + j;
    if (k < K) yb[k * UM_TILE + px] = acc[j];
  }
}

// r[c] = fmaf(-rows[K-1][c], co[K-1], ... fmaf(-rows[0][c], co[0], x[c])) over this wave's quarter of the bands, in place; co[k] =
// cb[k][pixel].  (rows + k cs + c is the same address in every lane of a wave.)
__device__ __forceinline__ void um_residual(float* __restrict__ xrow, const float* __restrict__ rows, const float* __restrict__ cb, int K,
                                            int cs, int wave, int px) {
  float co[UM_MAX_M];
#pragma unroll
  for (int k = 0; k < UM_MAX_M; ++k) co[k] = k < K ? cb[k * UM_TILE + px] : 0.f;
  const int c0 = wave * (cs >> 2), c1 = c0 + (cs >> 2);
  for (int c = c0; c < c1; c += 2) {
    float2 r = *reinterpret_cast<const float2*>(xrow + c);
#pragma unroll
    for (int k = 0; k < UM_MAX_M; ++k) {
      if (k < K) {
        const float2 e = *reinterpret_cast<const float2*>(rows + k * cs + c);
        r.x = fmaf(-e.x, co[k], r.x);
        r.y = fmaf(-e.y, co[k], r.y);
      }
    }
    *reinterpret_cast<float2*>(xrow + c) = r;
  }
}

__device__ __forceinline__ float um_sumsq(const float* __restrict__ xrow, int cs) {
  float s = 0.f;
  for (int c = 0; c < cs; c += 2) {
    const float2 r = *reinterpret_cast<const float2*>(xrow + c);
    s = fmaf(r.x, r.x, s);
    s = fmaf(r.y, r.y, s);
  }
  return s;
}

// ---- the solver: one lane, one pixel, fp64 -----------------------------------------------------------------------------------------
template <int M> struct UmState {
  double L[M * (M + 1) / 2];            // the factor, row i at i (i + 1) / 2; its diagonal is kept as the reciprocal in inv
  double inv[M];
  double u[M], v[M];
};

// G with the rows and columns outside S replaced by the identity's = L L^T
template <int M>
__device__ __forceinline__ void um_factor(const double* __restrict__ G, unsigned S, UmState<M>& st) {
#pragma unroll
  for (int j = 0; j < M; ++j) {
    const bool sj = (S >> j) & 1u;
    double d = sj ? G[j * M + j] : 1.0;
#pragma unroll
    for (int k = 0; k < j; ++k) d = fma(-st.L[j * (j + 1) / 2 + k], st.L[j * (j + 1) / 2 + k], d);
    st.inv[j] = 1.0 / sqrt(d);
#pragma unroll
    for (int i = j + 1; i < M; ++i) {
      double e = (sj && ((S >> i) & 1u)) ? G[i * M + j] : 0.0;
#pragma unroll
      for (int k = 0; k < j; ++k) e = fma(-st.L[i * (i + 1) / 2 + k], st.L[j * (j + 1) / 2 + k], e);
      st.L[i * (i + 1) / 2 + j] = e * st.inv[j];
    }
  }
}

// x = (L L^T)^-1 rhs, in place
template <int M>
__device__ __forceinline__ void um_solve(const UmState<M>& st, double (&x)[M]) {
#pragma unroll
  for (int i = 0; i < M; ++i) {
    double z = x[i];
#pragma unroll
    for (int k = 0; k < i; ++k) z = fma(-st.L[i * (i + 1) / 2 + k], x[k], z);
    x[i] = z * st.inv[i];
  }
#pragma unroll
  for (int i = M - 1; i >= 0; --i) {
    double z = x[i];
#pragma unroll
    for (int k = i + 1; k < M; ++k) z = fma(-st.L[k * (k + 1) / 2 + i], x[k], z);
    x[i] = z * st.inv[i];
  }
}

// the minimiser on the support S (zero elsewhere) into st.u, and its multiplier; eq: the sum-to-one constraint is carried
template <int M>
__device__ __forceinline__ double um_subsolve(const double* __restrict__ G, const double (&b)[M], unsigned S, bool eq, UmState<M>& st) {
  um_factor<M>(G, S, st);
#pragma unroll
  for (int i = 0; i < M; ++i) st.u[i] = ((S >> i) & 1u) ? b[i] : 0.0;
  um_solve<M>(st, st.u);
  double lam = 0.0;
  if (eq) {
#pragma unroll
    for (int i = 0; i < M; ++i) st.v[i] = ((S >> i) & 1u) ? 1.0 : 0.0;
    um_solve<M>(st, st.v);
    double su = 0.0, sv = 0.0;
#pragma unroll
    for (int i = 0; i < M; ++i) { su += st.u[i]; sv += st.v[i]; }
    lam = (su - 1.0) / sv;
#pragma unroll
    for (int i = 0; i < M; ++i) st.u[i] = fma(-lam, st.v[i], st.u[i]);
  }
#pragma unroll
  for (int i = 0; i < M; ++i) st.u[i] = ((S >> i) & 1u) ? st.u[i] : 0.0;
  return lam;
}

// tri: R (M x M, row-major, upper triangular) then G = R^T R.  Returns whether the pixel reached the cap.
template <int M>
__device__ __forceinline__ bool um_pixel(const double* __restrict__ tri, const float (&y)[M], int mode, int cap, double (&a)[M]) {
  const double* __restrict__ G = tri + M * M;
  double b[M];
  double ymax = 1.0, gmax = 0.0;
#pragma unroll
  for (int m = 0; m < M; ++m) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k <= m; ++k) s = fma(tri[k * M + m], (double)y[k], s);
    b[m] = s;
    ymax = fmax(ymax, fabs((double)y[m]));
    gmax = fmax(gmax, G[m * M + m]);
  }
  const double tau = UM_TAU * gmax * ymax;
  const bool eq = mode & 1;
  UmState<M> st;
  if (!(mode & 2)) {                    // ucls, scls: one solve on the full support
    um_subsolve<M>(G, b, (1u << M) - 1u, eq, st);
#pragma unroll
    for (int i = 0; i < M; ++i) a[i] = st.u[i];
    return false;
  }
  unsigned S = 0u;
#pragma unroll
  for (int i = 0; i < M; ++i) a[i] = 0.0;
  if (eq) {
    int j = 0;
    double best = fma(-0.5, G[0], b[0]);
#pragma unroll
    for (int i = 1; i < M; ++i) {
      const double f = fma(-0.5, G[i * M + i], b[i]);
      if (f > best) { best = f; j = i; }
    }
    S = 1u << j;
#pragma unroll
    for (int i = 0; i < M; ++i) a[i] = i == j ? 1.0 : 0.0;
  }
  for (int it = 0;; ++it) {
    if (it == cap) return true;
    const double lam = um_subsolve<M>(G, b, S, eq, st);
    bool feasible = true;
#pragma unroll
    for (int i = 0; i < M; ++i) feasible = feasible && (!((S >> i) & 1u) || st.u[i] > 0.0);
    if (feasible) {
      int j = -1;
      double best = 0.0;
#pragma unroll
      for (int i = 0; i < M; ++i) {
        a[i] = st.u[i];
        double w = b[i] - lam;
#pragma unroll
        for (int k = 0; k < M; ++k) w = fma(-G[i * M + k], st.u[k], w);
        if (!((S >> i) & 1u) && (j < 0 || w > best)) { best = w; j = i; }
      }
      if (j < 0 || !(best > tau)) return false;
      S |= 1u << j;
    } else {
      double alpha = 2.0;
#pragma unroll
      for (int i = 0; i < M; ++i) {
        if (((S >> i) & 1u) && st.u[i] <= 0.0) {
          const double ratio = a[i] == 0.0 ? 0.0 : a[i] / (a[i] - st.u[i]);
          st.v[i] = ratio;
          alpha = fmin(alpha, ratio);
        }
      }
#pragma unroll
      for (int i = 0; i < M; ++i) {
        const bool in = (S >> i) & 1u;
        const bool hit = in && st.u[i] <= 0.0 && st.v[i] == alpha;
        const double n = fma(alpha, st.u[i] - a[i], a[i]);
        const bool out = hit || !in || !(n > 0.0);
        a[i] = out ? 0.0 : n;
        if (out) S &= ~(1u << i);
      }
    }
  }
}

// ---- unmix -------------------------------------------------------------------------------------------------------------------------
struct UmArgs {
  const float* x; long long P; int q4; const float* basis; const float* members; const double* tri; int mode, cap; unsigned fg; int C;
  float* abund; float* rmse; float* value;
};

template <int M, bool SOLVER>
__device__ __forceinline__ unsigned um_tiles(const UmArgs& g, float* __restrict__ dl) {
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int cs = 4 * g.q4, ldx = band_tile_stride(cs);
  float* xl = dl;                                      // [UM_TILE][ldx]
  float* yb = dl + UM_TILE * ldx;                      // [UM_MAX_M][UM_TILE] y
  float* ab = yb + UM_MAX_M * UM_TILE;                 // [UM_MAX_M][UM_TILE] a32
  const int col = lane & 15, kq = lane >> 4;
  const long long tiles = (g.P + UM_TILE - 1) / UM_TILE;
  const int lt = t - 64;                               // a loader's index
  unsigned ncap = 0;
  f32x4 v[SOLVER ? 1 : UM_LOADS];
  int ql = g.q4;                                       // (hidden from the optimiser per tile: band_tile_stage)
  auto load = [&](long long tile) {
    const long long p0 = tile * UM_TILE;               // (left: the quads of the tile that lie inside the batch)
    band_tile_load<(SOLVER ? 1 : UM_LOADS), UM_LOADERS>(v, g.x + p0 * cs, lt, (int)min((long long)UM_TILE, g.P - p0) * ql);
  };
  if (!SOLVER && blockIdx.x < tiles) load(blockIdx.x);
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    __syncthreads();                                   // (the previous tile has been consumed)
    asm volatile("" : "+s"(ql));
    if (!SOLVER) band_tile_stage<(SOLVER ? 1 : UM_LOADS), UM_LOADERS>(xl, v, lt, UM_TILE * ql, ql, ldx, BandQuadAsIs());
    __syncthreads();
    {
      const int px = wave * 16 + col;
      const f32x4 acc = um_project(xl + px * ldx + kq, g.basis + col * cs + kq, cs);
      um_put_rows(yb, acc, M, px, kq);
    }
    __syncthreads();
    const long long pix = tile * UM_TILE + lane;
    if (SOLVER) {
      float y[M];
#pragma unroll
      for (int m = 0; m < M; ++m) y[m] = yb[m * UM_TILE + lane];
      double a[M];
      ncap += um_pixel<M>(g.tri, y, g.mode, g.cap, a) && pix < g.P ? 1u : 0u;
      float f = 0.f;
#pragma unroll
      for (int m = 0; m < M; ++m) {
        const float a32 = (float)a[m];
        ab[m * UM_TILE + lane] = a32;
        if (pix < g.P) g.abund[(long long)m * g.P + pix] = a32;
        if ((g.fg >> m) & 1u) f += a32;
      }
      if (g.value != nullptr && pix < g.P) g.value[pix] = hpri_clamped_logit(f);
    } else if (tile + gridDim.x < tiles) {
      load(tile + gridDim.x);
    }
    if (g.rmse != nullptr) {
      __syncthreads();
      um_residual(xl + lane * ldx, g.members, ab, M, cs, wave, lane);
      __syncthreads();
      if (SOLVER && pix < g.P) g.rmse[pix] = sqrtf(um_sumsq(xl + lane * ldx, cs) / (float)g.C);
    }
  }
  return ncap;
}

template <int M>
__global__ __launch_bounds__(UM_THREADS, 2) void band_unmix_kernel(UmArgs g, unsigned long long* __restrict__ capped) {
  extern __shared__ float dl[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  unsigned ncap = 0;
  if (wave == 0) ncap = um_tiles<M, true>(g, dl);
  else um_tiles<M, false>(g, dl);
  hpri_block_count4(capped, [&](unsigned int (&c)[4]) { c[0] += ncap; });
}

// ---- one ATGP step -----------------------------------------------------------------------------------------------------------------
struct UmBest { float v; int pad; long long pos; };

__device__ __forceinline__ bool um_better(float v, long long pos, float bv, long long bpos) {
  return pos >= 0 && (bpos < 0 || v > bv || (v == bv && pos < bpos));
}

template <typename T>
__global__ __launch_bounds__(UM_THREADS, 2) void band_extreme_kernel(const T* __restrict__ cache, const unsigned char* __restrict__ masks,
                                                                     const int* __restrict__ table, int slots, long long P, int q4,
                                                                     long long tiles_per_slot, long long tiles, int select,
                                                                     const float* __restrict__ basis, int K, UmBest* __restrict__ part) {
  extern __shared__ float dl[];
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int cs = 4 * q4, ldx = band_tile_stride(cs);
  float* xl = dl;                                      // [UM_TILE][ldx]
  float* yb = dl + UM_TILE * ldx;                      // [UM_MAX_M][UM_TILE]
  UmBest* wb = reinterpret_cast<UmBest*>(yb + UM_MAX_M * UM_TILE);     // [64], 16-byte aligned: every part before it is
  const int col = lane & 15, kq = lane >> 4;
  decltype(band_raw(cache)) v[UM_XLOADS];
  int ql = q4;
  // tile -> (first pixel in the cache, pixels of the tile that lie inside the slot, position of the first pixel in the list)
  auto place = [&](long long tile, long long& base, int& npix, long long& pos) {
    const long long e = tile / tiles_per_slot, p0 = (tile - e * tiles_per_slot) * UM_TILE;
    const int slot = min(max(table[e], 0), slots - 1);
    base = (long long)slot * P + p0;
    npix = (int)min((long long)UM_TILE, P - p0);
    pos = e * P + p0;
  };
  auto load = [&](long long tile) {
    long long base, pos;
    int npix;
    place(tile, base, npix, pos);
    band_tile_load<UM_XLOADS, UM_THREADS>(v, cache + base * cs, t, npix * ql);
  };
  float bv = 0.f;
  long long bpos = -1;
  if (blockIdx.x < tiles) load(blockIdx.x);
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    __syncthreads();
    asm volatile("" : "+s"(ql));
    band_tile_stage<UM_XLOADS, UM_THREADS>(xl, v, t, UM_TILE * ql, ql, ldx, BandQuadAsIs());
    __syncthreads();
    if (tile + gridDim.x < tiles) load(tile + gridDim.x);
    if (K > 0) {
      const int px = wave * 16 + col;
      const f32x4 acc = um_project(xl + px * ldx + kq, basis + col * cs + kq, cs);
      um_put_rows(yb, acc, K, px, kq);
      __syncthreads();
      um_residual(xl + lane * ldx, basis, yb, K, cs, wave, lane);
      __syncthreads();
    }
    if (wave == 0) {
      long long base, pos;
      int npix;
      place(tile, base, npix, pos);
      if (lane < npix && band_selected(masks, base + lane, select)) {
        const float s = um_sumsq(xl + lane * ldx, cs);
        if (um_better(s, pos + lane, bv, bpos)) { bv = s; bpos = pos + lane; }
      }
    }
  }
  __syncthreads();
  if (wave == 0) {
    wb[lane].v = bv;
    wb[lane].pos = bpos;
  }
  __syncthreads();
  if (t == 0) {
    for (int i = 1; i < 64; ++i)
      if (um_better(wb[i].v, wb[i].pos, bv, bpos)) { bv = wb[i].v; bpos = wb[i].pos; }
    part[blockIdx.x].v = bv;
    part[blockIdx.x].pos = bpos;
  }
}

__global__ void band_extreme_finish_kernel(const UmBest* __restrict__ part, int parts, float* __restrict__ value, long long* __restrict__ position) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  float bv = 0.f;
  long long bpos = -1;
  for (int i = 0; i < parts; ++i)
    if (um_better(part[i].v, part[i].pos, bv, bpos)) { bv = part[i].v; bpos = part[i].pos; }
  value[0] = bv;
  position[0] = bpos;
}

// ---- host --------------------------------------------------------------------------------------------------------------------------
static inline size_t um_lds_bytes(int cs) {
  return ((size_t)UM_TILE * band_tile_stride(cs) + 2 * (size_t)UM_MAX_M * UM_TILE) * 4;
}

extern "C" int hpri_band_unmix_max_members(void) { return UM_MAX_M; }

extern "C" int hpri_band_unmix(const float* x, long long pixels, int cs, int C, const float* basis, const float* members,
                               const double* tri, int M, int mode, int cap, int foreground, float* abundances, float* rmse,
                               float* value, unsigned long long* capped, hipStream_t stream) {
  HPRI_REQUIRE(x && basis && members && tri && abundances && capped, "band_unmix: null pointer");
  HPRI_REQUIRE(pixels > 0, "band_unmix: bad sizes");
  HPRI_REQUIRE(band_cs_ok(cs), "band_unmix: the channel stride must be a multiple of 8 up to hpri_band_max_cs");
  HPRI_REQUIRE(M > 0 && M <= UM_MAX_M, "band_unmix: M must lie in [1, hpri_band_unmix_max_members]");
  HPRI_REQUIRE(C >= M && C <= cs, "band_unmix: the band count must lie in [M, cs]");
  HPRI_REQUIRE(mode >= 0 && mode <= 3, "band_unmix: mode must be 0 (ucls), 1 (scls), 2 (ncls) or 3 (fcls)");
  HPRI_REQUIRE(cap >= 0, "band_unmix: the iteration cap must not be negative (0: 3 M)");
  HPRI_REQUIRE(foreground >= 0 && (foreground >> M) == 0, "band_unmix: the foreground mask names a member beyond M");
  HPRI_REQUIRE(hpri_aligned16(x, basis, members) && (((uintptr_t)tri | (uintptr_t)capped) & 7) == 0 &&
                   (((uintptr_t)abundances | (uintptr_t)rmse | (uintptr_t)value) & 3) == 0,
               "band_unmix: misaligned pointer");
  const size_t lds = um_lds_bytes(cs);
  const long long tiles = (pixels + UM_TILE - 1) / UM_TILE;
  const dim3 grid = cache_grid(tiles, 2 * lds <= BAND_LDS_BYTES ? 2 : 1);
  const UmArgs g = {x, pixels, cs / 4, basis, members, tri, mode, cap == 0 ? 3 * M : cap, (unsigned)foreground, C, abundances, rmse, value};
#define UM_LAUNCH(M_)                                                                                                              \
  case M_:                                                                                                                         \
    hpri_ask_dynamic_lds(band_unmix_kernel<M_>, lds);                                                                              \
    hipLaunchKernelGGL(band_unmix_kernel<M_>, grid, dim3(UM_THREADS), lds, stream, g, capped);                                      \
    break
  switch (M) {
    UM_LAUNCH(1); UM_LAUNCH(2); UM_LAUNCH(3); UM_LAUNCH(4); UM_LAUNCH(5); UM_LAUNCH(6); UM_LAUNCH(7);
    default: hpri_ask_dynamic_lds(band_unmix_kernel<8>, lds); hipLaunchKernelGGL(band_unmix_kernel<8>, grid, dim3(UM_THREADS), lds, stream, g, capped); break;
  }
#undef UM_LAUNCH
  HPRI_CHECK_LAUNCH();
  return HPRI_OK;
}

extern "C" size_t hpri_band_extreme_workspace_bytes(void) { return (size_t)UM_PARTIALS * sizeof(UmBest); }

extern "C" int hpri_band_extreme(const void* cache, int cache_dtype, int slots, int Hs, int Ws, int cs, const unsigned char* masks,
                                 const int* slot_table, int n, int select, const float* basis, int K, void* workspace,
                                 size_t workspace_bytes, float* value, long long* position, hipStream_t stream) {
  const BandPass p = {"band_extreme", cache, cache_dtype, slots, Hs, Ws, cs, masks, slot_table, n, select};
  CACHE_REQUIRE(p.who, value && position, "null pointer");
  if (int e = band_check(p, workspace, workspace_bytes, hpri_band_extreme_workspace_bytes())) return e;
  CACHE_REQUIRE(p.who, K >= 0 && K <= UM_MAX_M, "K must lie in [0, hpri_band_unmix_max_members]");
  CACHE_REQUIRE(p.who, K == 0 || basis != nullptr, "K rows need the basis");
  CACHE_REQUIRE(p.who, hpri_aligned16(basis) && ((uintptr_t)value & 3) == 0 && ((uintptr_t)position & 7) == 0, "misaligned pointer");
  const long long P = (long long)Hs * Ws;
  const long long tps = (P + UM_TILE - 1) / UM_TILE, tiles = tps * n;
  const size_t lds = um_lds_bytes(cs) + 64 * sizeof(UmBest) - (size_t)UM_MAX_M * UM_TILE * 4;
  dim3 grid = cache_grid(tiles, 2 * lds <= BAND_LDS_BYTES ? 2 : 1);
  if (grid.x > UM_PARTIALS) grid.x = UM_PARTIALS;
  UmBest* part = (UmBest*)workspace;
  if (cache_dtype == 0) {
    hpri_ask_dynamic_lds(band_extreme_kernel<float>, lds);
    hipLaunchKernelGGL(band_extreme_kernel<float>, grid, dim3(UM_THREADS), lds, stream, (const float*)cache, masks, slot_table, slots, P,
                       cs / 4, tps, tiles, select, basis, K, part);
  } else {
    hpri_ask_dynamic_lds(band_extreme_kernel<_Float16>, lds);
    hipLaunchKernelGGL(band_extreme_kernel<_Float16>, grid, dim3(UM_THREADS), lds, stream, (const _Float16*)cache, masks, slot_table,
                       slots, P, cs / 4, tps, tiles, select, basis, K, part);
  }
  HPRI_CHECK_LAUNCH();
  hipLaunchKernelGGL(band_extreme_finish_kernel, dim3(1), dim3(64), 0, stream, (const UmBest*)part, (int)grid.x, value, position);
  HPRI_CHECK_LAUNCH();
  return HPRI_OK;
}
