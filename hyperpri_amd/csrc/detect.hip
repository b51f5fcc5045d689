// Spectral detectors (hyperpri_amd/detect.py): a cube plus band statistics -> score maps, in one pass over the batch.
//
//   z[k] = fmaf(W[k][cend-1], x[cend-1], ... fmaf(W[k][0], x[0], b[k]))      every row k < Kq + T     (fp32 MFMA chain, ascending c)
//   q    = sum over k < Kq of z[k]^2                                          (fp32, the order below)
//   t[j] = z[Kq + j],  j < T
//
// x: the zero-padded channels-last fp32 batch (P, cs) hpri_band_project takes; W (ks, cs), b (ks): Kq QUADRATIC rows (a whitener), then
// T <= DET_MAX_T FILTER rows, zero pad rows and columns.  Written: q (P) and T planes of scores (T, P), mapped in the epilogue (raw,
// cosine t * rsqrt(q), or the logit of either).  Nothing of size P x K ever leaves the workgroup.
//
// Layout.  A workgroup is eight waves and owns one tile of DET_TILE = 64 pixels at a time (a persistent grid of two workgroups per
// CU -- one where two tiles do not fit the LDS -- strides over the tiles; 128 registers a lane, so that two fit).  The tile sits in LDS as band_common.h keeps it
// (band_tile_load, band_tile_stage: rows at band_tile_stride(cs), written as 8-byte pairs) and is the B operand of
// EVERY wave: it is read from HBM once, with 16-byte loads, and the next tile travels global -> registers while this one is
// multiplied.  W at cs = 240 is 245 KB and fits no LDS beside a tile, so the 16-row blocks of W are looped over and W is streamed
// from L2: wave w owns the row blocks of its rounds (round r: block 8 r + w, or 8 r + 7 - w in odd rounds -- the serpentine pairs a
// short block of a triangular whitener with a long one) against all four 16-pixel groups of the tile, so one A value feeds four
// MFMAs.  No other wave ever needs that A value: staging W in LDS would add a write, a read and a barrier per block and buy no
// reuse, so the stream goes L2 -> L1 -> register (a lane's consecutive k-steps walk one cache line; the A operands of the next
// two iterations are in flight while this one's eight MFMAs issue), and the LDS holds what IS shared: the tile.
// v_mfma_f32_16x16x4_f32: lane l holds A[i = l & 15][k = l >> 4] = W[16 rb + i][c + k] and B[k][j = l & 15] = x[pixel j][c + k];
// D: column (pixel) = l & 15, row = 4 (l >> 4) + reg.  The k loop of block rb stops at its column extent cend[rb] (a multiple of 8;
// cs without a table): the skipped terms are fmaf(0, x, acc), exact no-ops for finite x up to the sign of a zero.
//
// The order of q (fixed by Kq alone -- not by P, the grid or the pixel's place in its tile).  Lane (w, kq = l >> 4) of a pixel keeps
//   s(w, kq) = fmaf(z, z, s) over the QUADRATIC rows 16 rb + 4 kq + j, j = 0 .. 3, of wave w's blocks rb in round order, from s = 0,
// and one thread per pixel adds the 32 partials from LDS:  q = s(0,0) + s(0,1) + s(0,2) + s(0,3) + s(1,0) + ... + s(7,3), left to right.
// No floating-point atomic; identical arguments give identical bits.
//
// Identity metric (W == NULL, Kq == 0): q = fmaf(x[c], x[c], q) and t[j] = fmaf(F[j][c], x[c], t[j]) ascending c from 0 (from b[j]
// with a bias), F the (T, cs) filter rows.  No matrix unit: the same tile pipeline (one sweep, 16-byte loads), one thread per
// (pixel, chain).
#include "band_common.h"

#define DET_THREADS 512
#define DET_WAVES 8
#define DET_TILE 64
#define DET_MAX_T 8
#define DET_LOADS ((DET_TILE * (BAND_MAX_CS / 4) + DET_THREADS - 1) / DET_THREADS)

// cend[rb] / 8, one byte per block: a table in registers (an array argument indexed by a loop variable would live in scratch)
struct DetExtents { unsigned long long w[3]; };

__device__ __forceinline__ int det_extent(const DetExtents& e, int rb) {
  const unsigned long long v = rb < 8 ? e.w[0] : rb < 16 ? e.w[1] : e.w[2];
  return (int)((v >> (8 * (rb & 7))) & 255ull) * 8;
}

template <bool IDENTITY>
__global__ __launch_bounds__(DET_THREADS, 4) void band_detect_kernel(const float* __restrict__ x, long long P, int q4,
                                                                  const float* __restrict__ W, const float* __restrict__ bias, int ks,
                                                                  int Kq, int T, DetExtents ext, int score, float* __restrict__ qout,
                                                                  float* __restrict__ scores) {
  extern __shared__ float dl[];
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int cs = 4 * q4, ldx = band_tile_stride(cs);
  float* xl = dl;                                      // [DET_TILE][ldx]
  float* qb = dl + DET_TILE * ldx;                     // [DET_WAVES * 4][DET_TILE] partial q (identity: row 0 holds q)
  float* tb = qb + DET_WAVES * 4 * DET_TILE;           // [DET_MAX_T][DET_TILE] filter outputs
  const int col = lane & 15, kq = lane >> 4;
  const int nrb = (Kq + T + 15) >> 4;
  const long long tiles = (P + DET_TILE - 1) / DET_TILE;
  f32x4 v[DET_LOADS];
  // (q4 is hidden from the optimiser per tile, as band_gram_kernel hides it: the ten quotients idx / q4 and the addresses made of
  // them would otherwise be computed once and held in registers across the k loops)
  int ql = q4;
  auto load = [&](long long tile) {
    const long long p0 = tile * DET_TILE;              // (left: the quads of the tile that lie inside the batch)
    band_tile_load<DET_LOADS, DET_THREADS>(v, x + p0 * cs, t, (int)min((long long)DET_TILE, P - p0) * ql);
  };
  if (blockIdx.x < tiles) load(blockIdx.x);
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    __syncthreads();                                   // (the previous tile and its partials have been consumed)
    asm volatile("" : "+s"(ql));
    band_tile_stage<DET_LOADS, DET_THREADS>(xl, v, t, DET_TILE * q4, ql, ldx, BandQuadAsIs());
    __syncthreads();
    if (tile + gridDim.x < tiles) load(tile + gridDim.x);
    if (IDENTITY) {
      // chain j < T: filter j; chain T: q.  Thread (pixel t & 63, group t >> 6) takes the chains group, group + 8.
      const float* xr = xl + (t & 63) * ldx;
      for (int j = wave; j <= T; j += DET_WAVES) {
        if (j < T) {
          const float* f = W + (long long)j * cs;
          float a = bias != nullptr ? bias[j] : 0.f;
          for (int c = 0; c < cs; c += 2) {
            const float2 xv = *reinterpret_cast<const float2*>(xr + c);
            a = fmaf(f[c], xv.x, a);
            a = fmaf(f[c + 1], xv.y, a);
          }
          tb[j * DET_TILE + (t & 63)] = a;
        } else {
          float a = 0.f;
          for (int c = 0; c < cs; c += 2) {
            const float2 xv = *reinterpret_cast<const float2*>(xr + c);
            a = fmaf(xv.x, xv.x, a);
            a = fmaf(xv.y, xv.y, a);
          }
          qb[t & 63] = a;
        }
      }
    } else {
      float qs[4] = {0.f, 0.f, 0.f, 0.f};
      const float* xr = xl + col * ldx + kq;
      for (int r = 0; r * DET_WAVES < nrb; ++r) {
        const int rb = r * DET_WAVES + ((r & 1) ? DET_WAVES - 1 - wave : wave);
        if (rb >= nrb) break;
        const int ce = det_extent(ext, rb);
        const int row = rb * 16 + col;
        const bool live = row < ks;                        // (rows past ks are not read: their A operand is zero)
        const float* wr = W + (long long)min(row, ks - 1) * cs + kq;
        f32x4 acc[4];
        {
          const int n0 = rb * 16 + kq * 4;
          f32x4 b4 = {0.f, 0.f, 0.f, 0.f};
          if (n0 + 3 < ks) b4 = *reinterpret_cast<const f32x4*>(bias + n0);
          else {
#pragma unroll
            for (int j = 0; j < 4; ++j) b4[j] = n0 + j < ks ? bias[n0 + j] : 0.f;
          }
#pragma unroll
          for (int g = 0; g < 4; ++g) acc[g] = b4;
        }
        // two k-steps per iteration (ce % 8 == 0).  A operands: this iteration's, the next one's and the one after are in registers
        // or in flight; B operands of the next iteration are read from LDS before this one's MFMAs issue.  (The last iterations
        // read their own operands again.)
        const int c1 = min(8, ce - 8);
        float a0 = live ? wr[0] : 0.f, a1 = live ? wr[4] : 0.f;
        float n0 = live ? wr[c1] : 0.f, n1 = live ? wr[c1 + 4] : 0.f;
        float b0[4], b1[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) { b0[g] = xr[g * 16 * ldx]; b1[g] = xr[g * 16 * ldx + 4]; }
        for (int c = 0; c < ce; c += 8) {
          const int c2 = min(c + 16, ce - 8), cn = min(c + 8, ce - 8);
          const float m0 = live ? wr[c2] : 0.f, m1 = live ? wr[c2 + 4] : 0.f;
          float nb0[4], nb1[4];
#pragma unroll
          for (int g = 0; g < 4; ++g) { nb0[g] = xr[g * 16 * ldx + cn]; nb1[g] = xr[g * 16 * ldx + cn + 4]; }
#pragma unroll
          for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0[g], acc[g], 0, 0, 0);
#pragma unroll
          for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1[g], acc[g], 0, 0, 0);
          a0 = n0; a1 = n1; n0 = m0; n1 = m1;
#pragma unroll
          for (int g = 0; g < 4; ++g) { b0[g] = nb0[g]; b1[g] = nb1[g]; }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int k = rb * 16 + kq * 4 + j;
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const float z = acc[g][j];
            qs[g] = k < Kq ? fmaf(z, z, qs[g]) : qs[g];
            if (k >= Kq && k < Kq + T) tb[(k - Kq) * DET_TILE + g * 16 + col] = z;
          }
        }
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) qb[(wave * 4 + kq) * DET_TILE + g * 16 + col] = qs[g];
    }
    __syncthreads();
    // epilogue: thread (pixel t & 63, plane t >> 6) writes plane j < T of the scores, plane T is q
    {
      const int px = t & 63;
      const long long pix = tile * DET_TILE + px;
      if (pix < P) {
        float qv = qb[px];
        if (!IDENTITY) {
#pragma unroll 4
          for (int i = 1; i < DET_WAVES * 4; ++i) qv += qb[i * DET_TILE + px];
        }
        for (int j = wave; j <= T; j += DET_WAVES) {
          if (j < T) {
            float s = tb[j * DET_TILE + px];
            if (score & 1) s = qv == 0.f ? 0.f : s * rsqrtf(qv);
            if (score & 2) s = hpri_clamped_logit(s);
            scores[(long long)j * P + pix] = s;
          } else if (qout != nullptr) {
            qout[pix] = (!IDENTITY && (score & 2)) ? hpri_clamped_logit(qv / (qv + (float)Kq)) : qv;
          }
        }
      }
    }
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------
static inline size_t band_detect_lds(int cs) {
  return ((size_t)DET_TILE * band_tile_stride(cs) + (size_t)DET_WAVES * 4 * DET_TILE + (size_t)DET_MAX_T * DET_TILE) * 4;
}

extern "C" int hpri_band_detect_max_targets(void) { return DET_MAX_T; }

// cend: HOST array of one column extent per 16-row block of the Kq + T rows (NULL: cs).  The caller owns its truth: W lives on the
// device, so a table that cuts off a non-zero is not detected here -- the rows are then evaluated without those terms.
extern "C" int hpri_band_detect(const float* x, long long pixels, int cs, const float* weight, const float* bias, int ks, int Kq, int T,
                                const float* filters, const int* cend, int score, float* q, float* scores, hipStream_t stream) {
  HPRI_REQUIRE(x != nullptr, "band_detect: null pointer");
  HPRI_REQUIRE(pixels > 0 && Kq >= 0, "band_detect: bad sizes");
  HPRI_REQUIRE(band_cs_ok(cs), "band_detect: the channel stride must be a multiple of 8 up to hpri_band_max_cs");
  HPRI_REQUIRE(T >= 0 && T <= DET_MAX_T, "band_detect: T exceeds hpri_band_detect_max_targets");
  HPRI_REQUIRE(score >= 0 && score <= 3, "band_detect: score must be 0 (raw), 1 (cosine), 2 or 3 (their logits)");
  HPRI_REQUIRE((T > 0) == (scores != nullptr), "band_detect: the score planes come with the filter rows");
  HPRI_REQUIRE(q != nullptr || T > 0, "band_detect: nothing to write");
  const bool identity = weight == nullptr;
  DetExtents ext = {{0ull, 0ull, 0ull}};
  if (identity) {
    HPRI_REQUIRE(Kq == 0 && cend == nullptr, "band_detect: the identity metric (weight == NULL) has no quadratic rows and no extents");
    HPRI_REQUIRE((T > 0) == (filters != nullptr), "band_detect: the identity metric takes its T filter rows in `filters`");
    HPRI_REQUIRE(hpri_aligned16(x, filters) && (((uintptr_t)bias | (uintptr_t)q | (uintptr_t)scores) & 3) == 0, "band_detect: misaligned pointer");
  } else {
    HPRI_REQUIRE(bias != nullptr && filters == nullptr, "band_detect: a weight comes with its bias and without `filters`");
    HPRI_REQUIRE(Kq > 0 && Kq <= cs, "band_detect: Kq must lie in [1, cs]");
    HPRI_REQUIRE(ks > 0 && Kq + T <= ks, "band_detect: Kq + T does not fit ks");
    HPRI_REQUIRE(hpri_aligned16(x, weight, bias) && (((uintptr_t)q | (uintptr_t)scores) & 3) == 0, "band_detect: misaligned pointer");
    const int nrb = (Kq + T + 15) / 16;
    for (int rb = 0; rb < nrb; ++rb) {
      const int ce = cend != nullptr ? cend[rb] : cs;
      HPRI_REQUIRE(ce >= 8 && ce <= cs && ce % 8 == 0, "band_detect: a column extent must be a multiple of 8 in [8, cs]");
      ext.w[rb >> 3] |= (unsigned long long)(ce / 8) << (8 * (rb & 7));
    }
  }
  const size_t lds = band_detect_lds(cs);
  const long long tiles = (pixels + DET_TILE - 1) / DET_TILE;
  const dim3 grid = cache_grid(tiles, 2 * lds <= BAND_LDS_BYTES ? 2 : 1);
#define BAND_DETECT_LAUNCH(ID_, W_)                                                                                                \
  do {                                                                                                                             \
    hpri_ask_dynamic_lds(band_detect_kernel<ID_>, lds);                                                                            \
    hipLaunchKernelGGL(band_detect_kernel<ID_>, grid, dim3(DET_THREADS), lds, stream, x, pixels, cs / 4, W_, bias, ks, Kq, T, ext, \
                       score, q, scores);                                                                                          \
  } while (0)
  if (identity) BAND_DETECT_LAUNCH(true, filters);
  else BAND_DETECT_LAUNCH(false, weight);
#undef BAND_DETECT_LAUNCH
  HPRI_CHECK_LAUNCH();
  return HPRI_OK;
}
