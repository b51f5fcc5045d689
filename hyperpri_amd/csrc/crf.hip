// Dense CRF restricted to a window (Teichmann and Cipolla's convolutional CRF; Kraehenbuehl and Koltun's fully connected CRF inside a
// (2r+1)^2 window, exact there): hpri_dense_crf, mean-field refinement of score maps.
//
// Unaries U (N, C, H, W) -- or binary logits z (N, H, W), defined as the two-class problem U = (0, z) --, a K-channel guide I (K <= 3,
// channels-last with channel stride gs, K = 0: none), radius r <= 8, T <= 16 iterations.  include/hyperpri_hip.h states the contract:
//
//   Q^0 = softmax(U);  per iteration and pixel i, fp32, the window row by row (dy ascending, dx ascending inside a row), the centre
//   skipped, a neighbour outside the image adding +0.0:
//     s = fmaf(dI_c, dI_c, s) over the guide's channels, dI_c = I_j,c - I_i,c;  e = expf(-(s * b));  k = fmaf(ga, e, gs_) with
//     ga = (w_a ta[|dy|]) ta[|dx|], gs_ = (w_s tg[|dy|]) tg[|dx|];  M_l = fmaf(k, Q_j(l), M_l)
//   m_l = M_l / (float)(n - 1) (n the clipped window's pixels; n = 1: m = 0);  L_l = U_l - sum_l' mu(l, l') m_l' (Potts: U_l + m_l);
//   Q^t = softmax(L)
//
// A workgroup of 512 lanes owns a tile of 16 x 32 pixels, one lane a pixel; the tile plus a halo of r -- the guide and the C planes of
// Q^(t-1), zeros where the image ends -- lies in LDS (r = 8, K = 3, C = 8: 66 KB, two workgroups a CU).  One launch per iteration over
// ping-pong Q planes; the first launch forms softmax(U) while it fills LDS, the last one writes the output instead of Q.  The kernel
// weights k are recomputed every iteration; the spatial tables, mu and the scalars travel in the kernel's arguments (a workgroup copies
// a given mu behind its planes in LDS once, so that the C^2 values occupy no registers).  A pixel's M_l sits in registers for all C
// classes at once: no class grouping, no atomics.
#include "tail_helpers.h"

#define CRF_TILE_H 16
#define CRF_TILE_W 32
#define CRF_THREADS (CRF_TILE_H * CRF_TILE_W)
#define CRF_MAX_R 8
#define CRF_MAX_K 3
#define CRF_MAX_C 8
#define CRF_MAX_T 16
#define CRF_PER_CU 2                         // workgroups a CU is offered (what its LDS holds at r = 8); the kernel strides over the rest

struct CrfArgs {
  const float* unary;      // (N, C, H, W), or (N, H, W) with binary
  const float* guide;      // (N, H, W, gs)
  const float* qin;        // (N, C, H, W): Q^(t-1); not read by the first launch
  float* qout;             // (N, C, H, W): Q^t; not written by the last launch
  float* out;              // the last launch writes
  long long items;         // tiles x images
  float ta[CRF_MAX_R + 1], tg[CRF_MAX_R + 1];
  float mu[CRF_MAX_C * CRF_MAX_C];
  float b, wa, ws;
  int gs, vec, N, H, W, r, tiles_x, tiles_y, binary, potts, first, last, output;
};

// in-image pixels of the window of coordinate v on an axis of length L
__device__ __forceinline__ int crf_extent(int v, int r, int L) { return min(v + r, L - 1) - max(v - r, 0) + 1; }

// e_l = expf(L_l - max L), summed in class order, one division per class
template <int C>
__device__ __forceinline__ void crf_softmax(const float (&L)[C], float (&Q)[C]) {
  float mx = L[0];
#pragma unroll
  for (int l = 1; l < C; ++l) mx = fmaxf(mx, L[l]);
  float sum = 0.f;
#pragma unroll
  for (int l = 0; l < C; ++l) {
    Q[l] = expf(L[l] - mx);
    sum += Q[l];
  }
#pragma unroll
  for (int l = 0; l < C; ++l) Q[l] = Q[l] / sum;
}

template <int C>
__device__ __forceinline__ void crf_unary(const CrfArgs& g, int n, long long hw, long long px, float (&U)[C]) {
  if (C == 2 && g.binary) {
    U[0] = 0.f;
    U[1] = g.unary[n * hw + px];
  } else {
#pragma unroll
    for (int l = 0; l < C; ++l) U[l] = g.unary[((long long)n * C + l) * hw + px];
  }
}

template <int K, int C>
__global__ __launch_bounds__(CRF_THREADS) void crf_iter_kernel(const CrfArgs g) {
  extern __shared__ __align__(16) float crf_lds[];
  const int r = g.r, lw = CRF_TILE_W + 2 * r, plane = lw * (CRF_TILE_H + 2 * r);
  const long long hw = (long long)g.H * g.W;
  float* __restrict__ mu = crf_lds + (K + C) * plane;            // C x C behind the planes: read from there, not held in registers
  if (!g.potts)
    for (int i = threadIdx.x; i < C * C; i += CRF_THREADS) mu[i] = g.mu[i];
  for (long long item = blockIdx.x; item < g.items; item += gridDim.x) {
    const int txi = (int)(item % g.tiles_x);
    const long long rest = item / g.tiles_x;
    const int tyi = (int)(rest % g.tiles_y), n = (int)(rest / g.tiles_y);
    const int y0 = tyi * CRF_TILE_H, x0 = txi * CRF_TILE_W;
    for (int idx = threadIdx.x; idx < plane; idx += CRF_THREADS) {
      const int ly = idx / lw, lx = idx - ly * lw;
      const int yy = y0 - r + ly, xx = x0 - r + lx;
      const bool in = (unsigned)yy < (unsigned)g.H && (unsigned)xx < (unsigned)g.W;
      const long long px = (long long)yy * g.W + xx;
      float Q[C];
#pragma unroll
      for (int l = 0; l < C; ++l) Q[l] = 0.f;
      if (K > 0) {
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (in) hpri_load4(g.guide + (n * hw + px) * g.gs, K, g.vec, v);
#pragma unroll
        for (int a = 0; a < K; ++a) crf_lds[a * plane + idx] = v[a];
      }
      if (in) {
        if (g.first) {
          float U[C];
          crf_unary<C>(g, n, hw, px, U);
          crf_softmax<C>(U, Q);
        } else {
#pragma unroll
          for (int l = 0; l < C; ++l) Q[l] = g.qin[((long long)n * C + l) * hw + px];
        }
      }
#pragma unroll
      for (int l = 0; l < C; ++l) crf_lds[(K + l) * plane + idx] = Q[l];
    }
    __syncthreads();
    const int y = y0 + threadIdx.x / CRF_TILE_W, x = x0 + threadIdx.x % CRF_TILE_W;
    if (y < g.H && x < g.W) {
      const int c0 = (threadIdx.x / CRF_TILE_W + r) * lw + threadIdx.x % CRF_TILE_W + r;
      float Ii[K > 0 ? K : 1], M[C];
#pragma unroll
      for (int a = 0; a < K; ++a) Ii[a] = crf_lds[a * plane + c0];
#pragma unroll
      for (int l = 0; l < C; ++l) M[l] = 0.f;
      for (int dy = -r; dy <= r; ++dy) {
        const float war = g.wa * g.ta[abs(dy)], wsr = g.ws * g.tg[abs(dy)];
        for (int dx = -r; dx <= r; ++dx) {
          if (dy == 0 && dx == 0) continue;
          const float ga = war * g.ta[abs(dx)], gs_ = wsr * g.tg[abs(dx)];
          const int o = c0 + dy * lw + dx;
          float s = 0.f;
#pragma unroll
          for (int a = 0; a < K; ++a) {
            const float d = crf_lds[a * plane + o] - Ii[a];
            s = fmaf(d, d, s);
          }
          const float e = K > 0 ? expf(-(s * g.b)) : 1.f;       // (no guide: s = 0 and expf(-0) = 1)
          const float k = fmaf(ga, e, gs_);
#pragma unroll
          for (int l = 0; l < C; ++l) M[l] = fmaf(k, crf_lds[(K + l) * plane + o], M[l]);
        }
      }
      const int cnt = crf_extent(y, r, g.H) * crf_extent(x, r, g.W);
      const long long px = (long long)y * g.W + x;
      float U[C], L[C];
      crf_unary<C>(g, n, hw, px, U);
#pragma unroll
      for (int l = 0; l < C; ++l) M[l] = cnt > 1 ? M[l] / (float)(cnt - 1) : 0.f;
      if (g.potts) {
#pragma unroll
        for (int l = 0; l < C; ++l) L[l] = U[l] + M[l];
      } else {
#pragma unroll
        for (int l = 0; l < C; ++l) {
          float p = 0.f;
#pragma unroll
          for (int k = 0; k < C; ++k) p = fmaf(mu[l * C + k], M[k], p);
          L[l] = U[l] - p;
        }
      }
      if (g.last && g.output == 0) {
        if (C == 2 && g.binary) {
          g.out[n * hw + px] = L[1] - L[0];
        } else {
#pragma unroll
          for (int l = 0; l < C; ++l) g.out[((long long)n * C + l) * hw + px] = L[l];
        }
      } else {
        float Q[C];
        crf_softmax<C>(L, Q);
        if (g.last && C == 2 && g.binary) {
          g.out[n * hw + px] = Q[1];
        } else {
          float* __restrict__ dst = g.last ? g.out : g.qout;
#pragma unroll
          for (int l = 0; l < C; ++l) dst[((long long)n * C + l) * hw + px] = Q[l];
        }
      }
    }
    __syncthreads();
  }
}

// ---- host --------------------------------------------------------------------------------------------------------------------------
extern "C" int hpri_crf_max_radius(void) { return CRF_MAX_R; }
extern "C" int hpri_crf_max_classes(void) { return CRF_MAX_C; }
extern "C" int hpri_crf_max_guides(void) { return CRF_MAX_K; }
extern "C" int hpri_crf_max_iterations(void) { return CRF_MAX_T; }
extern "C" int hpri_crf_tile_h(void) { return CRF_TILE_H; }
extern "C" int hpri_crf_tile_w(void) { return CRF_TILE_W; }

static inline bool crf_frame_ok(int N, int C, int H, int W) {
  return N > 0 && C >= 2 && C <= CRF_MAX_C && H > 0 && W > 0 && (long long)H * W < (1LL << 31) && (long long)N * C < (1LL << 31) &&
         (long long)N * C * H * W < (1LL << 40);
}

extern "C" size_t hpri_crf_workspace_bytes(int N, int C, int H, int W) {
  if (!crf_frame_ok(N, C, H, W)) return 0;
  return (size_t)2 * N * C * H * W * sizeof(float);
}

template <int K, int C>
static inline void crf_launch(const CrfArgs& g, int blocks, size_t lds, hipStream_t stream) {
  hpri_ask_dynamic_lds(crf_iter_kernel<K, C>, lds);
  hipLaunchKernelGGL((crf_iter_kernel<K, C>), dim3(blocks), dim3(CRF_THREADS), lds, stream, g);
}

template <int K>
static inline void crf_launch_classes(const CrfArgs& g, int C, int blocks, size_t lds, hipStream_t stream) {
  switch (C) {
    case 2: crf_launch<K, 2>(g, blocks, lds, stream); break;
    case 3: crf_launch<K, 3>(g, blocks, lds, stream); break;
    case 4: crf_launch<K, 4>(g, blocks, lds, stream); break;
    case 5: crf_launch<K, 5>(g, blocks, lds, stream); break;
    case 6: crf_launch<K, 6>(g, blocks, lds, stream); break;
    case 7: crf_launch<K, 7>(g, blocks, lds, stream); break;
    default: crf_launch<K, 8>(g, blocks, lds, stream); break;
  }
}

static inline bool crf_unit_table(const float* t, int r) {      // exp(-d^2 / (2 theta^2)): 1 at d = 0, in [0, 1] and not increasing
  if (t[0] != 1.f) return false;
  for (int d = 1; d <= r; ++d)
    if (!(t[d] >= 0.f && t[d] <= t[d - 1])) return false;
  return true;
}

extern "C" int hpri_dense_crf(const float* unary, int binary, const float* guide, int gs, int K, int N, int C, int H, int W, int radius,
                              int iterations, const float* ta, const float* tg, float b, float w_a, float w_s, const float* compat,
                              int output, void* workspace, size_t workspace_bytes, float* out, hipStream_t stream) {
  HPRI_REQUIRE(unary && ta && tg && out, "dense_crf: null pointer");
  HPRI_REQUIRE(crf_frame_ok(N, C, H, W), "dense_crf: bad sizes (N, H, W >= 1, C in [2, hpri_crf_max_classes])");
  HPRI_REQUIRE(binary == 0 || (binary == 1 && C == 2), "dense_crf: binary must be 0, or 1 with C = 2");
  HPRI_REQUIRE(K >= 0 && K <= CRF_MAX_K, "dense_crf: K must lie in [0, hpri_crf_max_guides]");
  HPRI_REQUIRE(K == 0 || (guide && gs >= K), "dense_crf: a guide needs a pointer and a channel stride of at least K");
  HPRI_REQUIRE(radius >= 1 && radius <= CRF_MAX_R, "dense_crf: the radius must lie in [1, hpri_crf_max_radius]");
  HPRI_REQUIRE(iterations >= 1 && iterations <= CRF_MAX_T, "dense_crf: the iterations must lie in [1, hpri_crf_max_iterations]");
  HPRI_REQUIRE(crf_unit_table(ta, radius) && crf_unit_table(tg, radius), "dense_crf: a spatial table must start at 1 and fall to no less than 0");
  HPRI_REQUIRE(w_a >= 0.f && w_a <= 3.0e38f && w_s >= 0.f && w_s <= 3.0e38f, "dense_crf: the weights must be non-negative and finite");
  HPRI_REQUIRE(K > 0 ? (b > 0.f && b <= 3.0e38f) : w_a == 0.f, "dense_crf: b must be positive and finite; without a guide w_a must be 0");
  HPRI_REQUIRE(output == 0 || output == 1, "dense_crf: output must be 0 (logit) or 1 (prob)");
  HPRI_REQUIRE(iterations == 1 || (workspace && workspace_bytes >= hpri_crf_workspace_bytes(N, C, H, W)), "dense_crf: the workspace is too small");
  HPRI_REQUIRE((((uintptr_t)unary | (uintptr_t)guide | (uintptr_t)out | (uintptr_t)workspace) & 3) == 0, "dense_crf: misaligned pointer");
  CrfArgs g = {};
  if (compat) {
    for (int i = 0; i < C * C; ++i) {
      HPRI_REQUIRE(compat[i] >= -3.0e38f && compat[i] <= 3.0e38f, "dense_crf: the compatibility matrix must be finite");
      g.mu[i] = compat[i];
    }
  }
  for (int d = 0; d <= radius; ++d) {
    g.ta[d] = ta[d];
    g.tg[d] = tg[d];
  }
  g.unary = unary; g.guide = guide; g.out = out; g.b = K > 0 ? b : 0.f; g.wa = w_a; g.ws = w_s;
  g.gs = gs; g.vec = K > 0 && gs % 4 == 0 && hpri_aligned16(guide); g.N = N; g.H = H; g.W = W; g.r = radius;
  g.tiles_x = hpri_cdiv(W, CRF_TILE_W); g.tiles_y = hpri_cdiv(H, CRF_TILE_H); g.binary = binary; g.potts = compat == nullptr;
  g.output = output; g.items = (long long)g.tiles_x * g.tiles_y * N;
  const size_t lds = (size_t)(CRF_TILE_W + 2 * radius) * (CRF_TILE_H + 2 * radius) * (K + C) * sizeof(float) +
                     (compat ? (size_t)C * C * sizeof(float) : 0);
  const int blocks = hpri_grid_per_cu(g.items, 1, CRF_PER_CU);
  float* q[2] = {(float*)workspace, (float*)workspace + (size_t)N * C * H * W};
  for (int t = 0; t < iterations; ++t) {
    g.first = t == 0; g.last = t == iterations - 1;
    g.qin = g.first ? nullptr : q[(t - 1) & 1];
    g.qout = g.last ? nullptr : q[t & 1];
    switch (K) {
      case 0: crf_launch_classes<0>(g, C, blocks, lds, stream); break;
      case 1: crf_launch_classes<1>(g, C, blocks, lds, stream); break;
      case 2: crf_launch_classes<2>(g, C, blocks, lds, stream); break;
      default: crf_launch_classes<3>(g, C, blocks, lds, stream); break;
    }
    HPRI_CHECK_LAUNCH();
  }
  return HPRI_OK;
}
