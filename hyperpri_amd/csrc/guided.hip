// Guided filter (He, Sun and Tang) for score maps: hpri_guided_coeffs, hpri_guided_apply.
//
// A K-channel guide I (K <= 3, channels-last with channel stride gs) and T maps p_t on the same (N, H, W) frame, radius r <= 8.  The
// window of a pixel is the (2r+1)^2 square clipped to the image, n its in-image pixels.  include/hyperpri_hip.h states the contract:
//
//   stage 1 (guided_coeff_kernel<K>), per pixel k, centred on k itself so that no mean is subtracted from a moment:
//     dI_j = I_j - I_k, dp_j = p_j - p_k (fp32); S1 += dI, S2 = fmaf(dI_a, dI_b, S2), s += dp, Sp = fmaf(dI_a, dp, Sp) in fp32 from 0,
//     the window row by row (dy ascending, dx ascending inside a row), pixels outside the image skipped
//     fp64: m = S1/n, C = S2/n - m m^T, c = Sp/n - m (s/n), a = (C + eps Id)^-1 c (Cholesky; K = 1: one division)
//     fp32 planes: a (K), mI = I_k + m (K), mp = p_k + s/n
//   stage 2 (guided_apply_kernel<K>), per pixel i:
//     q = (1/n) sum over the window, the same order, of fmaf(a[K-1], I_i[K-1] - mI[K-1], ... fmaf(a[0], I_i[0] - mI[0], mp))
//
// A workgroup of 512 lanes owns a tile of 16 x 32 pixels, one lane a pixel; the tile plus a halo of r (guide and maps, or the 2K+1
// planes) lies in LDS, zeros where the image ends.  An out-of-image term is added as +0.0, which leaves a sum that started at +0.0
// bit for bit what skipping it leaves: the result of a pixel depends on its neighbourhood and its distance to the borders only, not
// on N, the grid or its place in a tile.  The maps of a launch go through stage 1 in groups of up to four (the sums of four fit the
// registers beside the guide's); a map's planes do not depend on its group.  No atomics.
#include "tail_helpers.h"

#define GF_TILE_H 16
#define GF_TILE_W 32
#define GF_THREADS (GF_TILE_H * GF_TILE_W)
#define GF_MAX_R 8
#define GF_MAX_K 3
#define GF_GROUP 4                           // maps of one pass through stage 1
#define GF_PER_CU 4                          // workgroups a CU is offered; the kernels stride over the rest

struct GfArgs {
  const float* guide;      // (N, H, W, gs)
  const float* maps;       // (N, T, H, W): stage 1 reads
  float* work;             // (N, T, 2K+1, H, W): a | mI | mp
  float* out;              // (N, T, H, W): stage 2 writes
  double eps;
  long long items;         // tiles x images x (groups | maps)
  int gs, vec, N, T, H, W, r, domain, tiles_x, tiles_y, groups;
};

// in-image pixels of the window of coordinate v on an axis of length L
__device__ __forceinline__ int gf_extent(int v, int r, int L) { return min(v + r, L - 1) - max(v - r, 0) + 1; }

// ---- stage 1: the window sums of one pixel and the solve, for TG maps ---------------------------------------------------------------
template <int K, int TG>
__device__ __forceinline__ void gf_coeff_pixel(const GfArgs& g, const float* __restrict__ lds, int plane, int lw, int n, int t0, int y,
                                               int x) {
  const int r = g.r;
  const int c0 = (threadIdx.x / GF_TILE_W + r) * lw + threadIdx.x % GF_TILE_W + r;
  float Ik[K], pk[TG], S1[K], S2[K][K], s[TG], Sp[TG][K];
#pragma unroll
  for (int a = 0; a < K; ++a) {
    Ik[a] = lds[a * plane + c0];
    S1[a] = 0.f;
#pragma unroll
    for (int b = a; b < K; ++b) S2[a][b] = 0.f;
  }
#pragma unroll
  for (int t = 0; t < TG; ++t) {
    pk[t] = lds[(K + t) * plane + c0];
    s[t] = 0.f;
#pragma unroll
    for (int a = 0; a < K; ++a) Sp[t][a] = 0.f;
  }
  for (int dy = -r; dy <= r; ++dy) {
    const bool vy = (unsigned)(y + dy) < (unsigned)g.H;
    for (int dx = -r; dx <= r; ++dx) {
      const bool v = vy && (unsigned)(x + dx) < (unsigned)g.W;
      const int o = c0 + dy * lw + dx;
      float dI[K];
#pragma unroll
      for (int a = 0; a < K; ++a) {
        dI[a] = v ? lds[a * plane + o] - Ik[a] : 0.f;
        S1[a] += dI[a];
      }
#pragma unroll
      for (int a = 0; a < K; ++a)
#pragma unroll
        for (int b = a; b < K; ++b) S2[a][b] = fmaf(dI[a], dI[b], S2[a][b]);
#pragma unroll
      for (int t = 0; t < TG; ++t) {
        const float dp = v ? lds[(K + t) * plane + o] - pk[t] : 0.f;
        s[t] += dp;
#pragma unroll
        for (int a = 0; a < K; ++a) Sp[t][a] = fmaf(dI[a], dp, Sp[t][a]);
      }
    }
  }
  if (y >= g.H || x >= g.W) return;
  {
#pragma clang fp contract(off)          // the solve is the reference's, operation by operation
    const double nd = (double)(gf_extent(y, r, g.H) * gf_extent(x, r, g.W));
    double m[K], L[K][K];
#pragma unroll
    for (int a = 0; a < K; ++a) m[a] = (double)S1[a] / nd;
    // the Cholesky factor of A = C + eps Id, column by column
#pragma unroll
    for (int j = 0; j < K; ++j) {
      double d = ((double)S2[j][j] / nd - m[j] * m[j]) + g.eps;
#pragma unroll
      for (int k = 0; k < j; ++k) d = d - L[j][k] * L[j][k];
      L[j][j] = K == 1 ? d : sqrt(d);
#pragma unroll
      for (int i = j + 1; i < K; ++i) {
        double e = (double)S2[j][i] / nd - m[i] * m[j];
#pragma unroll
        for (int k = 0; k < j; ++k) e = e - L[i][k] * L[j][k];
        L[i][j] = e / L[j][j];
      }
    }
    const long long hw = (long long)g.H * g.W;
#pragma unroll
    for (int t = 0; t < TG; ++t) {
      const double sn = (double)s[t] / nd;
      double z[K];
#pragma unroll
      for (int i = 0; i < K; ++i) {
        z[i] = (double)Sp[t][i] / nd - m[i] * sn;
        if (K > 1) {
#pragma unroll
          for (int k = 0; k < i; ++k) z[i] = z[i] - L[i][k] * z[k];
        }
        z[i] = z[i] / L[i][i];          // (K = 1: L[0][0] holds A itself: a = c / A, one division)
      }
      if (K > 1) {
#pragma unroll
        for (int i = K - 1; i >= 0; --i) {
#pragma unroll
          for (int k = i + 1; k < K; ++k) z[i] = z[i] - L[k][i] * z[k];
          z[i] = z[i] / L[i][i];
        }
      }
      float* w = g.work + ((long long)n * g.T + t0 + t) * (2 * K + 1) * hw + (long long)y * g.W + x;
#pragma unroll
      for (int a = 0; a < K; ++a) {
        w[a * hw] = (float)z[a];
        w[(K + a) * hw] = (float)((double)Ik[a] + m[a]);
      }
      w[2 * K * hw] = (float)((double)pk[t] + sn);
    }
  }
}

template <int K>
__global__ __launch_bounds__(GF_THREADS) void guided_coeff_kernel(const GfArgs g) {
  extern __shared__ __align__(16) float gf_lds[];
  const int r = g.r, lw = GF_TILE_W + 2 * r, plane = lw * (GF_TILE_H + 2 * r);
  for (long long item = blockIdx.x; item < g.items; item += gridDim.x) {
    const int txi = (int)(item % g.tiles_x);
    long long rest = item / g.tiles_x;
    const int tyi = (int)(rest % g.tiles_y);
    rest /= g.tiles_y;
    const int grp = (int)(rest % g.groups), n = (int)(rest / g.groups);
    const int t0 = grp * GF_GROUP, tg = min(GF_GROUP, g.T - t0);
    const int y0 = tyi * GF_TILE_H, x0 = txi * GF_TILE_W;
    for (int idx = threadIdx.x; idx < plane; idx += GF_THREADS) {
      const int ly = idx / lw, lx = idx - ly * lw;
      const int yy = y0 - r + ly, xx = x0 - r + lx;
      const bool in = (unsigned)yy < (unsigned)g.H && (unsigned)xx < (unsigned)g.W;
      const long long px = ((long long)n * g.H + yy) * g.W + xx;
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      if (in) hpri_load4(g.guide + px * g.gs, K, g.vec, v);
#pragma unroll
      for (int a = 0; a < K; ++a) gf_lds[a * plane + idx] = v[a];
#pragma unroll
      for (int t = 0; t < GF_GROUP; ++t) {
        if (t < tg) {
          float p = 0.f;
          if (in) {
            p = g.maps[(((long long)n * g.T + t0 + t) * g.H + yy) * g.W + xx];
            if (g.domain) {
              float sn;
              hpri_sigmoids(p, p, sn);
            }
          }
          gf_lds[(K + t) * plane + idx] = p;
        }
      }
    }
    __syncthreads();
    const int y = y0 + threadIdx.x / GF_TILE_W, x = x0 + threadIdx.x % GF_TILE_W;
    switch (tg) {
      case 1: gf_coeff_pixel<K, 1>(g, gf_lds, plane, lw, n, t0, y, x); break;
      case 2: gf_coeff_pixel<K, 2>(g, gf_lds, plane, lw, n, t0, y, x); break;
      case 3: gf_coeff_pixel<K, 3>(g, gf_lds, plane, lw, n, t0, y, x); break;
      default: gf_coeff_pixel<K, 4>(g, gf_lds, plane, lw, n, t0, y, x); break;
    }
    __syncthreads();
  }
}

// ---- stage 2: the mean over the window of the neighbours' lines, evaluated at the centre's guide ------------------------------------
template <int K>
__global__ __launch_bounds__(GF_THREADS) void guided_apply_kernel(const GfArgs g) {
  extern __shared__ __align__(16) float gf_lds[];
  const int r = g.r, lw = GF_TILE_W + 2 * r, plane = lw * (GF_TILE_H + 2 * r);
  const long long hw = (long long)g.H * g.W;
  for (long long item = blockIdx.x; item < g.items; item += gridDim.x) {
    const int txi = (int)(item % g.tiles_x);
    long long rest = item / g.tiles_x;
    const int tyi = (int)(rest % g.tiles_y);
    rest /= g.tiles_y;                                           // rest = n * T + t
    const int n = (int)(rest / g.T);
    const int y0 = tyi * GF_TILE_H, x0 = txi * GF_TILE_W;
    const float* __restrict__ w = g.work + rest * (2 * K + 1) * hw;
    for (int idx = threadIdx.x; idx < plane; idx += GF_THREADS) {
      const int ly = idx / lw, lx = idx - ly * lw;
      const int yy = y0 - r + ly, xx = x0 - r + lx;
      const bool in = (unsigned)yy < (unsigned)g.H && (unsigned)xx < (unsigned)g.W;
      const long long px = (long long)yy * g.W + xx;
#pragma unroll
      for (int c = 0; c < 2 * K + 1; ++c) gf_lds[c * plane + idx] = in ? w[c * hw + px] : 0.f;
    }
    __syncthreads();
    const int y = y0 + threadIdx.x / GF_TILE_W, x = x0 + threadIdx.x % GF_TILE_W;
    if (y < g.H && x < g.W) {
      float Ii[4] = {0.f, 0.f, 0.f, 0.f};
      hpri_load4(g.guide + (((long long)n * g.H + y) * g.W + x) * g.gs, K, g.vec, Ii);
      const int c0 = (threadIdx.x / GF_TILE_W + r) * lw + threadIdx.x % GF_TILE_W + r;
      float acc = 0.f;
      for (int dy = -r; dy <= r; ++dy) {
        const bool vy = (unsigned)(y + dy) < (unsigned)g.H;
        for (int dx = -r; dx <= r; ++dx) {
          const bool v = vy && (unsigned)(x + dx) < (unsigned)g.W;
          const int o = c0 + dy * lw + dx;
          float t = gf_lds[2 * K * plane + o];
#pragma unroll
          for (int a = 0; a < K; ++a) t = fmaf(gf_lds[a * plane + o], Ii[a] - gf_lds[(K + a) * plane + o], t);
          acc += v ? t : 0.f;
        }
      }
      const float q = acc / (float)(gf_extent(y, r, g.H) * gf_extent(x, r, g.W));
      g.out[rest * hw + (long long)y * g.W + x] = g.domain ? hpri_clamped_logit(q) : q;
    }
    __syncthreads();
  }
}

// ---- host --------------------------------------------------------------------------------------------------------------------------
extern "C" int hpri_guided_max_radius(void) { return GF_MAX_R; }
extern "C" int hpri_guided_max_guides(void) { return GF_MAX_K; }
extern "C" int hpri_guided_tile_h(void) { return GF_TILE_H; }
extern "C" int hpri_guided_tile_w(void) { return GF_TILE_W; }

static inline bool gf_frame_ok(int N, int T, int H, int W, int K) {
  return N > 0 && T > 0 && H > 0 && W > 0 && K >= 1 && K <= GF_MAX_K && (long long)H * W < (1LL << 31) &&
         (long long)N * T < (1LL << 31) && (long long)N * T * H * W < (1LL << 40);
}

extern "C" size_t hpri_guided_workspace_bytes(int N, int T, int H, int W, int K) {
  if (!gf_frame_ok(N, T, H, W, K)) return 0;
  return (size_t)N * T * (2 * K + 1) * H * W * sizeof(float);
}

static inline size_t gf_lds_bytes(int r, int planes) {
  return (size_t)(GF_TILE_W + 2 * r) * (GF_TILE_H + 2 * r) * planes * sizeof(float);
}

#define GF_COMMON_CHECKS(who)                                                                                                       \
  HPRI_REQUIRE(gf_frame_ok(N, T, H, W, K), who ": bad sizes (N, T, H, W >= 1, K in [1, hpri_guided_max_guides])");                  \
  HPRI_REQUIRE(gs >= K, who ": the guide's channel stride must be at least K");                                                     \
  HPRI_REQUIRE(radius >= 1 && radius <= GF_MAX_R, who ": the radius must lie in [1, hpri_guided_max_radius]");                      \
  HPRI_REQUIRE(domain == 0 || domain == 1, who ": domain must be 0 (linear) or 1 (prob)");                                          \
  HPRI_REQUIRE(workspace_bytes >= hpri_guided_workspace_bytes(N, T, H, W, K), who ": the workspace is too small")

#define GF_LAUNCH(kernel_, lds_, args_)                                                                                            \
  do {                                                                                                                             \
    const int blocks = hpri_grid_per_cu((args_).items, 1, GF_PER_CU);                                                              \
    switch (K) {                                                                                                                   \
      case 1: hipLaunchKernelGGL(kernel_<1>, dim3(blocks), dim3(GF_THREADS), lds_, stream, args_); break;                          \
      case 2: hipLaunchKernelGGL(kernel_<2>, dim3(blocks), dim3(GF_THREADS), lds_, stream, args_); break;                          \
      default: hipLaunchKernelGGL(kernel_<3>, dim3(blocks), dim3(GF_THREADS), lds_, stream, args_); break;                         \
    }                                                                                                                              \
  } while (0)

extern "C" int hpri_guided_coeffs(const float* guide, int gs, int K, const float* maps, int N, int T, int H, int W, int radius,
                                  float eps, int domain, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  HPRI_REQUIRE(guide && maps && workspace, "guided_coeffs: null pointer");
  GF_COMMON_CHECKS("guided_coeffs");
  HPRI_REQUIRE(eps > 0.f && eps <= 3.0e38f, "guided_coeffs: eps must be positive and finite");
  HPRI_REQUIRE((((uintptr_t)guide | (uintptr_t)maps | (uintptr_t)workspace) & 3) == 0, "guided_coeffs: misaligned pointer");
  GfArgs g = {};
  g.guide = guide; g.maps = maps; g.work = (float*)workspace; g.out = nullptr; g.eps = (double)eps;
  g.gs = gs; g.vec = gs % 4 == 0 && hpri_aligned16(guide); g.N = N; g.T = T; g.H = H; g.W = W; g.r = radius; g.domain = domain;
  g.tiles_x = hpri_cdiv(W, GF_TILE_W); g.tiles_y = hpri_cdiv(H, GF_TILE_H); g.groups = hpri_cdiv(T, GF_GROUP);
  g.items = (long long)g.tiles_x * g.tiles_y * g.groups * N;
  const size_t lds = gf_lds_bytes(radius, K + GF_GROUP);
  GF_LAUNCH(guided_coeff_kernel, lds, g);
  HPRI_CHECK_LAUNCH();
  return HPRI_OK;
}

extern "C" int hpri_guided_apply(const float* guide, int gs, int K, int N, int T, int H, int W, int radius, int domain,
                                 const void* workspace, size_t workspace_bytes, float* out, hipStream_t stream) {
  HPRI_REQUIRE(guide && workspace && out, "guided_apply: null pointer");
  GF_COMMON_CHECKS("guided_apply");
  HPRI_REQUIRE((((uintptr_t)guide | (uintptr_t)out | (uintptr_t)workspace) & 3) == 0, "guided_apply: misaligned pointer");
  GfArgs g = {};
  g.guide = guide; g.maps = nullptr; g.work = (float*)workspace; g.out = out; g.eps = 0.0;
  g.gs = gs; g.vec = gs % 4 == 0 && hpri_aligned16(guide); g.N = N; g.T = T; g.H = H; g.W = W; g.r = radius; g.domain = domain;
  g.tiles_x = hpri_cdiv(W, GF_TILE_W); g.tiles_y = hpri_cdiv(H, GF_TILE_H); g.groups = 1;
  g.items = (long long)g.tiles_x * g.tiles_y * N * T;
  const size_t lds = gf_lds_bytes(radius, 2 * K + 1);
  GF_LAUNCH(guided_apply_kernel, lds, g);
  HPRI_CHECK_LAUNCH();
  return HPRI_OK;
}
