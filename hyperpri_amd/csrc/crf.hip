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
#include "crf_common.h"

template <int K, int C>
__global__ __launch_bounds__(CRF_THREADS) void crf_iter_kernel(const CrfArgs g) {
  extern __shared__ __align__(16) float crf_lds[];
  const int r = g.r, lw = CRF_TILE_W + 2 * r, plane = lw * (CRF_TILE_H + 2 * r);
  const long long hw = (long long)g.H * g.W;
  const bool vec = g.flags & CRF_VEC, binary = g.flags & CRF_BINARY, potts = g.flags & CRF_POTTS, first = g.flags & CRF_FIRST,
             last = g.flags & CRF_LAST, prob = g.flags & CRF_PROB;
  float* __restrict__ mu = crf_lds + (K + C) * plane;            // C x C behind the planes: read from there, not held in registers
  if (!potts)
    for (int i = threadIdx.x; i < C * C; i += CRF_THREADS) mu[i] = g.mu_dev ? g.mu_dev[i] : g.mu[i];
  const float w_a = g.wa_dev ? *g.wa_dev : g.wa, w_s = g.ws_dev ? *g.ws_dev : g.ws;      // (the training entries: device memory)
  for (int item = blockIdx.x; item < g.items; item += gridDim.x) {
    const int txi = item % g.tiles_x;
    const int rest = item / g.tiles_x;
    const int tyi = rest % g.tiles_y, n = rest / g.tiles_y;
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
        if (in) hpri_load4(g.guide + (n * hw + px) * g.gs, K, vec, v);
#pragma unroll
        for (int a = 0; a < K; ++a) crf_lds[a * plane + idx] = v[a];
      }
      if (in) {
        if (first) {
          float U[C];
          crf_unary<C>(g.unary, binary, n, hw, px, U);
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
        const float war = w_a * g.ta[abs(dy)], wsr = w_s * g.tg[abs(dy)];
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
      crf_unary<C>(g.unary, binary, n, hw, px, U);
#pragma unroll
      for (int l = 0; l < C; ++l) M[l] = cnt > 1 ? M[l] / (float)(cnt - 1) : 0.f;
      if (potts) {
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
      if (last && !prob) {
        if (C == 2 && binary) {
          g.out[n * hw + px] = L[1] - L[0];
        } else {
#pragma unroll
          for (int l = 0; l < C; ++l) g.out[((long long)n * C + l) * hw + px] = L[l];
        }
      } else {
        float Q[C];
        crf_softmax<C>(L, Q);
        if (last && C == 2 && binary) {
          g.out[n * hw + px] = Q[1];
        } else {
          float* __restrict__ dst = last ? g.out : g.qout;
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

// The geometry, the tables and the launches the plain and the training forward share.  q[t] is where iteration t + 1 writes Q^(t+1)
// and where iteration t + 2 reads it.  The last iteration writes out; with keep_last it writes Q^T into q[T - 1] as every other does.
static int crf_run(CrfArgs& g, int K, int N, int C, int binary, int output, int radius, int iterations, const float* ta, const float* tg,
                   bool compat, float* const* q, bool keep_last, hipStream_t stream) {
  for (int d = 0; d <= radius; ++d) {
    g.ta[d] = ta[d];
    g.tg[d] = tg[d];
  }
  g.r = radius; g.tiles_x = hpri_cdiv(g.W, CRF_TILE_W); g.tiles_y = hpri_cdiv(g.H, CRF_TILE_H);
  g.items = (int)((long long)g.tiles_x * g.tiles_y * N);
  const int flags = (K > 0 && g.gs % 4 == 0 && hpri_aligned16(g.guide) ? CRF_VEC : 0) | (binary ? CRF_BINARY : 0) | (compat ? 0 : CRF_POTTS) |
                    (output ? CRF_PROB : 0);
  const size_t lds = crf_plane_lds(radius, K, C) + (compat ? (size_t)C * C * sizeof(float) : 0);
  const int blocks = hpri_grid_per_cu(g.items, 1, CRF_PER_CU);
  for (int t = 0; t < iterations; ++t) {
    g.flags = flags | (t == 0 ? CRF_FIRST : 0) | (t == iterations - 1 && !keep_last ? CRF_LAST : 0);
    g.qin = t == 0 ? nullptr : q[t - 1];
    g.qout = q[t];
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
  g.unary = unary; g.guide = guide; g.out = out; g.b = K > 0 ? b : 0.f; g.wa = w_a; g.ws = w_s;
  g.gs = gs; g.H = H; g.W = W;
  float* q[CRF_MAX_T];
  for (int t = 0; t < iterations; ++t) q[t] = t == iterations - 1 ? nullptr : (float*)workspace + (size_t)(t & 1) * N * C * H * W;
  return crf_run(g, K, N, C, binary, output, radius, iterations, ta, tg, compat != nullptr, q, false, stream);
}

// ---- the training forward: the same kernel, the weights from device memory, Q^1 .. Q^(T-1) (and Q^T under output prob) kept ---------
extern "C" size_t hpri_crf_train_workspace_bytes(int N, int C, int H, int W, int T) {
  if (!crf_frame_ok(N, C, H, W) || T < 1 || T > CRF_MAX_T) return 0;
  return crf_train_partials(N, C, H, W, T) * sizeof(double) + (size_t)(T + 2) * N * C * H * W * sizeof(float);
}

extern "C" int hpri_dense_crf_train_forward(const float* unary, int binary, const float* guide, int gs, int K, int N, int C, int H, int W,
                                            int radius, int iterations, const float* ta, const float* tg, float b, const float* w_a,
                                            const float* w_s, const float* compat, int output, int keep, void* workspace,
                                            size_t workspace_bytes, float* out, hipStream_t stream) {
  HPRI_REQUIRE(unary && ta && tg && out && w_s, "dense_crf_train_forward: null pointer");
  HPRI_REQUIRE(crf_frame_ok(N, C, H, W), "dense_crf_train_forward: bad sizes (N, H, W >= 1, C in [2, hpri_crf_max_classes])");
  HPRI_REQUIRE(binary == 0 || (binary == 1 && C == 2), "dense_crf_train_forward: binary must be 0, or 1 with C = 2");
  HPRI_REQUIRE(K >= 0 && K <= CRF_MAX_K, "dense_crf_train_forward: K must lie in [0, hpri_crf_max_guides]");
  HPRI_REQUIRE(K == 0 || (guide && gs >= K && w_a), "dense_crf_train_forward: a guide needs a pointer, a channel stride of at least K and w_a");
  HPRI_REQUIRE(radius >= 1 && radius <= CRF_MAX_R, "dense_crf_train_forward: the radius must lie in [1, hpri_crf_max_radius]");
  HPRI_REQUIRE(iterations >= 1 && iterations <= CRF_MAX_T, "dense_crf_train_forward: the iterations must lie in [1, hpri_crf_max_iterations]");
  HPRI_REQUIRE(crf_unit_table(ta, radius) && crf_unit_table(tg, radius),
               "dense_crf_train_forward: a spatial table must start at 1 and fall to no less than 0");
  HPRI_REQUIRE(K == 0 || (b > 0.f && b <= 3.0e38f), "dense_crf_train_forward: b must be positive and finite");
  HPRI_REQUIRE(output == 0 || output == 1, "dense_crf_train_forward: output must be 0 (logit) or 1 (prob)");
  HPRI_REQUIRE(keep == 0 || keep == 1, "dense_crf_train_forward: keep must be 0 or 1");
  HPRI_REQUIRE(keep ? (workspace && workspace_bytes >= hpri_crf_train_workspace_bytes(N, C, H, W, iterations))
                    : (iterations == 1 || (workspace && workspace_bytes >= hpri_crf_workspace_bytes(N, C, H, W))),
               "dense_crf_train_forward: the workspace is too small");
  HPRI_REQUIRE((((uintptr_t)unary | (uintptr_t)guide | (uintptr_t)out | (uintptr_t)w_a | (uintptr_t)w_s | (uintptr_t)compat) & 3) == 0 &&
                   ((uintptr_t)workspace & 7) == 0, "dense_crf_train_forward: misaligned pointer");
  CrfArgs g = {};
  g.unary = unary; g.guide = guide; g.out = out; g.b = K > 0 ? b : 0.f;
  g.wa_dev = K > 0 ? w_a : nullptr; g.wa = 0.f;                  // (no guide: no appearance kernel, w_a is not read)
  g.ws_dev = w_s; g.mu_dev = compat;
  g.gs = gs; g.H = H; g.W = W;
  const size_t set = (size_t)N * C * H * W;
  float* q[CRF_MAX_T];
  if (keep) {
    float* stack = (float*)((double*)workspace + crf_train_partials(N, C, H, W, iterations));
    for (int t = 0; t < iterations; ++t) q[t] = t == iterations - 1 && output == 0 ? nullptr : stack + (size_t)t * set;
  } else {
    for (int t = 0; t < iterations; ++t) q[t] = t == iterations - 1 ? nullptr : (float*)workspace + (size_t)(t & 1) * set;
  }
  // Under output prob the backward starts from Q^T (both planes of a binary input): the last iteration writes it into the stack as
  // every other does, and out is a copy of it (binary: of plane 1 of every image).
  const bool keep_last = keep && output == 1;
  const int rc = crf_run(g, K, N, C, binary, output, radius, iterations, ta, tg, compat != nullptr, q, keep_last, stream);
  if (rc != HPRI_OK || !keep_last) return rc;
  const float* qT = q[iterations - 1];
  const size_t hw = (size_t)H * W * sizeof(float);
  const hipError_t e = binary ? hipMemcpy2DAsync(out, hw, qT + (size_t)H * W, 2 * hw, hw, N, hipMemcpyDeviceToDevice, stream)
                              : hipMemcpyAsync(out, qT, set * sizeof(float), hipMemcpyDeviceToDevice, stream);
  if (e != hipSuccess) return hpri_set_error(HPRI_ERR_LAUNCH, hipGetErrorString(e));
  return HPRI_OK;
}
