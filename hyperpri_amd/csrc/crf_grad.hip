// The backward of the dense CRF (crf.hip): hpri_dense_crf_backward, the adjoint of the T mean-field iterations for the unaries, the two
// kernel weights and the compatibility matrix.  include/hyperpri_hip.h states the contract and its fp32 order.  The pairwise weights are
// symmetric bit for bit, so the adjoint of the message passing is a gather over the forward's window: no atomics, no scatter, the
// forward's tile and halo.  LDS holds the guide's K planes and the C planes of b = gL / (n - 1) behind 8 KB for the block sums; one
// launch per iteration over two ping-pong copies of gL; the parameter gradients are fp32 per pixel, fp64 per tile and iteration
// (hpri_block_sum), and one block adds the partial sums in a fixed order (crf_grad_finish_kernel).
#include "crf_common.h"

struct CrfBackArgs {
  const float* qsrc;       // Q^(t-1) (N, C, H, W); at t = 1 the unaries ((N, H, W) with binary), from which Q^0 is formed again
  const float* guide;      // (N, H, W, gs)
  const float* gl_in;      // (N, C, H, W): gL^t
  float* gl_out;           // (N, C, H, W): gL^(t-1); NULL at t = 1
  float* gu;               // (N, C, H, W), or (N, H, W) with binary: written at t = T, accumulated after
  double* partials;        // this iteration's (items, 2 + C^2) sums
  const float* wa_dev;
  const float* ws_dev;
  const float* mu_dev;     // NULL: Potts
  float ta[CRF_MAX_R + 1], tg[CRF_MAX_R + 1];
  float b;
  int items;               // tiles x images
  int gs, H, W, r, tiles_x, tiles_y;
  int flags;               // CRF_VEC, CRF_BINARY, CRF_FIRST (t = T), CRF_LAST (t = 1), CRF_WANT_MU
};
#define CRF_WANT_MU 64

#define CRF_RED_DOUBLES (2 * CRF_THREADS)    // the block sums' scratch in front of the planes

template <int K, int C>
__global__ __launch_bounds__(CRF_THREADS) void crf_back_kernel(const CrfBackArgs g) {
  extern __shared__ __align__(16) double crf_back_lds[];
  double (*red)[CRF_THREADS] = reinterpret_cast<double (*)[CRF_THREADS]>(crf_back_lds);
  float* __restrict__ lds = reinterpret_cast<float*>(crf_back_lds + CRF_RED_DOUBLES);
  const int r = g.r, lw = CRF_TILE_W + 2 * r, plane = lw * (CRF_TILE_H + 2 * r);
  const long long hw = (long long)g.H * g.W;
  constexpr int R = 2 + C * C;
  const bool vec = g.flags & CRF_VEC, binary = g.flags & CRF_BINARY, first = g.flags & CRF_FIRST, last = g.flags & CRF_LAST;
  const bool potts = g.mu_dev == nullptr;
  float* __restrict__ mu = lds + (K + C) * plane;
  if (!potts)
    for (int i = threadIdx.x; i < C * C; i += CRF_THREADS) mu[i] = g.mu_dev[i];
  const float w_a = K > 0 ? *g.wa_dev : 0.f, w_s = *g.ws_dev;
  {                                                              // one tile a workgroup: nothing of the block sums stays alive
    const int item = blockIdx.x;                                 // across a loop over tiles, in scalar registers
    const int txi = item % g.tiles_x;
    const int rest = item / g.tiles_x;
    const int tyi = rest % g.tiles_y, n = rest / g.tiles_y;
    const int y0 = tyi * CRF_TILE_H, x0 = txi * CRF_TILE_W;
    for (int idx = threadIdx.x; idx < plane; idx += CRF_THREADS) {
      const int ly = idx / lw, lx = idx - ly * lw;
      const int yy = y0 - r + ly, xx = x0 - r + lx;
      const bool in = (unsigned)yy < (unsigned)g.H && (unsigned)xx < (unsigned)g.W;
      const long long px = (long long)yy * g.W + xx;
      if (K > 0) {
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (in) hpri_load4(g.guide + (n * hw + px) * g.gs, K, vec, v);
#pragma unroll
        for (int a = 0; a < K; ++a) lds[a * plane + idx] = v[a];
      }
      const int cnt = in ? crf_extent(yy, r, g.H) * crf_extent(xx, r, g.W) : 1;
#pragma unroll
      for (int l = 0; l < C; ++l)
        lds[(K + l) * plane + idx] = cnt > 1 ? g.gl_in[((long long)n * C + l) * hw + px] / (float)(cnt - 1) : 0.f;
    }
    __syncthreads();
    const int y = y0 + threadIdx.x / CRF_TILE_W, x = x0 + threadIdx.x % CRF_TILE_W;
    float H[C], Q[C];
    double s2[2] = {0.0, 0.0};
#pragma unroll
    for (int l = 0; l < C; ++l) H[l] = Q[l] = 0.f;
    if (y < g.H && x < g.W) {
      const int c0 = (threadIdx.x / CRF_TILE_W + r) * lw + threadIdx.x % CRF_TILE_W + r;
      float Ii[K > 0 ? K : 1], GA[K > 0 ? C : 1], GS[C];
#pragma unroll
      for (int a = 0; a < K; ++a) Ii[a] = lds[a * plane + c0];
#pragma unroll
      for (int l = 0; l < C; ++l) GS[l] = 0.f;
      if (K > 0) {
#pragma unroll
        for (int l = 0; l < C; ++l) GA[l] = 0.f;
      }
      for (int dy = -r; dy <= r; ++dy) {
        const float tay = g.ta[abs(dy)], tgy = g.tg[abs(dy)];
        for (int dx = -r; dx <= r; ++dx) {
          if (dy == 0 && dx == 0) continue;
          const float ps = tgy * g.tg[abs(dx)];
          const int o = c0 + dy * lw + dx;
          float ka = 0.f;
          if (K > 0) {
            float s = 0.f;
#pragma unroll
            for (int a = 0; a < K; ++a) {
              const float d = lds[a * plane + o] - Ii[a];
              s = fmaf(d, d, s);
            }
            ka = (tay * g.ta[abs(dx)]) * expf(-(s * g.b));
          }
#pragma unroll
          for (int l = 0; l < C; ++l) {
            const float bl = lds[(K + l) * plane + o];
            if (K > 0) GA[l] = fmaf(ka, bl, GA[l]);
            GS[l] = fmaf(ps, bl, GS[l]);
          }
        }
      }
      const long long px = (long long)y * g.W + x;
      if (last) {
        float U[C];
        crf_unary<C>(g.qsrc, binary, n, hw, px, U);
        crf_softmax<C>(U, Q);
      } else {
#pragma unroll
        for (int l = 0; l < C; ++l) Q[l] = g.qsrc[((long long)n * C + l) * hw + px];
      }
#pragma unroll
      for (int l = 0; l < C; ++l) H[l] = K > 0 ? fmaf(w_a, GA[l], w_s * GS[l]) : w_s * GS[l];
      float gQ[C], pwa = 0.f, pws = 0.f;
      if (potts) {
#pragma unroll
        for (int k = 0; k < C; ++k) {
          gQ[k] = H[k];
          if (K > 0) pwa = fmaf(GA[k], Q[k], pwa);
          pws = fmaf(GS[k], Q[k], pws);
        }
      } else {
#pragma unroll
        for (int k = 0; k < C; ++k) {
          float p = 0.f, pa = 0.f, pg = 0.f;
#pragma unroll
          for (int l = 0; l < C; ++l) {
            const float m = mu[l * C + k];
            p = fmaf(m, H[l], p);
            if (K > 0) pa = fmaf(m, GA[l], pa);
            pg = fmaf(m, GS[l], pg);
          }
          gQ[k] = -p;
          if (K > 0) pwa = fmaf(-pa, Q[k], pwa);
          pws = fmaf(-pg, Q[k], pws);
        }
      }
      s2[0] = (double)pwa;
      s2[1] = (double)pws;
      float d = 0.f;
#pragma unroll
      for (int l = 0; l < C; ++l) d = fmaf(Q[l], gQ[l], d);
      float gLp[C];
#pragma unroll
      for (int l = 0; l < C; ++l) gLp[l] = Q[l] * (gQ[l] - d);
      // gU accumulates t = T, T-1, .., 1, then gL^0, by the lane that owns the pixel
#pragma unroll
      for (int l = 0; l < C; ++l) {
        if (C == 2 && binary && l == 0) continue;              // binary: gz = gU_1
        const long long ui = (C == 2 && binary) ? n * hw + px : ((long long)n * C + l) * hw + px;
        const float gl = g.gl_in[((long long)n * C + l) * hw + px];
        float acc = first ? gl : g.gu[ui] + gl;
        if (last) acc = acc + gLp[l];
        g.gu[ui] = acc;
      }
      if (!last) {
#pragma unroll
        for (int l = 0; l < C; ++l) g.gl_out[((long long)n * C + l) * hw + px] = gLp[l];
      }
    }
    // fp64 per tile and iteration; a lane outside the image adds zeros
    hpri_block_sum<2, CRF_THREADS>(red, s2);
    if (threadIdx.x == 0) {
      g.partials[(long long)item * R + 0] = red[0][0];
      g.partials[(long long)item * R + 1] = red[1][0];
    }
    if (g.flags & CRF_WANT_MU) {
#pragma unroll
      for (int i = 0; i < C * C; i += 2) {
        s2[0] = (double)(-(H[i / C] * Q[i % C]));
        s2[1] = i + 1 < C * C ? (double)(-(H[(i + 1) / C] * Q[(i + 1) % C])) : 0.0;
        __syncthreads();                                         // (thread 0 has read the sums before)
        hpri_block_sum<2, CRF_THREADS>(red, s2);
        if (threadIdx.x == 0) {
          g.partials[(long long)item * R + 2 + i] = red[0][0];
          if (i + 1 < C * C) g.partials[(long long)item * R + 3 + i] = red[1][0];
        }
      }
    }
    __syncthreads();
  }
}

// gL^T from the gradient of the output, one lane a pixel.  Binary logit: (-g, +g).  Prob: gv = g (binary: (0, g)), d = fmaf(Q_l, gv_l, d)
// over l, gL_l = Q_l (gv_l - d) with Q = Q^T as the forward kept it.
__global__ void crf_grad_start_kernel(const float* __restrict__ g, const float* __restrict__ q, float* __restrict__ gl, long long pixels,
                                      long long hw, int C, int binary, int output) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < pixels; i += (long long)gridDim.x * blockDim.x) {
    const long long n = i / hw, px = i - n * hw;
    const long long base = n * C * hw + px;
    if (output == 0) {
      const float v = g[i];
      gl[base] = -v;
      gl[base + hw] = v;
    } else {
      float d = 0.f;
      for (int l = 0; l < C; ++l) {
        const float gv = binary ? (l == 1 ? g[i] : 0.f) : g[base + l * hw];
        d = fmaf(q[base + l * hw], gv, d);
      }
      for (int l = 0; l < C; ++l) {
        const float gv = binary ? (l == 1 ? g[i] : 0.f) : g[base + l * hw];
        gl[base + l * hw] = q[base + l * hw] * (gv - d);
      }
    }
  }
}

// One block of 256 threads adds the fp64 partial sums of value v of (w_a, w_s, mu row-major): the T x tiles sums are taken in the order t
// descending, tile ascending; thread j adds entries j, j + 256, .. of that sequence in that order, the halving tree adds the 256 threads'
// sums, and the total rounds once to fp32.  Nothing in it depends on the grid of the launches before.
#define CRF_FINISH_THREADS 256
__global__ __launch_bounds__(CRF_FINISH_THREADS) void crf_grad_finish_kernel(const double* __restrict__ partials, int T, int items, int R,
                                                                             int count, float* __restrict__ gwa, float* __restrict__ gws,
                                                                             float* __restrict__ gmu) {
  __shared__ double red[1][CRF_FINISH_THREADS];
  const long long total = (long long)T * items;
  for (int v = 0; v < count; ++v) {
    float* dst = v == 0 ? gwa : v == 1 ? gws : (gmu ? gmu + (v - 2) : nullptr);
    if (!dst) continue;                                          // (uniform: every thread sees the same pointers)
    double s[1] = {0.0};
    for (long long i = threadIdx.x; i < total; i += CRF_FINISH_THREADS) {
      const long long t = T - 1 - i / items, tile = i % items;
      s[0] += partials[(t * items + tile) * R + v];
    }
    hpri_block_sum<1, CRF_FINISH_THREADS>(red, s);
    if (threadIdx.x == 0) *dst = (float)red[0][0];
    __syncthreads();
  }
}

// ---- host --------------------------------------------------------------------------------------------------------------------------
template <int K, int C>
static inline void crf_back_launch(const CrfBackArgs& g, int blocks, size_t lds, hipStream_t stream) {
  hpri_ask_dynamic_lds(crf_back_kernel<K, C>, lds);
  hipLaunchKernelGGL((crf_back_kernel<K, C>), dim3(blocks), dim3(CRF_THREADS), lds, stream, g);
}

template <int K>
static inline void crf_back_launch_classes(const CrfBackArgs& g, int C, int blocks, size_t lds, hipStream_t stream) {
  switch (C) {
    case 2: crf_back_launch<K, 2>(g, blocks, lds, stream); break;
    case 3: crf_back_launch<K, 3>(g, blocks, lds, stream); break;
    case 4: crf_back_launch<K, 4>(g, blocks, lds, stream); break;
    case 5: crf_back_launch<K, 5>(g, blocks, lds, stream); break;
    case 6: crf_back_launch<K, 6>(g, blocks, lds, stream); break;
    case 7: crf_back_launch<K, 7>(g, blocks, lds, stream); break;
    default: crf_back_launch<K, 8>(g, blocks, lds, stream); break;
  }
}

extern "C" int hpri_dense_crf_backward(const float* grad_out, const float* unary, int binary, const float* guide, int gs, int K, int N, int C,
                                       int H, int W, int radius, int iterations, const float* ta, const float* tg, float b,
                                       const float* w_a, const float* w_s, const float* compat, int output, void* workspace,
                                       size_t workspace_bytes, float* grad_unary, float* grad_w_a, float* grad_w_s, float* grad_compat,
                                       hipStream_t stream) {
  HPRI_REQUIRE(grad_out && unary && ta && tg && w_s && workspace && grad_unary, "dense_crf_backward: null pointer");
  HPRI_REQUIRE(crf_frame_ok(N, C, H, W), "dense_crf_backward: bad sizes (N, H, W >= 1, C in [2, hpri_crf_max_classes])");
  HPRI_REQUIRE(binary == 0 || (binary == 1 && C == 2), "dense_crf_backward: binary must be 0, or 1 with C = 2");
  HPRI_REQUIRE(K >= 0 && K <= CRF_MAX_K, "dense_crf_backward: K must lie in [0, hpri_crf_max_guides]");
  HPRI_REQUIRE(K == 0 || (guide && gs >= K && w_a), "dense_crf_backward: a guide needs a pointer, a channel stride of at least K and w_a");
  HPRI_REQUIRE(radius >= 1 && radius <= CRF_MAX_R, "dense_crf_backward: the radius must lie in [1, hpri_crf_max_radius]");
  HPRI_REQUIRE(iterations >= 1 && iterations <= CRF_MAX_T, "dense_crf_backward: the iterations must lie in [1, hpri_crf_max_iterations]");
  HPRI_REQUIRE(crf_unit_table(ta, radius) && crf_unit_table(tg, radius),
               "dense_crf_backward: a spatial table must start at 1 and fall to no less than 0");
  HPRI_REQUIRE(K == 0 || (b > 0.f && b <= 3.0e38f), "dense_crf_backward: b must be positive and finite");
  HPRI_REQUIRE(output == 0 || output == 1, "dense_crf_backward: output must be 0 (logit) or 1 (prob)");
  HPRI_REQUIRE(compat || !grad_compat, "dense_crf_backward: Potts has no compatibility matrix to differentiate");
  HPRI_REQUIRE(K > 0 || !grad_w_a, "dense_crf_backward: without a guide there is no w_a to differentiate");
  HPRI_REQUIRE(workspace_bytes >= hpri_crf_train_workspace_bytes(N, C, H, W, iterations), "dense_crf_backward: the workspace is too small");
  HPRI_REQUIRE((((uintptr_t)grad_out | (uintptr_t)unary | (uintptr_t)guide | (uintptr_t)w_a | (uintptr_t)w_s | (uintptr_t)compat |
                 (uintptr_t)grad_unary | (uintptr_t)grad_w_a | (uintptr_t)grad_w_s | (uintptr_t)grad_compat) & 3) == 0 &&
                   ((uintptr_t)workspace & 7) == 0, "dense_crf_backward: misaligned pointer");
  CrfBackArgs g = {};
  for (int d = 0; d <= radius; ++d) {
    g.ta[d] = ta[d];
    g.tg[d] = tg[d];
  }
  g.guide = guide; g.gu = grad_unary; g.wa_dev = w_a; g.ws_dev = w_s; g.mu_dev = compat; g.b = K > 0 ? b : 0.f;
  g.gs = gs; g.H = H; g.W = W; g.r = radius; g.tiles_x = hpri_cdiv(W, CRF_TILE_W); g.tiles_y = hpri_cdiv(H, CRF_TILE_H);
  g.items = (int)((long long)g.tiles_x * g.tiles_y * N);
  const int flags = (K > 0 && gs % 4 == 0 && hpri_aligned16(guide) ? CRF_VEC : 0) | (binary ? CRF_BINARY : 0) | (grad_compat ? CRF_WANT_MU : 0);
  const int R = 2 + C * C;
  const size_t set = (size_t)N * C * H * W;
  double* partials = (double*)workspace;
  float* stack = (float*)(partials + crf_train_partials(N, C, H, W, iterations));
  float* gl[2] = {stack + (size_t)iterations * set, stack + (size_t)(iterations + 1) * set};
  const float* cur = grad_out;
  if (binary || output == 1) {
    const long long pixels = (long long)N * H * W;
    hipLaunchKernelGGL(crf_grad_start_kernel, dim3(hpri_grid_capped(pixels, 256)), dim3(256), 0, stream, grad_out,
                       stack + (size_t)(iterations - 1) * set, gl[0], pixels, (long long)H * W, C, binary, output);
    HPRI_CHECK_LAUNCH();
    cur = gl[0];
  }
  const size_t lds = CRF_RED_DOUBLES * sizeof(double) + crf_plane_lds(radius, K, C) + (compat ? (size_t)C * C * sizeof(float) : 0);
  const int blocks = g.items;
  for (int t = iterations; t >= 1; --t) {
    float* next = cur == gl[0] ? gl[1] : gl[0];
    g.flags = flags | (t == iterations ? CRF_FIRST : 0) | (t == 1 ? CRF_LAST : 0);
    g.gl_in = cur; g.gl_out = t == 1 ? nullptr : next;
    g.qsrc = t == 1 ? unary : stack + (size_t)(t - 2) * set;
    g.partials = partials + (size_t)(t - 1) * g.items * R;
    switch (K) {
      case 0: crf_back_launch_classes<0>(g, C, blocks, lds, stream); break;
      case 1: crf_back_launch_classes<1>(g, C, blocks, lds, stream); break;
      case 2: crf_back_launch_classes<2>(g, C, blocks, lds, stream); break;
      default: crf_back_launch_classes<3>(g, C, blocks, lds, stream); break;
    }
    HPRI_CHECK_LAUNCH();
    cur = next;
  }
  if (grad_w_a || grad_w_s || grad_compat) {
    hipLaunchKernelGGL(crf_grad_finish_kernel, dim3(1), dim3(CRF_FINISH_THREADS), 0, stream, (const double*)partials, iterations, g.items, R,
                       grad_compat ? R : 2, grad_w_a, grad_w_s, grad_compat);
    HPRI_CHECK_LAUNCH();
  }
  return HPRI_OK;
}
