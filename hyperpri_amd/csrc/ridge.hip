// Multi-scale Hessian ridge filter ("vesselness", after Frangi et al. and Sato et al.) for thin roots: hpri_ridge_filter.
//
// T fp32 planes on an (N, H, W) frame, addressed by an image, a plane and a pixel stride; 1 <= S <= 8 scales sigma in [0.5, 4] with the
// tap radius R = ceil(3 sigma) <= 12.  The host hands over three half-kernels per scale, g0 | g1 | g2 for x = 1 .. R, as fp32 values
// (hyperpri_amd/ridge.py: ridge_taps); there is no centre tap, every pass works on differences from its own centre, so the kernels are
// exactly unit-sum (g0) or zero-sum (g1, g2) whatever the rounding of the taps.  include/hyperpri_hip.h states the contract:
//
//   borders: half-sample symmetric reflection rho (d c b a | a b c d), period 2n: defined on images smaller than R, down to 1 x 1
//   row pass, per pixel and scale, fp32 from +0.0, c = I[y, x], j = 1 .. R:
//     dp = I[y, rho(x+j)] - c,  dm = I[y, rho(x-j)] - c
//     s0 = fmaf(g0[j], dp + dm, s0),  r1 = fmaf(g1[j], dp - dm, r1),  r2 = fmaf(g2[j], dp + dm, r2)
//   column pass, fp32 from +0.0, i = 1 .. R, +- the rows rho(y +- i) at the same x:
//     axx = fmaf(g0[i], (r2+ - r2c) + (r2- - r2c), axx),  Hxx = (r2c + axx) sigma^2
//     axy = fmaf(g1[i], r1+ - r1-, axy),                  Hxy = axy sigma^2
//     ayy = fmaf(g2[i], e+ + e-, ayy),                    Hyy = ayy sigma^2,   e+- = (I+- - Ic) + (s0+- - s0c)
//   measure, fp64, no contraction; the maximum over the scales in the order given, the index of the first scale that attains it.
//
// A workgroup of 512 lanes owns a tile of 16 x 32 pixels, one lane a pixel.  The tile with a halo of the launch's largest R lies in LDS
// once, already reflected (domain prob: the sigmoid is applied while staging); per scale the row pass writes s0 | r1 | r2 for the
// tile's rows plus 2R halo rows into three LDS planes of 32 columns, the column pass reads them back, the fp64 epilogue keeps the
// running maximum and its index in registers.  In both passes consecutive lanes read consecutive LDS words; every loop bound is
// uniform.  A reflected halo makes every LDS word a pixel of the image, so no lane needs a validity test: the result of a pixel depends
// on its neighbourhood and its distance to the borders only, not on N, T, the other maps, the grid, the tile or its place in a tile, and
// a scale's Hessian planes do not depend on the other scales.  No atomics.
#include "tail_helpers.h"

#pragma clang fp contract(off)               // every fmaf of the contract is written out; nothing else is fused

#define RF_TILE_H 16
#define RF_TILE_W 32
#define RF_THREADS (RF_TILE_H * RF_TILE_W)
#define RF_MAX_S 8
#define RF_MAX_R 12
#define RF_PER_CU 8                          // workgroups a CU is offered (measured at 2, 4, 6, 8); the kernel strides over the rest
#define RF_IMG_H (RF_TILE_H + 2 * RF_MAX_R)  // 40 rows of the staged tile at the largest halo
#define RF_IMG_W (RF_TILE_W + 2 * RF_MAX_R)  // 56 columns

struct RfArgs {
  const float* in;
  float* out;              // (N, T, H, W): the response, or its logit
  unsigned char* scale;    // (N, T, H, W) or null: the index of the winning scale
  float* hess;             // (N, T, S, 3, H, W): Hxx | Hxy | Hyy (HESS instantiations)
  long long si, st, sp;    // image, plane and pixel stride of `in`, in floats
  long long items;         // tiles x maps x images
  float taps[RF_MAX_S][3][RF_MAX_R];
  float sigma2[RF_MAX_S];
  int radius[RF_MAX_S];
  float beta, c;
  int N, T, H, W, S, Rm, logit, tiles_x, tiles_y;
};

// half-sample symmetric reflection of any integer onto [0, n)
__device__ __forceinline__ int rf_reflect(int i, int n) {
  const int p = 2 * n;
  int m = i % p;
  if (m < 0) m += p;
  return m < n ? m : p - 1 - m;
}

// POL 0 bright, 1 dark, 2 both; MEAS 0 frangi, 1 sato
template <int POL, int MEAS>
__device__ __forceinline__ double rf_measure(float hxx, float hxy, float hyy, double two_beta2, double two_c2) {
  const double a = (double)hxx, b = (double)hxy, e = (double)hyy;
  const double mu = (a + e) / 2.0, hd = (a - e) / 2.0;
  const double d = sqrt(hd * hd + b * b);
  double l1, l2;
  bool gate = true;
  if (POL == 0) {
    l2 = mu - d; l1 = mu + d; gate = mu < 0.0;
  } else if (POL == 1) {
    l2 = mu + d; l1 = mu - d; gate = mu > 0.0;
  } else if (mu >= 0.0) {
    l2 = mu + d; l1 = mu - d;
  } else {
    l2 = mu - d; l1 = mu + d;
  }
  if (MEAS == 1) {
    const double x = POL == 0 ? -l2 : (POL == 1 ? l2 : fabs(l2));
    return x > 0.0 ? x : 0.0;
  }
  if (!gate || l2 == 0.0) return 0.0;
  const double rb = l1 / l2;
  const double blob = exp(-(rb * rb) / two_beta2);
  const double structure = -expm1(-(l1 * l1 + l2 * l2) / two_c2);
  return blob * structure;
}

template <int POL, int MEAS, int PROB, int HESS>
__global__ __launch_bounds__(RF_THREADS) void ridge_filter_kernel(const RfArgs g) {
  __shared__ float img[RF_IMG_H * RF_IMG_W];
  __shared__ float rows[3][RF_IMG_H * RF_TILE_W];
  const int Rm = g.Rm, lw = RF_TILE_W + 2 * Rm, lh = RF_TILE_H + 2 * Rm;
  const int ty = threadIdx.x / RF_TILE_W, tx = threadIdx.x % RF_TILE_W;
  const long long hw = (long long)g.H * g.W;
  const double two_beta2 = 2.0 * (double)g.beta * (double)g.beta, two_c2 = 2.0 * (double)g.c * (double)g.c;
  for (long long item = blockIdx.x; item < g.items; item += gridDim.x) {
    const int txi = (int)(item % g.tiles_x);
    long long rest = item / g.tiles_x;
    const int tyi = (int)(rest % g.tiles_y);
    rest /= g.tiles_y;                                           // rest = n * T + t
    const int t = (int)(rest % g.T), n = (int)(rest / g.T);
    const int y0 = tyi * RF_TILE_H, x0 = txi * RF_TILE_W;
    const float* __restrict__ src = g.in + n * g.si + t * g.st;
    for (int idx = threadIdx.x; idx < lw * lh; idx += RF_THREADS) {
      const int ly = idx / lw, lx = idx - ly * lw;
      const int yy = rf_reflect(y0 - Rm + ly, g.H), xx = rf_reflect(x0 - Rm + lx, g.W);
      float v = src[((long long)yy * g.W + xx) * g.sp];
      if (PROB) {
        float sn;
        hpri_sigmoids(v, v, sn);
      }
      img[idx] = v;
    }
    __syncthreads();
    const int y = y0 + ty, x = x0 + tx;
    const bool inside = y < g.H && x < g.W;
    const int ic = (Rm + ty) * lw + Rm + tx, rc = (Rm + ty) * RF_TILE_W + tx;
    double best = 0.0;
    int arg = 0;
    for (int s = 0; s < g.S; ++s) {
      const int R = g.radius[s];
      // row pass: the tile's rows and R halo rows above and below, 32 columns
      for (int idx = threadIdx.x; idx < (RF_TILE_H + 2 * R) * RF_TILE_W; idx += RF_THREADS) {
        const int ly = Rm - R + idx / RF_TILE_W, col = idx % RF_TILE_W;
        const int b = ly * lw + Rm + col;
        const float c = img[b];
        float s0 = 0.f, r1 = 0.f, r2 = 0.f;
        for (int j = 1; j <= R; ++j) {
          const float dp = img[b + j] - c, dm = img[b - j] - c;
          const float sum = dp + dm;
          s0 = fmaf(g.taps[s][0][j - 1], sum, s0);
          r1 = fmaf(g.taps[s][1][j - 1], dp - dm, r1);
          r2 = fmaf(g.taps[s][2][j - 1], sum, r2);
        }
        rows[0][ly * RF_TILE_W + col] = s0;
        rows[1][ly * RF_TILE_W + col] = r1;
        rows[2][ly * RF_TILE_W + col] = r2;
      }
      __syncthreads();
      // column pass
      const float Ic = img[ic], s0c = rows[0][rc], r2c = rows[2][rc];
      float axx = 0.f, axy = 0.f, ayy = 0.f;
      for (int i = 1; i <= R; ++i) {
        const int up = rc + i * RF_TILE_W, dn = rc - i * RF_TILE_W;
        const float ep = (img[ic + i * lw] - Ic) + (rows[0][up] - s0c);
        const float em = (img[ic - i * lw] - Ic) + (rows[0][dn] - s0c);
        axx = fmaf(g.taps[s][0][i - 1], (rows[2][up] - r2c) + (rows[2][dn] - r2c), axx);
        axy = fmaf(g.taps[s][1][i - 1], rows[1][up] - rows[1][dn], axy);
        ayy = fmaf(g.taps[s][2][i - 1], ep + em, ayy);
      }
      const float s2 = g.sigma2[s];
      const float hxx = (r2c + axx) * s2, hxy = axy * s2, hyy = ayy * s2;
      if (HESS && inside) {
        float* h = g.hess + ((rest * g.S + s) * 3) * hw + (long long)y * g.W + x;
        h[0] = hxx;
        h[hw] = hxy;
        h[2 * hw] = hyy;
      }
      const double v = rf_measure<POL, MEAS>(hxx, hxy, hyy, two_beta2, two_c2);
      if (s == 0 || v > best) {
        best = v;
        arg = s;
      }
      __syncthreads();                       // the next scale's row pass (or the next item's staging) overwrites what this one read
    }
    if (inside) {
      const long long o = rest * hw + (long long)y * g.W + x;
      if (g.logit) {
        const double p = MEAS == 1 ? best / (best + (double)g.c) : best;
        g.out[o] = hpri_clamped_logit((float)p);
      } else {
        g.out[o] = (float)best;
      }
      if (g.scale) g.scale[o] = (unsigned char)arg;
    }
  }
}

// ---- host --------------------------------------------------------------------------------------------------------------------------
extern "C" int hpri_ridge_max_scales(void) { return RF_MAX_S; }
extern "C" int hpri_ridge_max_radius(void) { return RF_MAX_R; }
extern "C" int hpri_ridge_tile_h(void) { return RF_TILE_H; }
extern "C" int hpri_ridge_tile_w(void) { return RF_TILE_W; }

static inline bool rf_finite(float v) { return v == v && v <= 3.0e38f && v >= -3.0e38f; }

template <int POL, int MEAS>
static void rf_launch(const RfArgs& g, int prob, int hess, hipStream_t stream) {
  const int blocks = hpri_grid_per_cu(g.items, 1, RF_PER_CU);
  if (prob) {
    if (hess) hipLaunchKernelGGL((ridge_filter_kernel<POL, MEAS, 1, 1>), dim3(blocks), dim3(RF_THREADS), 0, stream, g);
    else hipLaunchKernelGGL((ridge_filter_kernel<POL, MEAS, 1, 0>), dim3(blocks), dim3(RF_THREADS), 0, stream, g);
  } else {
    if (hess) hipLaunchKernelGGL((ridge_filter_kernel<POL, MEAS, 0, 1>), dim3(blocks), dim3(RF_THREADS), 0, stream, g);
    else hipLaunchKernelGGL((ridge_filter_kernel<POL, MEAS, 0, 0>), dim3(blocks), dim3(RF_THREADS), 0, stream, g);
  }
}

extern "C" int hpri_ridge_filter(const float* maps, long long image_stride, long long plane_stride, long long pixel_stride, int N, int T,
                                 int H, int W, const float* taps, const int* radii, const float* sigma2, int S, float beta, float c,
                                 int polarity, int measure, int domain, int output, float* out, unsigned char* scale, float* hessian,
                                 hipStream_t stream) {
  HPRI_REQUIRE(maps && taps && radii && sigma2 && out, "ridge_filter: null pointer");
  HPRI_REQUIRE(N > 0 && T > 0 && H > 0 && W > 0 && H < (1 << 30) && W < (1 << 30) && (long long)N * T * H * W < (1LL << 31),
               "ridge_filter: bad sizes (N, T, H, W >= 1, N T H W < 2^31)");
  HPRI_REQUIRE(S >= 1 && S <= RF_MAX_S, "ridge_filter: the number of scales must lie in [1, hpri_ridge_max_scales]");
  HPRI_REQUIRE(pixel_stride >= 1 && image_stride >= 0 && plane_stride >= 0, "ridge_filter: bad strides");
  HPRI_REQUIRE(polarity >= 0 && polarity <= 2, "ridge_filter: polarity must be 0 (bright), 1 (dark) or 2 (both)");
  HPRI_REQUIRE(measure == 0 || measure == 1, "ridge_filter: measure must be 0 (frangi) or 1 (sato)");
  HPRI_REQUIRE(domain == 0 || domain == 1, "ridge_filter: domain must be 0 (linear) or 1 (prob)");
  HPRI_REQUIRE(output == 0 || output == 1, "ridge_filter: output must be 0 (value) or 1 (logit)");
  HPRI_REQUIRE(rf_finite(beta) && beta > 0.f && rf_finite(c) && c > 0.f, "ridge_filter: beta and c must be positive and finite");
  HPRI_REQUIRE((((uintptr_t)maps | (uintptr_t)out | (uintptr_t)hessian) & 3) == 0, "ridge_filter: misaligned pointer");
  RfArgs g = {};
  int Rm = 0;
  for (int s = 0; s < S; ++s) {
    const int R = radii[s];
    HPRI_REQUIRE(R >= 1 && R <= RF_MAX_R, "ridge_filter: a radius must lie in [1, hpri_ridge_max_radius]");
    HPRI_REQUIRE(rf_finite(sigma2[s]) && sigma2[s] > 0.f, "ridge_filter: sigma^2 must be positive and finite");
    for (int k = 0; k < 3; ++k)
      for (int j = 0; j < RF_MAX_R; ++j) {
        const float v = taps[(s * 3 + k) * RF_MAX_R + j];
        HPRI_REQUIRE(rf_finite(v), "ridge_filter: non-finite tap");
        g.taps[s][k][j] = j < R ? v : 0.f;
      }
    g.radius[s] = R;
    g.sigma2[s] = sigma2[s];
    if (R > Rm) Rm = R;
  }
  g.in = maps; g.out = out; g.scale = scale; g.hess = hessian;
  g.si = image_stride; g.st = plane_stride; g.sp = pixel_stride;
  g.beta = beta; g.c = c;
  g.N = N; g.T = T; g.H = H; g.W = W; g.S = S; g.Rm = Rm; g.logit = output;
  g.tiles_x = hpri_cdiv(W, RF_TILE_W); g.tiles_y = hpri_cdiv(H, RF_TILE_H);
  g.items = (long long)g.tiles_x * g.tiles_y * N * T;
  const int hess = hessian != nullptr;
  switch (polarity * 2 + measure) {
    case 0: rf_launch<0, 0>(g, domain, hess, stream); break;
    case 1: rf_launch<0, 1>(g, domain, hess, stream); break;
    case 2: rf_launch<1, 0>(g, domain, hess, stream); break;
    case 3: rf_launch<1, 1>(g, domain, hess, stream); break;
    case 4: rf_launch<2, 0>(g, domain, hess, stream); break;
    default: rf_launch<2, 1>(g, domain, hess, stream); break;
  }
  HPRI_CHECK_LAUNCH();
  return HPRI_OK;
}
