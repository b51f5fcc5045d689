// Imbalance-aware losses of the BINARY tail: what step.hip's BCE does for the unweighted mean, for one family
//
//   loss = w_point * R_elems[ a_t * (1 - p_t)^gf * ce(x, y) ]  +  w_overlap * mean_groups[ (1 - T_g)^gt ]
//
//   ce(x, y) = pos_weight * y * softplus(-x) + (1 - y) * softplus(x)          p = sigmoid(x)
//   1 - p_t  = y * sigmoid(-x) + (1 - y) * sigmoid(x)                         a_t = af * y + (1 - af) * (1 - y)   (af < 0: 1)
//   T_g = (I + s) / D,   D = I + alpha * (P - I) + beta * (Y - I) + s,   I = sum p*y, P = sum p, Y = sum y over group g
//
// -- weighted BCE (gf = 0), focal (torchvision's sigmoid_focal_loss: gf 2, af 0.25), soft Dice (alpha = beta = 1/2; the usual
// (2 I + smooth) / (P + Y + smooth) is s = smooth / 2), Tversky, focal Tversky (gt != 1) and any weighted sum of a pointwise and an
// overlap term.  R_elems: the mean or the sum over all elements; a group: one image (per_image) or the whole batch.  Logits and
// targets are contiguous fp32, n_img images of hw elements; targets lie in [0, 1] (soft labels allowed).
//
// One pass forward (8 bytes per element), one pass backward (12), HBM-bound.  A lane owns four adjacent elements of one image:
// 16-byte accesses when hw % 4 == 0 and every base pointer is 16-byte aligned, element accesses otherwise; which lane owns which
// element is the same in both forms, so their results are bit-identical (hpri_load4 / hpri_store4).  A workgroup works on one
// image at a time (a "unit": one of the bpi slices of an image), so its four fp64 partial sums (pointwise, I, P, Y) belong to one
// group; they are reduced through LDS in a fixed order, and the finalize kernel sums the units of a group in a fixed order too:
// no floating-point atomics, bit-reproducible.  No host synchronisation: the finalize kernel leaves what the backward needs in a
// small device buffer (`state`), the upstream gradient is read from device memory.  A term whose weight is 0 is not evaluated
// (template arguments), so a loss with a dropped term gives the bits of the stand-alone loss.
//
// Numerics: softplus(z) = max(z, 0) + log1p(exp(-|z|)); sigmoid(x) and sigmoid(-x) come from one exp(-|x|) (hpri_sigmoids), and
// (1 - p_t)^gf is formed from 1 - p_t itself, never from 1 - (p_t): a confident correct pixel keeps its relative accuracy.
//
// Backward, with G groups and g the upstream gradient:
//   dL/dT_g = -gt * (1 - T_g)^(gt - 1)
//   c1_g = w_overlap / G * dL/dT_g * (D - (I + s) * (1 - alpha - beta)) / D^2        (the factor of y_i)
//   c0_g = w_overlap / G * dL/dT_g * (-(I + s) * alpha) / D^2
//   dx_i = g * [ scale_point * d(pointwise_i)/dx_i + (c1_g * y_i + c0_g) * sigmoid(x_i) * sigmoid(-x_i) ]
//   d(pointwise)/dx = a_t * q^gf * [ gf * (1 - 2y) * (sigmoid(x) sigmoid(-x) / q) * ce + (1 - y) sigmoid(x) - pos_weight y sigmoid(-x) ]
// with q = 1 - p_t (analytic for any y in [0, 1]; for a hard label sigmoid(x) sigmoid(-x) / q is p_t).
//
// Edge rules: D == 0 (possible only with s = 0 when every p and y of the group underflows) gives T = 1; T >= 1 gives a term of 0
// and dL/dT = 0 (for gt < 1 the derivative is unbounded there; targets outside [0, 1] can push T past 1).
#include "tail_helpers.h"
#include <math.h>

#define SL_THREADS 256

struct SlPoint { float pos_weight, focal_gamma, focal_alpha; };      // the pointwise term's parameters

// units per image: ceil(quads / 256) slices, while n_img * bpi stays within HPRI_MAX_BLOCKS (one slice per image beyond that)
static inline int sl_bpi(int n_img, long long hw) {
  long long b = ((hw + 3) / 4 + SL_THREADS - 1) / SL_THREADS;
  const long long cap = n_img >= HPRI_MAX_BLOCKS ? 1 : HPRI_MAX_BLOCKS / n_img;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (int)b;
}

__device__ __forceinline__ float sl_ce(float x, float y, float lg, float pos_weight) {
  return pos_weight * y * (fmaxf(-x, 0.f) + lg) + (1.f - y) * (fmaxf(x, 0.f) + lg);
}

__device__ __forceinline__ float sl_pow(float q, float gamma) {      // q >= 0, gamma >= 0 (wave-uniform)
  return gamma == 0.f ? 1.f : gamma == 1.f ? q : gamma == 2.f ? q * q : powf(q, gamma);
}

__device__ __forceinline__ float sl_alpha_t(float y, float focal_alpha) {
  return focal_alpha < 0.f ? 1.f : focal_alpha * y + (1.f - focal_alpha) * (1.f - y);
}

// ------------------------------------------------------------------------------------------------
// Forward.  partial[r * units + u], r = 0..3: unit u's fp64 sums of the pointwise values, p*y, p and y (zeros for a dropped term).
// FOCAL: the pointwise term carries a_t * (1 - p_t)^gf (gf != 0 or af >= 0).
// ------------------------------------------------------------------------------------------------
template <int POINT, int FOCAL, int OVERLAP>
__global__ __launch_bounds__(SL_THREADS) void seg_loss_fwd_kernel(const float* __restrict__ x, const float* __restrict__ y, long long hw,
                                                                  int bpi, long long units, int vec, SlPoint pc,
                                                                  double* __restrict__ partial) {
  __shared__ double red[4][SL_THREADS];
  const long long qpi = (hw + 3) >> 2;
  for (long long unit = blockIdx.x; unit < units; unit += gridDim.x) {
    const long long img = unit / bpi;
    const int slice = (int)(unit - img * bpi);
    const float* px = x + img * hw;
    const float* py = y + img * hw;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (long long q = (long long)slice * SL_THREADS + threadIdx.x; q < qpi; q += (long long)bpi * SL_THREADS) {
      const long long p0 = q * 4;
      const int cnt = hw - p0 < 4 ? (int)(hw - p0) : 4;
      float xv[4], yv[4];
      hpri_load4(px + p0, cnt, vec, xv);
      hpri_load4(py + p0, cnt, vec, yv);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < cnt) {
          float sp, sn, lg;
          hpri_sigmoids<POINT>(xv[j], sp, sn, lg);
          if (POINT) {
            float v = sl_ce(xv[j], yv[j], lg, pc.pos_weight);
            if (FOCAL) v *= sl_alpha_t(yv[j], pc.focal_alpha) * sl_pow(yv[j] * sn + (1.f - yv[j]) * sp, pc.focal_gamma);
            s[0] += (double)v;
          }
          if (OVERLAP) {
            s[1] += (double)sp * (double)yv[j];
            s[2] += (double)sp;
            s[3] += (double)yv[j];
          }
        }
      }
    }
    hpri_block_sum(red, s);
    if (threadIdx.x < 4) partial[(size_t)threadIdx.x * units + unit] = red[threadIdx.x][0];
    __syncthreads();                                    // (red is written again by the block's next unit)
  }
}

// ------------------------------------------------------------------------------------------------
// Finalize: one workgroup, fp64.  Wave w takes groups w, w + 4, ...: its lanes stride over the group's units (one image's bpi
// slices, or every unit for a per-batch group), a xor-butterfly leaves the four sums in every lane -- a fixed order throughout.
//   loss[0]   the loss;  terms[0..2] = R_elems[...], mean_groups[(1 - T)^gt] (both unweighted; 0 for a dropped term), mean T
//   state[0]  scale_point = w_point (/ n for a mean);  state[1 + 2g], state[2 + 2g] = c1_g, c0_g
// ------------------------------------------------------------------------------------------------
struct SlOverlap { double w, alpha, beta, s, gamma; };

__global__ __launch_bounds__(SL_THREADS) void seg_loss_finalize_kernel(const double* __restrict__ partial, long long units, int bpi,
                                                                       int groups, int per_image, double w_point, double n_elems, int mean,
                                                                       SlOverlap oc, float* __restrict__ loss, double* __restrict__ state,
                                                                       float* __restrict__ terms) {
  __shared__ double wsum[3][SL_THREADS / 64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double accp = 0.0, acco = 0.0, acct = 0.0;
  for (int g = wave; g < groups; g += SL_THREADS / 64) {
    const long long u0 = per_image ? (long long)g * bpi : 0, u1 = per_image ? u0 + bpi : units;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (long long u = u0 + lane; u < u1; u += 64) {
#pragma unroll
      for (int r = 0; r < 4; ++r) s[r] += partial[(size_t)r * units + u];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) s[r] = hpri_wave_sum(s[r]);
    accp += s[0];
    double c1 = 0.0, c0 = 0.0;
    if (oc.w != 0.0) {
      const double I = s[1], P = s[2], Y = s[3];
      const double num = I + oc.s, D = I + oc.alpha * (P - I) + oc.beta * (Y - I) + oc.s;
      const double T = D == 0.0 ? 1.0 : num / D;                      // (edge rule: an empty group counts as a perfect overlap)
      const double om = 1.0 - T;
      double term = 0.0, dLdT = 0.0;
      if (om > 0.0) {                                                 // (edge rule: T >= 1 -> term 0, derivative 0)
        term = oc.gamma == 1.0 ? om : pow(om, oc.gamma);
        dLdT = oc.gamma == 1.0 ? -1.0 : -oc.gamma * pow(om, oc.gamma - 1.0);
      }
      if (D != 0.0) {
        const double k = oc.w / (double)groups * dLdT / (D * D);
        c1 = k * (D - num * (1.0 - oc.alpha - oc.beta));
        c0 = k * (-num * oc.alpha);
      }
      acco += term;
      acct += T;
    }
    if (lane == 0) { state[1 + 2 * (size_t)g] = c1; state[2 + 2 * (size_t)g] = c0; }
  }
  if (lane == 0) { wsum[0][wave] = accp; wsum[1][wave] = acco; wsum[2][wave] = acct; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double p = 0.0, o = 0.0, t = 0.0;
    for (int w = 0; w < SL_THREADS / 64; ++w) { p += wsum[0][w]; o += wsum[1][w]; t += wsum[2][w]; }
    const double point = w_point != 0.0 ? (mean ? p / n_elems : p) : 0.0;
    const double over = oc.w != 0.0 ? o / (double)groups : 0.0;
    double l = 0.0;
    if (w_point != 0.0) l = w_point * point;
    if (oc.w != 0.0) l = w_point != 0.0 ? l + oc.w * over : oc.w * over;
    loss[0] = (float)l;
    state[0] = mean ? w_point / n_elems : w_point;
    terms[0] = (float)point;
    terms[1] = (float)over;
    terms[2] = oc.w != 0.0 ? (float)(t / (double)groups) : 0.f;
  }
}

// ------------------------------------------------------------------------------------------------
// Backward: one pass, dx as in the header comment.  c1 * y + c0 is formed in fp64: for a soft label it may cancel.
// ------------------------------------------------------------------------------------------------
template <int POINT, int FOCAL, int OVERLAP>
__global__ __launch_bounds__(SL_THREADS) void seg_loss_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y, long long hw,
                                                                  int bpi, long long units, int vec, SlPoint pc, int per_image,
                                                                  const double* __restrict__ state, const float* __restrict__ gout,
                                                                  float* __restrict__ dx) {
  const float g = gout ? gout[0] : 1.f;
  const float scale = (float)state[0];
  const long long qpi = (hw + 3) >> 2;
  for (long long unit = blockIdx.x; unit < units; unit += gridDim.x) {
    const long long img = unit / bpi;
    const int slice = (int)(unit - img * bpi);
    const float* px = x + img * hw;
    const float* py = y + img * hw;
    float* pd = dx + img * hw;
    double c1 = 0.0, c0 = 0.0;
    if (OVERLAP) {
      const size_t grp = per_image ? (size_t)img : 0;
      c1 = state[1 + 2 * grp];
      c0 = state[2 + 2 * grp];
    }
    for (long long q = (long long)slice * SL_THREADS + threadIdx.x; q < qpi; q += (long long)bpi * SL_THREADS) {
      const long long p0 = q * 4;
      const int cnt = hw - p0 < 4 ? (int)(hw - p0) : 4;
      float xv[4], yv[4], o[4];
      hpri_load4(px + p0, cnt, vec, xv);
      hpri_load4(py + p0, cnt, vec, yv);
      // (no j < cnt guard as in the forward: elements past cnt are computed from the zeros hpri_load4 left and dropped by hpri_store4)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float sp, sn, lg;
        hpri_sigmoids<(POINT && FOCAL)>(xv[j], sp, sn, lg);
        const float yy = yv[j];
        float d = 0.f;
        if (POINT) {
          d = (1.f - yy) * sp - pc.pos_weight * yy * sn;
          if (FOCAL) {
            const float q1 = yy * sn + (1.f - yy) * sp;                       // 1 - p_t
            const float ratio = q1 > 0.f ? sp * sn / q1 : 0.f;                // (q1 == 0: q1^gf == 0 as well, or gf == 0)
            const float ce = sl_ce(xv[j], yy, lg, pc.pos_weight);
            d = sl_alpha_t(yy, pc.focal_alpha) * sl_pow(q1, pc.focal_gamma) * (pc.focal_gamma * (1.f - 2.f * yy) * ratio * ce + d);
          }
          d *= scale;
        }
        if (OVERLAP) d += (float)(c1 * (double)yy + c0) * (sp * sn);
        o[j] = d * g;
      }
      hpri_store4(pd + p0, cnt, vec, o);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
// the checks shared by the forward and the backward (written so that a NaN fails them)
static int sl_check(int n_img, long long hw, float w_point, float pos_weight, float focal_gamma, float focal_alpha, float w_overlap) {
  HPRI_REQUIRE(n_img > 0 && hw > 0, "seg_loss: bad sizes");
  HPRI_REQUIRE(pos_weight > 0.f, "seg_loss: pos_weight must be positive");
  HPRI_REQUIRE(focal_gamma >= 0.f, "seg_loss: focal gamma must not be negative");
  HPRI_REQUIRE(focal_alpha <= 1.f, "seg_loss: focal alpha must lie in [0, 1] (negative: none)");
  HPRI_REQUIRE(w_point == w_point && w_overlap == w_overlap && (w_point != 0.f || w_overlap != 0.f),
               "seg_loss: both weights are zero (or one is NaN): nothing to compute");
  return HPRI_OK;
}

extern "C" size_t hpri_seg_loss_workspace_doubles(int n_img, long long hw) {
  if (n_img <= 0 || hw <= 0) return 0;
  return 4 * (size_t)n_img * (size_t)sl_bpi(n_img, hw);
}

extern "C" size_t hpri_seg_loss_state_doubles(int n_img, int per_image) {
  if (n_img <= 0) return 0;
  return 1 + 2 * (size_t)(per_image ? n_img : 1);
}

#define SL_DISPATCH(KERNEL, ...)                                                                                              \
  do {                                                                                                                        \
    const int point__ = w_point != 0.f, focal__ = focal_gamma != 0.f || focal_alpha >= 0.f, over__ = w_overlap != 0.f;        \
    if (point__ && over__) { if (focal__) SL_LAUNCH(KERNEL, 1, 1, 1, __VA_ARGS__); else SL_LAUNCH(KERNEL, 1, 0, 1, __VA_ARGS__); } \
    else if (point__) { if (focal__) SL_LAUNCH(KERNEL, 1, 1, 0, __VA_ARGS__); else SL_LAUNCH(KERNEL, 1, 0, 0, __VA_ARGS__); }      \
    else SL_LAUNCH(KERNEL, 0, 0, 1, __VA_ARGS__);                                                                             \
  } while (0)
#define SL_LAUNCH(KERNEL, P, F, O, ...) \
  hipLaunchKernelGGL((KERNEL<P, F, O>), dim3(hpri_grid_capped(units, 1)), dim3(SL_THREADS), 0, stream, __VA_ARGS__)

extern "C" int hpri_seg_loss_fwd(const float* logits, const float* target, int n_img, long long hw, float w_point, float pos_weight,
                                 float focal_gamma, float focal_alpha, int mean, float w_overlap, float tversky_alpha,
                                 float tversky_beta, float smooth, float tversky_gamma, int per_image, float* loss, double* state,
                                 size_t state_doubles, float* terms, double* workspace, size_t ws_doubles, hipStream_t stream) {
  HPRI_REQUIRE(logits && target && loss && state && terms && workspace, "seg_loss_fwd: null pointer");
  if (int rc = sl_check(n_img, hw, w_point, pos_weight, focal_gamma, focal_alpha, w_overlap)) return rc;
  HPRI_REQUIRE(tversky_alpha >= 0.f && tversky_beta >= 0.f, "seg_loss_fwd: tversky alpha and beta must not be negative");
  HPRI_REQUIRE(tversky_alpha + tversky_beta > 0.f, "seg_loss_fwd: tversky alpha + beta must be positive");
  HPRI_REQUIRE(smooth >= 0.f, "seg_loss_fwd: smooth must not be negative");
  HPRI_REQUIRE(tversky_gamma > 0.f, "seg_loss_fwd: tversky gamma must be positive");
  const int bpi = sl_bpi(n_img, hw);
  const long long units = (long long)n_img * bpi;
  if (4 * (size_t)units > ws_doubles) return hpri_set_error(HPRI_ERR_WORKSPACE, "seg_loss_fwd: workspace too small");
  if (hpri_seg_loss_state_doubles(n_img, per_image) > state_doubles) return hpri_set_error(HPRI_ERR_WORKSPACE, "seg_loss_fwd: state buffer too small");
  const int vec = hw % 4 == 0 && hpri_aligned16(logits, target);
  const SlPoint pc = {pos_weight, focal_gamma, focal_alpha};
  SL_DISPATCH(seg_loss_fwd_kernel, logits, target, hw, bpi, units, vec, pc, workspace);
  HPRI_CHECK_LAUNCH();
  const SlOverlap oc = {(double)w_overlap, (double)tversky_alpha, (double)tversky_beta, (double)smooth, (double)tversky_gamma};
  hipLaunchKernelGGL(seg_loss_finalize_kernel, dim3(1), dim3(SL_THREADS), 0, stream, workspace, units, bpi, per_image ? n_img : 1,
                     per_image ? 1 : 0, (double)w_point, (double)n_img * (double)hw, mean, oc, loss, state, terms);
  HPRI_CHECK_LAUNCH();
  return HPRI_OK;
}

extern "C" int hpri_seg_loss_bwd(const float* logits, const float* target, int n_img, long long hw, float w_point, float pos_weight,
                                 float focal_gamma, float focal_alpha, float w_overlap, int per_image, const double* state,
                                 size_t state_doubles, const float* grad_out, float* dlogits, hipStream_t stream) {
  HPRI_REQUIRE(logits && target && state && dlogits, "seg_loss_bwd: null pointer");
  if (int rc = sl_check(n_img, hw, w_point, pos_weight, focal_gamma, focal_alpha, w_overlap)) return rc;
  // (a per_image or n_img other than the forward's would read past the forward's buffer)
  if (hpri_seg_loss_state_doubles(n_img, per_image) > state_doubles) return hpri_set_error(HPRI_ERR_WORKSPACE, "seg_loss_bwd: state buffer too small");
  const int bpi = sl_bpi(n_img, hw);
  const long long units = (long long)n_img * bpi;
  const int vec = hw % 4 == 0 && hpri_aligned16(logits, target, dlogits);
  const SlPoint pc = {pos_weight, focal_gamma, focal_alpha};
  SL_DISPATCH(seg_loss_bwd_kernel, logits, target, hw, bpi, units, vec, pc, per_image ? 1 : 0, state, grad_out, dlogits);
  HPRI_CHECK_LAUNCH();
  return HPRI_OK;
}
#undef SL_DISPATCH
#undef SL_LAUNCH
