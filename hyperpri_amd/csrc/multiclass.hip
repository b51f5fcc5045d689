// The caller-side tail of a MULTI-CLASS step: what step.hip does for one logit per pixel, for K class planes per pixel --
//   * nn.CrossEntropyLoss(weight, ignore_index, reduction) forward (softmax_ce_fwd_kernel + softmax_ce_finalize_kernel) and its
//     gradient (softmax_ce_bwd_kernel),
//   * pred = argmax over the class planes and the K x K confusion matrix every multi-class metric reduces to
//     (seg_confusion_kernel), optionally the uint8 class map itself.
// Logits are contiguous NCHW fp32 (N, K, h, w): class plane k of image n starts at (n*K + k)*HW.  Targets hold one class index
// per pixel as fp32 (what CubeCache emits; truncated toward zero like mask.to(int)), uint8 or int64.
//
// All kernels are HBM-bound single passes (forward 4K + 8 bytes per pixel, backward 8K + 8): a lane owns four adjacent pixels of
// one image and walks the K planes, so a wave reads 1 KB contiguous per plane -- 16-byte accesses when HW % 4 == 0 and every base
// pointer is 16-byte aligned (hpri_load4 / hpri_store4), element accesses otherwise; which lane owns which pixel is the same
// in both forms, so their results are bit-identical.  As in step.hip: fixed-order fp64 partial sums, integer atomics only, no
// host synchronisation (scalars stay on the device), nothing allocated here.
//
// A target is VALID (0 <= t < K), IGNORED (use_ignore and t == ignore_index: contributes nothing, gradient exactly 0) or INVALID
// (anything else, a NaN / out-of-range fp32 value included).  The class of a pixel is never used as an index before that
// check -- the class's logit is picked by a select while the planes stream past, only the weight is read at [t].  An invalid
// target cannot be reported without a synchronisation, so it POISONS the result instead: the loss becomes NaN (gradient rows of
// such pixels are zero), the confusion pass counts it in counts[K*K].
#include "tail_helpers.h"

#define MC_THREADS 256
#define MC_MAX_K 64
enum { MC_T_F32 = 0, MC_T_U8 = 1, MC_T_I64 = 2 };
enum { MC_VALID = 0, MC_IGNORED = 1, MC_INVALID = 2 };

static inline int mc_blocks(long long items) { return hpri_grid_capped(items, MC_THREADS); }

struct McQuad {                 // four adjacent pixels of one image
  long long plane0;             // element offset of class plane 0 at the quad's first pixel
  long long pix;                // n*HW + first pixel: offset into (N, HW) arrays
  int cnt;                      // 1..4 pixels (the image's last quad may be short)
};

__device__ __forceinline__ McQuad mc_quad(long long it, long long qpi, long long HW, int K) {
  const long long n = it / qpi, p0 = (it - n * qpi) * 4;
  McQuad q;
  q.plane0 = n * K * HW + p0;
  q.pix = n * HW + p0;
  q.cnt = HW - p0 < 4 ? (int)(HW - p0) : 4;
  return q;
}

__device__ __forceinline__ void mc_classify(long long v, int K, int use_ignore, long long ignore_index, int& cls, int& state) {
  if (use_ignore && v == ignore_index) { cls = 0; state = MC_IGNORED; }
  else if (v < 0 || v >= K) { cls = 0; state = MC_INVALID; }
  else { cls = (int)v; state = MC_VALID; }
}

// the quad's targets: class (0 unless valid) and state per pixel; pixels past cnt are IGNORED
__device__ __forceinline__ void mc_targets(const void* __restrict__ target, int tkind, long long pix, int cnt, int vec, int K,
                                           int use_ignore, long long ignore_index, int (&cls)[4], int (&state)[4]) {
  long long v[4];
  bool bad[4] = {false, false, false, false};
  if (tkind == MC_T_F32) {
    float f[4];
    hpri_load4(reinterpret_cast<const float*>(target) + pix, cnt, vec, f);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      bad[j] = !(f[j] > -2147483648.f && f[j] < 2147483648.f);      // NaN, infinities, beyond any class index
      v[j] = bad[j] ? 0 : (long long)(int)f[j];
    }
  } else if (tkind == MC_T_U8) {
    const unsigned char* t = reinterpret_cast<const unsigned char*>(target) + pix;
    if (vec) {
      const unsigned w = *reinterpret_cast<const unsigned*>(t);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = (w >> (8 * j)) & 255u;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = j < cnt ? t[j] : 0;
    }
  } else {
    const long long* t = reinterpret_cast<const long long*>(target) + pix;
    typedef long long i64x2 __attribute__((ext_vector_type(2)));
    if (vec) {
      const i64x2 a = *reinterpret_cast<const i64x2*>(t), b = *reinterpret_cast<const i64x2*>(t + 2);
      v[0] = a[0]; v[1] = a[1]; v[2] = b[0]; v[3] = b[1];
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = j < cnt ? t[j] : 0;
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    mc_classify(v[j], K, use_ignore, ignore_index, cls[j], state[j]);
    if (bad[j]) { cls[j] = 0; state[j] = MC_INVALID; }
    if (j >= cnt) { cls[j] = 0; state[j] = MC_IGNORED; }
  }
}

// ------------------------------------------------------------------------------------------------
// Cross-entropy forward.  Per pixel, one walk over the planes with a running maximum m and s = sum exp(x - m) (one expf per
// element: e = exp(-|x - m|) rescales s when x is the new maximum, is the new term otherwise):
//   lse = m + log(s);   l = w[t] * (lse - x_t)
// lse goes out for the backward; partial[b], partial[nb + b], partial[2 nb + b] = this block's fp64 sums of l, of w[t] over the
// valid pixels and of the invalid-target count (fixed slice per block, fixed tree: bit-reproducible).
// ------------------------------------------------------------------------------------------------
template <int KT>
__global__ __launch_bounds__(MC_THREADS) void softmax_ce_fwd_kernel(const float* __restrict__ x, const void* __restrict__ target,
                                                                    int tkind, const float* __restrict__ weight, int N, int Krt,
                                                                    long long HW, int use_ignore, long long ignore_index, int vec,
                                                                    float* __restrict__ lse, double* __restrict__ partial) {
  const int K = KT > 0 ? KT : Krt;
  __shared__ double red[3][MC_THREADS];
  const long long qpi = (HW + 3) >> 2, items = (long long)N * qpi;
  double sl = 0.0, sw = 0.0, sb = 0.0;
  for (long long it = (long long)blockIdx.x * MC_THREADS + threadIdx.x; it < items; it += (long long)gridDim.x * MC_THREADS) {
    const McQuad q = mc_quad(it, qpi, HW, K);
    int cls[4], state[4];
    mc_targets(target, tkind, q.pix, q.cnt, vec, K, use_ignore, ignore_index, cls, state);
    float m[4], s[4], xt[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { m[j] = -INFINITY; s[j] = 0.f; xt[j] = 0.f; }
    const float* px = x + q.plane0;
    constexpr int UNROLL = KT > 0 ? KT : 4;
#pragma unroll UNROLL
    for (int k = 0; k < K; ++k) {
      float v[4];
      hpri_load4(px + (long long)k * HW, q.cnt, vec, v);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float d = v[j] - m[j];
        const float e = expf(-fabsf(d));
        s[j] = d > 0.f ? s[j] * e + 1.f : s[j] + e;
        m[j] = fmaxf(m[j], v[j]);
        xt[j] = k == cls[j] ? v[j] : xt[j];
      }
    }
    float o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      o[j] = m[j] + logf(s[j]);
      if (state[j] == MC_VALID) {
        const float w = weight ? weight[cls[j]] : 1.f;
        sl += (double)(w * (o[j] - xt[j]));
        sw += (double)w;
      } else if (state[j] == MC_INVALID) {
        sb += 1.0;
      }
    }
    hpri_store4(lse + q.pix, q.cnt, vec, o);
  }
  const double s3[3] = {sl, sw, sb};
  hpri_block_sum(red, s3);
  if (threadIdx.x < 3) partial[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = red[threadIdx.x][0];
}

// loss = mean ? sum l / sum w : sum l (NaN when any target was invalid; 0 / 0 = NaN for an all-ignored mean, as torch);
// denom[0] = the divisor the backward uses; totals (nullable): totals[0] += sum l, totals[1] += sum w, totals[2] += invalid count
__global__ __launch_bounds__(MC_THREADS) void softmax_ce_finalize_kernel(const double* __restrict__ partial, int nblk, int mean,
                                                                         float* __restrict__ loss, float* __restrict__ denom,
                                                                         double* __restrict__ totals) {
  __shared__ double red[3][MC_THREADS];
  double s[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int r = 0; r < 3; ++r)
    for (int i = threadIdx.x; i < nblk; i += MC_THREADS) s[r] += partial[(size_t)r * nblk + i];
  hpri_block_sum(red, s);
  if (threadIdx.x == 0) {
    const double sl = red[0][0], sw = red[1][0], sb = red[2][0];
    const double l = mean ? sl / sw : sl;
    loss[0] = sb > 0.0 ? __builtin_nanf("") : (float)l;
    denom[0] = mean ? (float)sw : 1.f;
    if (totals) { totals[0] += sl; totals[1] += sw; totals[2] += sb; }
  }
}

// ------------------------------------------------------------------------------------------------
// Cross-entropy backward: with p_k = exp(x_k - lse) and c = w[t] * (g / denom),
//   dx_k = p_k * c (k != t);   dx_t = -(sum over j != t of p_j) * c
// -- not (p_t - 1) * c: a confident correct pixel has p_t one ulp from 1 and would keep no relative accuracy (bce_bwd_kernel
// uses sigmoid(-x) for the same reason).  The K fixed at compile time keep their 4 K probabilities in registers: one walk over the
// planes; a runtime K walks them twice (the second walk finds the quad's lines in cache: they were just read).
// ------------------------------------------------------------------------------------------------
template <int KT>
__global__ __launch_bounds__(MC_THREADS) void softmax_ce_bwd_kernel(const float* __restrict__ x, const float* __restrict__ lse,
                                                                    const void* __restrict__ target, int tkind,
                                                                    const float* __restrict__ weight, int N, int Krt, long long HW,
                                                                    int use_ignore, long long ignore_index, int vec,
                                                                    const float* __restrict__ denom, const float* __restrict__ gout,
                                                                    float* __restrict__ dx) {
  const int K = KT > 0 ? KT : Krt;
  const float scale = (gout ? gout[0] : 1.f) / denom[0];
  const long long qpi = (HW + 3) >> 2, items = (long long)N * qpi;
  for (long long it = (long long)blockIdx.x * MC_THREADS + threadIdx.x; it < items; it += (long long)gridDim.x * MC_THREADS) {
    const McQuad q = mc_quad(it, qpi, HW, K);
    int cls[4], state[4];
    mc_targets(target, tkind, q.pix, q.cnt, vec, K, use_ignore, ignore_index, cls, state);
    float l[4], c[4], others[4];
    hpri_load4(lse + q.pix, q.cnt, vec, l);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      // (an ignored or invalid pixel: exact zeros, whatever g / denom is -- 0 * inf would be NaN)
      c[j] = state[j] == MC_VALID ? (weight ? weight[cls[j]] : 1.f) * scale : 0.f;
      others[j] = 0.f;
    }
    const float* px = x + q.plane0;
    float* pd = dx + q.plane0;
    if constexpr (KT > 0) {
      float p[KT][4];
#pragma unroll
      for (int k = 0; k < KT; ++k) {
        float v[4];
        hpri_load4(px + (long long)k * HW, q.cnt, vec, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          p[k][j] = expf(v[j] - l[j]);
          others[j] += k == cls[j] ? 0.f : p[k][j];
        }
      }
#pragma unroll
      for (int k = 0; k < KT; ++k) {
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = state[j] == MC_VALID ? (k == cls[j] ? -others[j] : p[k][j]) * c[j] : 0.f;
        hpri_store4(pd + (long long)k * HW, q.cnt, vec, o);
      }
    } else {
#pragma unroll 4
      for (int k = 0; k < K; ++k) {
        float v[4];
        hpri_load4(px + (long long)k * HW, q.cnt, vec, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) others[j] += k == cls[j] ? 0.f : expf(v[j] - l[j]);
      }
#pragma unroll 4
      for (int k = 0; k < K; ++k) {
        float v[4], o[4];
        hpri_load4(px + (long long)k * HW, q.cnt, vec, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = state[j] == MC_VALID ? (k == cls[j] ? -others[j] : expf(v[j] - l[j])) * c[j] : 0.f;
        hpri_store4(pd + (long long)k * HW, q.cnt, vec, o);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// pred = argmax over the planes as torch.argmax decides it: the lowest index among equal maxima, a NaN counts as the maximum
// (the first one wins).  hist[t*K + p] counts the block's pixels in LDS (uint32, at most 16 KB; the four pixels of a lane that
// fall into one cell are added at once), then goes to counts[] (int64, accumulated across calls like hpri_seg_counts);
// counts[K*K] counts invalid targets, ignored pixels are skipped.  classes (nullable): the uint8 class map.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MC_THREADS) void seg_confusion_kernel(const float* __restrict__ x, const void* __restrict__ target,
                                                                   int tkind, int N, int K, long long HW, int use_ignore,
                                                                   long long ignore_index, int vec,
                                                                   unsigned long long* __restrict__ counts,
                                                                   unsigned char* __restrict__ classes) {
  __shared__ unsigned hist[MC_MAX_K * MC_MAX_K + 1];
  const int cells = K * K + 1;
  if (counts) {
    for (int i = threadIdx.x; i < cells; i += MC_THREADS) hist[i] = 0;
    __syncthreads();
  }
  const long long qpi = (HW + 3) >> 2, items = (long long)N * qpi;
  for (long long it = (long long)blockIdx.x * MC_THREADS + threadIdx.x; it < items; it += (long long)gridDim.x * MC_THREADS) {
    const McQuad q = mc_quad(it, qpi, HW, K);
    float best[4];
    int arg[4];
    const float* px = x + q.plane0;
    hpri_load4(px, q.cnt, vec, best);
#pragma unroll
    for (int j = 0; j < 4; ++j) arg[j] = 0;
#pragma unroll 4
    for (int k = 1; k < K; ++k) {
      float v[4];
      hpri_load4(px + (long long)k * HW, q.cnt, vec, v);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool take = v[j] > best[j] || (v[j] != v[j] && best[j] == best[j]);
        best[j] = take ? v[j] : best[j];
        arg[j] = take ? k : arg[j];
      }
    }
    if (classes) {
      unsigned char* pc = classes + q.pix;
      if (vec) {
        *reinterpret_cast<unsigned*>(pc) = (unsigned)arg[0] | ((unsigned)arg[1] << 8) | ((unsigned)arg[2] << 16) | ((unsigned)arg[3] << 24);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < q.cnt) pc[j] = (unsigned char)arg[j];
      }
    }
    if (counts) {
      int cls[4], state[4], cell[4];
      mc_targets(target, tkind, q.pix, q.cnt, vec, K, use_ignore, ignore_index, cls, state);
#pragma unroll
      for (int j = 0; j < 4; ++j) cell[j] = state[j] == MC_VALID ? cls[j] * K + arg[j] : state[j] == MC_INVALID ? K * K : -1;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        bool seen = false;
        unsigned n = 1;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (i < j) seen = seen || cell[i] == cell[j];
          if (i > j) n += cell[i] == cell[j];
        }
        if (cell[j] >= 0 && !seen) atomicAdd(&hist[cell[j]], n);
      }
    }
  }
  if (counts) {
    __syncthreads();
    for (int i = threadIdx.x; i < cells; i += MC_THREADS)
      if (hist[i]) atomicAdd(&counts[i], (unsigned long long)hist[i]);
  }
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
static int mc_check(const char* who, int tkind, int N, int K, long long HW) {
  (void)who;
  HPRI_REQUIRE(K >= 2 && K <= MC_MAX_K, "multiclass: the number of classes must lie in [2, 64]");
  HPRI_REQUIRE(N > 0 && HW > 0, "multiclass: bad sizes");
  HPRI_REQUIRE(tkind == MC_T_F32 || tkind == MC_T_U8 || tkind == MC_T_I64, "multiclass: target kind must be 0 (fp32), 1 (uint8) or 2 (int64)");
  return HPRI_OK;
}

// (an upper bound for every (N, HW) with N*HW = npix: a quad holds at least one pixel)
extern "C" size_t hpri_softmax_ce_workspace_doubles(long long npix) { return 3 * (size_t)mc_blocks(npix); }

extern "C" int hpri_softmax_ce_fwd(const float* logits, const void* target, int target_kind, const float* weight, int N, int K,
                                   long long HW, int use_ignore, long long ignore_index, int mean, float* loss, float* lse,
                                   float* denom, double* totals, double* workspace, size_t ws_doubles, hipStream_t stream) {
  HPRI_REQUIRE(logits && target && loss && lse && denom && workspace, "softmax_ce_fwd: null pointer");
  if (int rc = mc_check("softmax_ce_fwd", target_kind, N, K, HW)) return rc;
  const long long items = (long long)N * ((HW + 3) / 4);
  const int nb = mc_blocks(items);
  if (3 * (size_t)nb > ws_doubles) return hpri_set_error(HPRI_ERR_WORKSPACE, "softmax_ce_fwd: workspace too small");
  const int vec = HW % 4 == 0 && hpri_aligned16(logits, target, lse);
#define MC_FWD(KT)                                                                                                              \
  hipLaunchKernelGGL(softmax_ce_fwd_kernel<KT>, dim3(nb), dim3(MC_THREADS), 0, stream, logits, target, target_kind, weight, N, K, \
                     HW, use_ignore, ignore_index, vec, lse, workspace)
  if (K == 2) MC_FWD(2); else if (K == 3) MC_FWD(3); else if (K == 4) MC_FWD(4); else MC_FWD(0);
#undef MC_FWD
  HPRI_CHECK_LAUNCH();
  hipLaunchKernelGGL(softmax_ce_finalize_kernel, dim3(1), dim3(MC_THREADS), 0, stream, workspace, nb, mean, loss, denom, totals);
  HPRI_CHECK_LAUNCH();
  return HPRI_OK;
}

extern "C" int hpri_softmax_ce_bwd(const float* logits, const float* lse, const void* target, int target_kind, const float* weight,
                                   int N, int K, long long HW, int use_ignore, long long ignore_index, const float* denom,
                                   const float* grad_out, float* dlogits, hipStream_t stream) {
  HPRI_REQUIRE(logits && lse && target && denom && dlogits, "softmax_ce_bwd: null pointer");
  if (int rc = mc_check("softmax_ce_bwd", target_kind, N, K, HW)) return rc;
  const long long items = (long long)N * ((HW + 3) / 4);
  const int nb = mc_blocks(items);
  const int vec = HW % 4 == 0 && hpri_aligned16(logits, target, lse, dlogits);
#define MC_BWD(KT)                                                                                                              \
  hipLaunchKernelGGL(softmax_ce_bwd_kernel<KT>, dim3(nb), dim3(MC_THREADS), 0, stream, logits, lse, target, target_kind, weight, \
                     N, K, HW, use_ignore, ignore_index, vec, denom, grad_out, dlogits)
  if (K == 2) MC_BWD(2); else if (K == 3) MC_BWD(3); else if (K == 4) MC_BWD(4); else MC_BWD(0);
#undef MC_BWD
  HPRI_CHECK_LAUNCH();
  return HPRI_OK;
}

extern "C" int hpri_seg_confusion(const float* logits, const void* target, int target_kind, int N, int K, long long HW,
                                  int use_ignore, long long ignore_index, long long* counts, unsigned char* classes,
                                  hipStream_t stream) {
  HPRI_REQUIRE(logits, "seg_confusion: null pointer");
  HPRI_REQUIRE((target != nullptr) == (counts != nullptr), "seg_confusion: target and counts come together (null: class map only)");
  HPRI_REQUIRE(counts || classes, "seg_confusion: null pointer (neither counts nor a class map asked for)");
  if (int rc = mc_check("seg_confusion", target ? target_kind : MC_T_F32, N, K, HW)) return rc;
  const long long items = (long long)N * ((HW + 3) / 4);
  const int vec = HW % 4 == 0 && hpri_aligned16(logits, target, classes);
  hipLaunchKernelGGL(seg_confusion_kernel, dim3(mc_blocks(items)), dim3(MC_THREADS), 0, stream, logits, target, target_kind, N, K, HW,
                     use_ignore, ignore_index, vec, reinterpret_cast<unsigned long long*>(counts), classes);
  HPRI_CHECK_LAUNCH();
  return HPRI_OK;
}
