// Soft skeletons and the centerline loss clDice (Shit et al., CVPR 2021) for thin roots.
//
//   E(I)[u] = min of I over the in-image part of the plus neighbourhood {N, W, C, E, S} of u
//   D(I)[u] = max of I over the in-image part of the 3x3 neighbourhood of u
//   I_0 = p,  I_{j+1} = E(I_j),  d_j = I_j - D(I_{j+1})                       j = 0 .. iters
//   S_0 = relu(d_0),  S_j = S_{j-1} + relu(fma(-S_{j-1}, d_j, d_j))           j = 1 .. iters;     soft_skeleton(p, iters) = S_iters
//
// the published soft_skel (soft_open = dilate o erode, skel += relu(delta - skel * delta)) on fp32 planes (N, h, w).  Every I_j is a
// copy of input values (min and max select), d_j >= 0, and a level rounds three times: the subtraction, the fma, the add.
//
// Forward: ONE launch for all levels (soft_skel_fwd_kernel).  A workgroup owns a SK_T x SK_T tile, stages it with a halo of
// iters + 2 in LDS, ping-pongs the erosions between two LDS planes and keeps S in registers (16 pixels of one column per lane, so the
// 3x3 maximum slides down the column: 3 LDS reads per pixel and level).  Cells outside the image hold NaN in both planes and are
// never written: fminf / fmaxf return their other operand, which is "the in-image part of the neighbourhood".  For the backward the
// launch leaves I_1 .. I_{iters+1} and S_0 .. S_{iters-1} of the tile's interior ("saved": 2 iters + 1 planes).  Two image lists go
// through one launch: the first may be logits (the sigmoid is applied as the tile is loaded, in the exp(-|x|) form of hpri_sigmoids,
// and written once), the second is never saved -- the prediction and the target of the loss.
//
// Backward: one launch per level, j = iters .. 0 (soft_skel_bwd_kernel), carrying gS (gradient wrt S_j) and gE (wrt I_{j+1}):
//   t_j = fma(-S_{j-1}, d_j, d_j)
//   gd  = gS * (1 - S_{j-1}) * [t_j > 0]                 (j = 0: S_{-1} = 0)
//   gS <- gS * (1 - d_j * [t_j > 0])
//   gI_j = gd + route_E(gE + route_D(-gd)),   gE <- gI_j
// A min or a max sends its whole gradient to the FIRST optimum in scan order (E: N, W, C, E, S; D: the 3x3 window row by row), and
// the routes are GATHERS: a pixel sums, in that fixed order and in fp64 (rounded once), what the neighbours whose recomputed argmin or
// argmax it is send.  No floating-point atomic anywhere; the bits do not depend on the tiling or on the run.  A workgroup owns a
// SK_BT x SK_BT tile and stages I_j and I_{j+1} with a halo of 3 (gd is needed two pixels out, and it reads D(I_{j+1}) one further).
//
// clDice:  Sp = soft_skeleton(sigmoid(x)), Sy = soft_skeleton(y);  per group g (an image, or the batch)
//   tprec = (sum Sp*y + s) / (sum Sp + s),  tsens = (sum Sy*p + s) / (sum Sy + s),  cl = 1 - 2 tprec tsens / (tprec + tsens)
// The forward launch leaves two fp64 partial sums per workgroup (reduced through LDS in a fixed order), cldice_finalize_kernel adds
// them in a fixed order and leaves the loss, the diagnostics and per group the coefficients a, b, c of
//   gSp[u] = a y[u] + b,   direct gp[u] = c Sy[u],   dx = g (skeleton-backward(gSp) + gp) sigmoid(x) sigmoid(-x)
// which the first and the last level launch of the backward read from device memory: no host round trip.  Edge rules: a ratio with
// a zero denominator (s = 0 and an empty skeleton) is 0 with zero coefficients; tprec + tsens == 0 gives cl = 1, zero coefficients.
#include "tail_helpers.h"
#include <math.h>

#define SK_T 64                      // forward tile
#define SK_THREADS 256
#define SK_ROWS (SK_T * SK_T / SK_THREADS)      // pixels of one column a lane owns
#define SK_MAX_ITERS 32
#define SK_BT 32                     // backward tile
#define SK_BH 3                      // its halo
#define SK_BL (SK_BT + 2 * SK_BH)
#define SK_BCELLS (SK_BL * SK_BL)
#define SK_NONE 255

// ------------------------------------------------------------------------------------------------
// Forward
// ------------------------------------------------------------------------------------------------
struct SkFwd {
  const float* src0; const float* src1;      // n0 and n1 images; src0 holds logits with sig0
  float* p_out;                              // sigmoid(src0) (sig0; may be null)
  float* S0; float* S1;                      // the skeletons (either may be null)
  float* saved;                              // null: nothing saved; else (2 iters + 1) planes of n0 images
  const float* other0; const float* other1;  // with partial: the factor of the first sum (src1 images: logits, sigmoid applied)
  double* partial;                           // [image][tile][2]: sum S * other, sum S
  int n0, n1, sig0, h, w, iters, tiles_x;
};

__global__ __launch_bounds__(SK_THREADS) void soft_skel_fwd_kernel(SkFwd a) {
  extern __shared__ double sk_lds_d[];
  float* A = reinterpret_cast<float*>(sk_lds_d);
  const int H = a.iters + 2, L = SK_T + 2 * H;
  float* B = A + L * L;
  const int img = blockIdx.y, tile = blockIdx.x;
  const bool first = img < a.n0;
  const int tyi = tile / a.tiles_x, txi = tile - tyi * a.tiles_x;
  const int y0 = tyi * SK_T, x0 = txi * SK_T;
  const size_t plane = (size_t)a.h * a.w, np0 = plane * a.n0;
  const size_t ioff = (size_t)(first ? img : img - a.n0) * plane;
  const float* src = (first ? a.src0 : a.src1) + ioff;
  const bool sig = first && a.sig0;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float qnan = __builtin_nanf("");

  for (int r = wave; r < L; r += SK_THREADS / 64) {
    const int gy = y0 - H + r;
    const bool rowin = gy >= 0 && gy < a.h;
    for (int c = lane; c < L; c += 64) {
      const int gx = x0 - H + c;
      float v = qnan;
      if (rowin && gx >= 0 && gx < a.w) {
        v = src[(size_t)gy * a.w + gx];
        if (sig) {
          float sp, sn;
          hpri_sigmoids(v, sp, sn);
          v = sp;
          if (a.p_out && r >= H && r < H + SK_T && c >= H && c < H + SK_T) a.p_out[ioff + (size_t)gy * a.w + gx] = v;
        }
      }
      A[r * L + c] = v;
      B[r * L + c] = qnan;
    }
  }
  // the in-image rectangle in LDS coordinates: nothing outside it is ever written
  const int rlo = max(0, H - y0), rhi = min(L - 1, H + a.h - 1 - y0);
  const int clo = max(0, H - x0), chi = min(L - 1, H + a.w - 1 - x0);
  const int cc = H + lane, rr0 = H + wave * SK_ROWS;       // this lane's column and first row
  const int gx = x0 + lane, gy0 = y0 + wave * SK_ROWS;
  const bool colin = gx < a.w;
  float* save = first ? a.saved : nullptr;
  float S[SK_ROWS];
#pragma unroll
  for (int k = 0; k < SK_ROWS; ++k) S[k] = 0.f;

  for (int j = 0; j <= a.iters; ++j) {
    __syncthreads();                                       // A is complete, and the last level's reads of B's cells are over
    const int r0 = max(j + 1, rlo), r1 = min(L - 2 - j, rhi), c0 = max(j + 1, clo), c1 = min(L - 2 - j, chi);
    for (int r = r0 + wave; r <= r1; r += SK_THREADS / 64)
      for (int c = c0 + lane; c <= c1; c += 64) {
        const float* q = A + r * L + c;
        B[r * L + c] = fminf(fminf(fminf(q[-L], q[-1]), fminf(q[0], q[1])), q[L]);
      }
    __syncthreads();
    const float* b = B + (rr0 - 1) * L + cc;
    float hprev = fmaxf(fmaxf(b[-1], b[0]), b[1]);
    b += L;
    float mid = b[0];
    float hcur = fmaxf(fmaxf(b[-1], mid), b[1]);
    float* sI = save ? save + (size_t)j * np0 + ioff : nullptr;                            // I_{j+1}
    float* sS = save && j > 0 ? save + (size_t)(a.iters + j) * np0 + ioff : nullptr;       // S_{j-1}
#pragma unroll
    for (int k = 0; k < SK_ROWS; ++k) {
      b += L;
      const float nmid = b[0];
      const float hnext = fmaxf(fmaxf(b[-1], nmid), b[1]);
      const float d = A[(rr0 + k) * L + cc] - fmaxf(fmaxf(hprev, hcur), hnext);
      const bool in = colin && gy0 + k < a.h;
      const size_t g = (size_t)(gy0 + k) * a.w + gx;
      if (in && sI) sI[g] = mid;
      if (in && sS) sS[g] = S[k];
      S[k] = j == 0 ? fmaxf(d, 0.f) : S[k] + fmaxf(fmaf(-S[k], d, d), 0.f);
      hprev = hcur; hcur = hnext; mid = nmid;
    }
    float* t = A; A = B; B = t;
  }

  float* So = first ? a.S0 : a.S1;
  double s0 = 0.0, s1 = 0.0;
  const float* other = first ? a.other0 : a.other1;
#pragma unroll
  for (int k = 0; k < SK_ROWS; ++k) {
    if (colin && gy0 + k < a.h) {
      const size_t g = ioff + (size_t)(gy0 + k) * a.w + gx;
      if (So) So[g] = S[k];
      if (a.partial) {
        float o = other[g];
        if (!first) { float sp, sn; hpri_sigmoids(o, sp, sn); o = sp; }
        s0 += (double)S[k] * (double)o;
        s1 += (double)S[k];
      }
    }
  }
  if (a.partial) {
    __syncthreads();                                       // the planes are done with
    double (*red)[SK_THREADS] = reinterpret_cast<double (*)[SK_THREADS]>(sk_lds_d);      // two rows; the planes are far larger
    const double s2[2] = {s0, s1};
    hpri_block_sum(red, s2);
    if (threadIdx.x < 2) a.partial[((size_t)img * gridDim.x + tile) * 2 + threadIdx.x] = red[threadIdx.x][0];
  }
}

// ------------------------------------------------------------------------------------------------
// clDice finalize: one workgroup, fp64.  Wave w takes groups w, w + 4, ...; its lanes stride over the group's (image, tile) partials
// of the prediction (images [0, N)) and of the target (images [N, 2N)), a xor-butterfly leaves the sums in every lane.
//   loss[0] = weight * mean_g cl_g (+ base_weight * base_loss[0]);  terms[0..2] = mean cl, mean tprec, mean tsens
//   state[3g .. 3g+2] = a_g, b_g, c_g (weight / G folded in)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SK_THREADS) void cldice_finalize_kernel(const double* __restrict__ partial, int N, int tiles, int groups,
                                                                     int per_image, double s, double weight, const float* base_loss,
                                                                     double base_weight, float* __restrict__ loss,
                                                                     double* __restrict__ state, float* __restrict__ terms) {
  __shared__ double wsum[3][SK_THREADS / 64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double accl = 0.0, accp = 0.0, accs = 0.0;
  for (int g = wave; g < groups; g += SK_THREADS / 64) {
    const long long cnt = per_image ? tiles : (long long)N * tiles, u0 = per_image ? (long long)g * tiles : 0;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (long long u = lane; u < cnt; u += 64) {
      const double* pp = partial + (size_t)(u0 + u) * 2;
      const double* pt = partial + (size_t)((long long)N * tiles + u0 + u) * 2;
      v[0] += pp[0]; v[1] += pp[1]; v[2] += pt[0]; v[3] += pt[1];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = hpri_wave_sum(v[r]);
    const double dp = v[1] + s, dt = v[3] + s;
    const double tp = dp == 0.0 ? 0.0 : (v[0] + s) / dp, ts = dt == 0.0 ? 0.0 : (v[2] + s) / dt;
    const double sum = tp + ts;
    double cl = 1.0, ca = 0.0, cb = 0.0, cc = 0.0;
    if (sum != 0.0) {
      cl = 1.0 - 2.0 * tp * ts / sum;
      const double k = weight / (double)groups, dtp = -2.0 * ts * ts / (sum * sum), dts = -2.0 * tp * tp / (sum * sum);
      if (dp != 0.0) { ca = k * dtp / dp; cb = -k * dtp * (v[0] + s) / (dp * dp); }
      if (dt != 0.0) cc = k * dts / dt;
    }
    accl += cl; accp += tp; accs += ts;
    if (lane == 0) { state[3 * (size_t)g] = ca; state[3 * (size_t)g + 1] = cb; state[3 * (size_t)g + 2] = cc; }
  }
  if (lane == 0) { wsum[0][wave] = accl; wsum[1][wave] = accp; wsum[2][wave] = accs; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double l = 0.0, p = 0.0, t = 0.0;
    for (int w = 0; w < SK_THREADS / 64; ++w) { l += wsum[0][w]; p += wsum[1][w]; t += wsum[2][w]; }
    l /= (double)groups;
    double out = weight * l;
    if (base_loss) out += base_weight * (double)base_loss[0];
    loss[0] = (float)out;
    terms[0] = (float)l; terms[1] = (float)(p / (double)groups); terms[2] = (float)(t / (double)groups);
  }
}

// ------------------------------------------------------------------------------------------------
// Backward, one level
// ------------------------------------------------------------------------------------------------
struct SkBwd {
  const float* Ij; const float* Ij1;     // I_j (j = 0: p) and I_{j+1}
  const float* Sprev;                    // S_{j-1}; null at j = 0
  const float* gS; const float* gE;      // incoming; gE null at the first level (zero); gS null with `state` at the first level
  float* gS_out;                         // null at j = 0
  float* gI_out;                         // gI_j; dlogits with `x`
  const double* state; const float* y;   // first level of the loss: gS[u] = a_g y[u] + b_g
  const float* x; const float* Sy; const float* gout; float* gbase; float base_weight;      // last level of the loss
  int per_image, first_level, h, w, tiles_x;
};

__global__ __launch_bounds__(SK_THREADS) void soft_skel_bwd_kernel(SkBwd a) {
  __shared__ float sI[SK_BCELLS], sN[SK_BCELLS], sgd[SK_BCELLS], sq[SK_BCELLS];
  __shared__ unsigned char samax[SK_BCELLS], samin[SK_BCELLS];
  const int img = blockIdx.y, tile = blockIdx.x;
  const int tyi = tile / a.tiles_x, txi = tile - tyi * a.tiles_x;
  const int y0 = tyi * SK_BT - SK_BH, x0 = txi * SK_BT - SK_BH;       // the image position of cell (0, 0)
  const size_t ioff = (size_t)img * a.h * a.w;
  const float qnan = __builtin_nanf("");
  const bool loss_first = a.first_level && a.state != nullptr;
  double ca = 0.0, cb = 0.0, ccf = 0.0;
  if (a.state) {
    const size_t g = a.per_image ? (size_t)img : 0;
    ca = a.state[3 * g]; cb = a.state[3 * g + 1]; ccf = a.state[3 * g + 2];
  }

  for (int i = threadIdx.x; i < SK_BCELLS; i += SK_THREADS) {
    const int r = i / SK_BL, c = i - r * SK_BL, gy = y0 + r, gx = x0 + c;
    float v = qnan, n = qnan;
    if (gy >= 0 && gy < a.h && gx >= 0 && gx < a.w) {
      const size_t g = ioff + (size_t)gy * a.w + gx;
      v = a.Ij[g]; n = a.Ij1[g];
    }
    sI[i] = v; sN[i] = n;
  }
  __syncthreads();

  // gd and the argmax of D, two pixels out
  for (int i = threadIdx.x; i < SK_BCELLS; i += SK_THREADS) {
    const int r = i / SK_BL, c = i - r * SK_BL, gy = y0 + r, gx = x0 + c;
    float gd = 0.f;
    int am = SK_NONE;
    if (r >= 1 && r < SK_BL - 1 && c >= 1 && c < SK_BL - 1 && gy >= 0 && gy < a.h && gx >= 0 && gx < a.w) {
      float best = 0.f;
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        const float v = sN[i + (k / 3 - 1) * SK_BL + (k % 3 - 1)];
        if (v == v && (am == SK_NONE || v > best)) { best = v; am = k; }
      }
      const size_t g = ioff + (size_t)gy * a.w + gx;
      const float d = sI[i] - best;
      const float S = a.Sprev ? a.Sprev[g] : 0.f;
      const float gs = loss_first ? (float)(ca * (double)a.y[g] + cb) : a.gS[g];
      const bool on = fmaf(-S, d, d) > 0.f;
      gd = on ? gs * (1.f - S) : 0.f;
      if (a.gS_out && r >= SK_BH && r < SK_BH + SK_BT && c >= SK_BH && c < SK_BH + SK_BT) a.gS_out[g] = gs * (1.f - (on ? d : 0.f));
    }
    sgd[i] = gd; samax[i] = (unsigned char)am;
  }
  __syncthreads();

  // q = gE + route_D(-gd) and the argmin of E, one pixel out
  for (int i = threadIdx.x; i < SK_BCELLS; i += SK_THREADS) {
    const int r = i / SK_BL, c = i - r * SK_BL, gy = y0 + r, gx = x0 + c;
    float q = 0.f;
    int am = SK_NONE;
    if (r >= 2 && r < SK_BL - 2 && c >= 2 && c < SK_BL - 2 && gy >= 0 && gy < a.h && gx >= 0 && gx < a.w) {
      double acc = a.gE ? (double)a.gE[ioff + (size_t)gy * a.w + gx] : 0.0;
#pragma unroll
      for (int k = 0; k < 9; ++k) {                        // the pixel at window position k has this one at its position 8 - k
        const int o = i + (k / 3 - 1) * SK_BL + (k % 3 - 1);
        if (samax[o] == 8 - k) acc -= (double)sgd[o];
      }
      q = (float)acc;
      const int off[5] = {-SK_BL, -1, 0, 1, SK_BL};
      float best = 0.f;
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        const float v = sI[i + off[k]];
        if (v == v && (am == SK_NONE || v < best)) { best = v; am = k; }
      }
    }
    sq[i] = q; samin[i] = (unsigned char)am;
  }
  __syncthreads();

  // gI_j = gd + route_E(q) on the tile
  for (int i = threadIdx.x; i < SK_BT * SK_BT; i += SK_THREADS) {
    const int r = SK_BH + i / SK_BT, c = SK_BH + i % SK_BT, gy = y0 + r, gx = x0 + c;
    if (gy < a.h && gx < a.w) {
      const int u = r * SK_BL + c;
      const int off[5] = {-SK_BL, -1, 0, 1, SK_BL};
      double acc = (double)sgd[u];
#pragma unroll
      for (int k = 0; k < 5; ++k)                          // the neighbour at position k has this pixel at its position 4 - k
        if (samin[u + off[k]] == 4 - k) acc += (double)sq[u + off[k]];
      float out = (float)acc;
      const size_t g = ioff + (size_t)gy * a.w + gx;
      if (a.x) {
        float sp, sn;
        hpri_sigmoids(a.x[g], sp, sn);
        out = (a.gout ? a.gout[0] : 1.f) * ((out + (float)(ccf * (double)a.Sy[g])) * (sp * sn));
      }
      a.gI_out[g] = out;
    }
  }
  if (a.gbase && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) a.gbase[0] = (a.gout ? a.gout[0] : 1.f) * a.base_weight;
}

// ------------------------------------------------------------------------------------------------
// The hard metric's counts: counts[4n .. 4n+3] += |skel(P)|, |skel(P) & T|, |skel(T)|, |skel(T) & P| of image n (integer atomics)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SK_THREADS) void centerline_count_kernel(const unsigned char* __restrict__ skp, const unsigned char* __restrict__ skt,
                                                                      const unsigned char* __restrict__ dp, const unsigned char* __restrict__ dt,
                                                                      long long per, int* __restrict__ counts) {
  const size_t base = (size_t)blockIdx.y * per;
  int v[4] = {0, 0, 0, 0};
  for (long long i = (long long)blockIdx.x * SK_THREADS + threadIdx.x; i < per; i += (long long)gridDim.x * SK_THREADS) {
    const int sp = skp[base + i] != 0, st = skt[base + i] != 0, p = dp[base + i] != 0, t = dt[base + i] != 0;
    v[0] += sp; v[1] += sp & t; v[2] += st; v[3] += st & p;
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    v[r] = hpri_wave_sum(v[r]);
    if ((threadIdx.x & 63) == 0 && v[r]) atomicAdd(counts + 4 * (size_t)blockIdx.y + r, v[r]);
  }
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
static inline int sk_tiles(int n, int t) { return (int)hpri_cdiv64(n, t); }        // (n + t - 1 may not fit an int)

static int sk_check(int N, int h, int w, int iters) {
  HPRI_REQUIRE(N > 0 && h > 0 && w > 0, "soft_skeleton: bad sizes");
  // (the kernels index tiles and halos with ints: a side of 2^30 leaves room for tile + halo)
  HPRI_REQUIRE(2 * (long long)N <= 65535 && h <= (1 << 30) && w <= (1 << 30) && (long long)N * h * w < (1ll << 31),
               "soft_skeleton: N beyond 32767, a side beyond 2^30 or N*h*w beyond 2^31");
  HPRI_REQUIRE(iters >= 0 && iters <= SK_MAX_ITERS, "soft_skeleton: iters must lie in [0, 32]");
  return HPRI_OK;
}

extern "C" int hpri_soft_skeleton_tile(void) { return SK_T; }
extern "C" int hpri_soft_skeleton_max_iters(void) { return SK_MAX_ITERS; }

extern "C" size_t hpri_soft_skeleton_lds_bytes(int iters) {
  if (iters < 0 || iters > SK_MAX_ITERS) return 0;
  const size_t L = SK_T + 2 * (size_t)(iters + 2);
  return 2 * L * L * sizeof(float);
}

extern "C" size_t hpri_soft_skeleton_saved_floats(int N, int h, int w, int iters) {
  if (N <= 0 || h <= 0 || w <= 0 || iters < 0 || iters > SK_MAX_ITERS) return 0;
  return (size_t)(2 * iters + 1) * (size_t)N * (size_t)h * (size_t)w;
}

extern "C" size_t hpri_soft_skeleton_workspace_floats(int N, int h, int w) {
  if (N <= 0 || h <= 0 || w <= 0) return 0;
  return 4 * (size_t)N * (size_t)h * (size_t)w;
}

extern "C" size_t hpri_cldice_workspace_doubles(int N, int h, int w) {
  if (N <= 0 || h <= 0 || w <= 0) return 0;
  return 4 * (size_t)N * (size_t)hpri_cdiv64(h, SK_T) * (size_t)hpri_cdiv64(w, SK_T);
}

extern "C" size_t hpri_cldice_state_doubles(int N, int per_image) {
  if (N <= 0) return 0;
  return 3 * (size_t)(per_image ? N : 1);
}

static int sk_launch_fwd(SkFwd& a, hipStream_t stream) {
  a.tiles_x = sk_tiles(a.w, SK_T);
  const size_t lds = hpri_soft_skeleton_lds_bytes(a.iters);
  hpri_ask_dynamic_lds(soft_skel_fwd_kernel, lds);
  hipLaunchKernelGGL(soft_skel_fwd_kernel, dim3(a.tiles_x * sk_tiles(a.h, SK_T), a.n0 + a.n1), dim3(SK_THREADS), lds, stream, a);
  HPRI_CHECK_LAUNCH();
  return HPRI_OK;
}

// the level launches j = iters .. 0; `loss`: the arguments of the loss's first and last level (state == null: the plain operator)
static int sk_launch_bwd(const float* p, const float* saved, const float* gS, int N, int h, int w, int iters, float* out, float* ws,
                         SkBwd loss, hipStream_t stream) {
  const size_t np = (size_t)N * h * w;
  float* wgS[2] = {ws, ws + np};
  float* wgE[2] = {ws + 2 * np, ws + 3 * np};
  const dim3 grid(sk_tiles(w, SK_BT) * sk_tiles(h, SK_BT), N);
  for (int j = iters; j >= 0; --j) {
    const int par = (iters - j) & 1;
    SkBwd a = {};
    a.Ij = j == 0 ? p : saved + (size_t)(j - 1) * np;
    a.Ij1 = saved + (size_t)j * np;
    a.Sprev = j > 0 ? saved + (size_t)(iters + j) * np : nullptr;
    a.gS = j == iters ? gS : wgS[par ^ 1];
    a.gE = j == iters ? nullptr : wgE[par ^ 1];
    a.gS_out = j > 0 ? wgS[par] : nullptr;
    a.gI_out = j > 0 ? wgE[par] : out;
    a.first_level = j == iters;
    a.per_image = loss.per_image; a.state = loss.state;
    if (j == iters) a.y = loss.y;
    if (j == 0) { a.x = loss.x; a.Sy = loss.Sy; a.gout = loss.gout; a.gbase = loss.gbase; a.base_weight = loss.base_weight; }
    a.h = h; a.w = w; a.tiles_x = sk_tiles(w, SK_BT);
    hipLaunchKernelGGL(soft_skel_bwd_kernel, grid, dim3(SK_THREADS), 0, stream, a);
    HPRI_CHECK_LAUNCH();
  }
  return HPRI_OK;
}

extern "C" int hpri_soft_skeleton_fwd(const float* p, int N, int h, int w, int iters, float* S, float* saved, size_t saved_floats,
                                      hipStream_t stream) {
  HPRI_REQUIRE(p && S, "soft_skeleton_fwd: null pointer");
  if (int rc = sk_check(N, h, w, iters)) return rc;
  if (saved && saved_floats < hpri_soft_skeleton_saved_floats(N, h, w, iters))
    return hpri_set_error(HPRI_ERR_ARG, "soft_skeleton_fwd: buffer of saved planes too small");
  SkFwd a = {};
  a.src0 = p; a.n0 = N; a.S0 = S; a.saved = saved; a.h = h; a.w = w; a.iters = iters;
  return sk_launch_fwd(a, stream);
}

extern "C" int hpri_soft_skeleton_bwd(const float* p, const float* saved, size_t saved_floats, const float* grad_S, int N, int h, int w,
                                      int iters, float* grad_p, float* workspace, size_t ws_floats, hipStream_t stream) {
  HPRI_REQUIRE(p && saved && grad_S && grad_p && workspace, "soft_skeleton_bwd: null pointer");
  if (int rc = sk_check(N, h, w, iters)) return rc;
  if (saved_floats < hpri_soft_skeleton_saved_floats(N, h, w, iters))
    return hpri_set_error(HPRI_ERR_ARG, "soft_skeleton_bwd: buffer of saved planes too small");
  if (ws_floats < hpri_soft_skeleton_workspace_floats(N, h, w)) return hpri_set_error(HPRI_ERR_ARG, "soft_skeleton_bwd: workspace too small");
  SkBwd none = {};
  return sk_launch_bwd(p, saved, grad_S, N, h, w, iters, grad_p, workspace, none, stream);
}

extern "C" int hpri_cldice_fwd(const float* logits, const float* target, int N, int h, int w, int iters, float smooth, int per_image,
                               float weight, const float* base_loss, float base_weight, float* p, float* Sp, float* Sy, float* saved,
                               size_t saved_floats, float* loss, float* terms, double* state, size_t state_doubles, double* workspace,
                               size_t ws_doubles, hipStream_t stream) {
  HPRI_REQUIRE(logits && target && p && Sy && saved && loss && terms && state && workspace, "cldice_fwd: null pointer");
  if (int rc = sk_check(N, h, w, iters)) return rc;
  HPRI_REQUIRE(smooth >= 0.f, "cldice_fwd: smooth must not be negative");
  HPRI_REQUIRE(weight == weight && base_weight == base_weight, "cldice_fwd: a weight is NaN");
  if (saved_floats < hpri_soft_skeleton_saved_floats(N, h, w, iters)) return hpri_set_error(HPRI_ERR_ARG, "cldice_fwd: buffer of saved planes too small");
  if (ws_doubles < hpri_cldice_workspace_doubles(N, h, w)) return hpri_set_error(HPRI_ERR_ARG, "cldice_fwd: workspace too small");
  if (state_doubles < hpri_cldice_state_doubles(N, per_image)) return hpri_set_error(HPRI_ERR_ARG, "cldice_fwd: state buffer too small");
  SkFwd a = {};
  a.src0 = logits; a.n0 = N; a.sig0 = 1; a.p_out = p; a.S0 = Sp; a.saved = saved; a.other0 = target;
  a.src1 = target; a.n1 = N; a.S1 = Sy; a.other1 = logits; a.partial = workspace;
  a.h = h; a.w = w; a.iters = iters;
  if (int rc = sk_launch_fwd(a, stream)) return rc;
  hipLaunchKernelGGL(cldice_finalize_kernel, dim3(1), dim3(SK_THREADS), 0, stream, workspace, N, sk_tiles(h, SK_T) * sk_tiles(w, SK_T),
                     per_image ? N : 1, per_image ? 1 : 0, (double)smooth, (double)weight, base_loss, (double)base_weight, loss, state, terms);
  HPRI_CHECK_LAUNCH();
  return HPRI_OK;
}

extern "C" int hpri_cldice_bwd(const float* logits, const float* target, const float* p, const float* Sy, const float* saved,
                               size_t saved_floats, int N, int h, int w, int iters, int per_image, const double* state,
                               size_t state_doubles, const float* grad_out, float base_weight, float* grad_base, float* dlogits,
                               float* workspace, size_t ws_floats, hipStream_t stream) {
  HPRI_REQUIRE(logits && target && p && Sy && saved && state && dlogits && workspace, "cldice_bwd: null pointer");
  if (int rc = sk_check(N, h, w, iters)) return rc;
  if (saved_floats < hpri_soft_skeleton_saved_floats(N, h, w, iters)) return hpri_set_error(HPRI_ERR_ARG, "cldice_bwd: buffer of saved planes too small");
  if (ws_floats < hpri_soft_skeleton_workspace_floats(N, h, w)) return hpri_set_error(HPRI_ERR_ARG, "cldice_bwd: workspace too small");
  if (state_doubles < hpri_cldice_state_doubles(N, per_image)) return hpri_set_error(HPRI_ERR_ARG, "cldice_bwd: state buffer too small");
  SkBwd l = {};
  l.state = state; l.y = target; l.x = logits; l.Sy = Sy; l.gout = grad_out; l.gbase = grad_base; l.base_weight = base_weight;
  l.per_image = per_image ? 1 : 0;
  return sk_launch_bwd(p, saved, nullptr, N, h, w, iters, dlogits, workspace, l, stream);
}

extern "C" int hpri_centerline_counts(const unsigned char* skel_pred, const unsigned char* skel_truth, const unsigned char* pred,
                                      const unsigned char* truth, int N, long long per_image, int* counts, hipStream_t stream) {
  HPRI_REQUIRE(skel_pred && skel_truth && pred && truth && counts, "centerline_counts: null pointer");
  HPRI_REQUIRE(N > 0 && N <= 65535 && per_image > 0 && per_image < (1ll << 31), "centerline_counts: bad sizes");
  const long long blocks = (per_image + SK_THREADS - 1) / SK_THREADS;
  hipLaunchKernelGGL(centerline_count_kernel, dim3((unsigned)(blocks < 256 ? blocks : 256), N), dim3(SK_THREADS), 0, stream, skel_pred,
                     skel_truth, pred, truth, per_image, counts);
  HPRI_CHECK_LAUNCH();
  return HPRI_OK;
}
