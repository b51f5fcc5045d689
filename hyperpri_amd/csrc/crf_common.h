// What crf.hip (the mean-field forward) and crf_grad.hip (its backward) share: the tile, the limits, the launch arguments of the
// iteration kernel and the per-pixel pieces whose fp32 order both sides must keep -- the softmax and the reading of the unaries.
#pragma once
#include "tail_helpers.h"

#define CRF_TILE_H 16
#define CRF_TILE_W 32
#define CRF_THREADS (CRF_TILE_H * CRF_TILE_W)
#define CRF_MAX_R 8
#define CRF_MAX_K 3
#define CRF_MAX_C 8
#define CRF_MAX_T 16
#define CRF_PER_CU 2                         // workgroups a CU is offered (what its LDS holds at r = 8); the kernels stride over the rest

struct CrfArgs {
  const float* unary;      // (N, C, H, W), or (N, H, W) with binary
  const float* guide;      // (N, H, W, gs)
  const float* qin;        // (N, C, H, W): Q^(t-1); not read by the first launch
  float* qout;             // (N, C, H, W): Q^t; not written by the last launch
  float* out;              // the last launch writes
  const float* wa_dev;     // the training entries: w_a, w_s and mu in device memory (NULL: the values below)
  const float* ws_dev;
  const float* mu_dev;
  float ta[CRF_MAX_R + 1], tg[CRF_MAX_R + 1];
  float mu[CRF_MAX_C * CRF_MAX_C];
  float b, wa, ws;
  int items;               // tiles x images (below 2^31: crf_frame_ok)
  int gs, H, W, r, tiles_x, tiles_y;
  int flags;               // CRF_VEC .. CRF_PROB: one scalar register for the six switches
};
#define CRF_VEC 1          // the guide is read 16 bytes at a time
#define CRF_BINARY 2
#define CRF_POTTS 4
#define CRF_FIRST 8
#define CRF_LAST 16
#define CRF_PROB 32

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
__device__ __forceinline__ void crf_unary(const float* __restrict__ unary, int binary, int n, long long hw, long long px, float (&U)[C]) {
  if (C == 2 && binary) {
    U[0] = 0.f;
    U[1] = unary[n * hw + px];
  } else {
#pragma unroll
    for (int l = 0; l < C; ++l) U[l] = unary[((long long)n * C + l) * hw + px];
  }
}

// ---- host --------------------------------------------------------------------------------------------------------------------------
static inline bool crf_frame_ok(int N, int C, int H, int W) {
  return N > 0 && C >= 2 && C <= CRF_MAX_C && H > 0 && W > 0 && (long long)H * W < (1LL << 31) && (long long)N * C < (1LL << 31) &&
         (long long)N * C * H * W < (1LL << 40) &&
         (long long)N * ((H + CRF_TILE_H - 1) / CRF_TILE_H) * ((W + CRF_TILE_W - 1) / CRF_TILE_W) < (1LL << 31);      // the tiles: an int
}

static inline bool crf_unit_table(const float* t, int r) {      // exp(-d^2 / (2 theta^2)): 1 at d = 0, in [0, 1] and not increasing
  if (t[0] != 1.f) return false;
  for (int d = 1; d <= r; ++d)
    if (!(t[d] >= 0.f && t[d] <= t[d - 1])) return false;
  return true;
}

static inline size_t crf_plane_lds(int radius, int K, int C) {
  return (size_t)(CRF_TILE_W + 2 * radius) * (CRF_TILE_H + 2 * radius) * (K + C) * sizeof(float);
}

// The training workspace, one region for the forward and the backward of a call (hpri_crf_train_workspace_bytes):
//   [ fp64 partial sums: T x tiles x (2 + C^2) ][ the stack: T plane sets, slot t-1 = Q^t ][ two plane sets of gL ]
extern "C" size_t hpri_crf_train_workspace_bytes(int N, int C, int H, int W, int T);      // crf.hip
static inline size_t crf_train_partials(int N, int C, int H, int W, int T) {
  return (size_t)T * hpri_cdiv(W, CRF_TILE_W) * hpri_cdiv(H, CRF_TILE_H) * N * (2 + C * C);
}
