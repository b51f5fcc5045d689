// Distances on the device (hyperpri_amd/distance.py): the exact squared Euclidean distance transform of a binary decision map, a
// histogram of such a map over a selection of pixels, Zhang-Suen thinning and the link counts of a skeleton.
//
// Everything is integer arithmetic on a contiguous (N, h, w) map, N*h*w < 2^31, indexed linearly; images never influence each other;
// the only atomics are integer adds and maxima on vector memory whose result does not depend on the order of arrival: every output
// is bit-reproducible.  The decision of a pixel is the one components.hip takes (decision.h).  No workgroup waits for another; every
// grid is capped with a grid-stride loop.
//
// Distance transform:  d2[n,y,x] = min(FAR, min over the sites q of image n of (y-qy)^2 + (x-qx)^2),  FAR = h*h + w*w < 2^31, which
// no pair of pixels attains: an image without a site is FAR everywhere.  sites: 0 = the background pixels, 1 = the foreground
// pixels, 2 = the boundary: foreground pixels with an edge neighbour in the background or outside the image.  Two separable passes:
//   1. dt_column_kernel  one thread per column (neighbouring threads on neighbouring x: every row access is coalesced) sweeps down
//                        and then up and leaves g[y][x] = |y - y'| to the nearest site of that column, DT_NONE without one.  The site
//                        predicate is evaluated here, from the caller's map (the boundary form keeps the pixel above and below in
//                        registers and reads left and right); no site map exists.
//   2. dt_row_kernel     one workgroup per row, in place: the row of g^2 is staged in LDS (DT_MAX_W words), every thread owns the
//                        pixels x = tid, tid + 256, ...: best = g[x]^2, then k = 1, 2, ...: best = min(best, g[x -+ k]^2 + k^2) until
//                        k^2 >= best -- exact, since a column k away contributes at least k^2, and proportional to the answer.
//                        Sums stay below 2^32 (both terms are below 2^31) and are taken unsigned.
//
// Selection histogram: the pixels of image n that the selector picks (sel_kind 0: a uint8 map, value != 0; 1: an int32 map, value
// == 0 -- the site pixels of a distance transform) and whose value is >= 0.  dt_select_stats_kernel adds their number to stats[0] and
// raises stats[1] to their maximum; dt_select_hist_kernel adds 1 to hist[value] for every such pixel with value < bins, through an
// LDS copy of the histogram per 16384 pixels where bins <= DT_HIST_LDS_BINS, straight into global memory otherwise.
//
// Thinning (Zhang-Suen): P2..P9 are the neighbours clockwise from north (N, NE, E, SE, S, SW, W, NW), outside the image background;
// B = their sum, A = the 0 -> 1 steps around the ring P2, P3, ..., P9, P2.  Sub-iteration 1 deletes a foreground pixel when
// 2 <= B <= 6, A == 1, P2*P4*P6 == 0 and P4*P6*P8 == 0; sub-iteration 2 when the same holds with P2*P4*P8 == 0 and P2*P6*P8 == 0.
// A launch is one sub-iteration over the batch, out of place; deletions of pair j are added to deleted[j*N + n].
//
// Links of a skeleton, per image: S pixels; E4 pairs of horizontally or vertically adjacent pixels; Ed pairs of diagonally adjacent
// pixels whose two common edge neighbours are both off the skeleton (so a corner is not counted twice).
#include "decision.h"
#include "tail_helpers.h"

#define DT_THREADS 256
#define DT_MAX_W 8192                    // the row of g^2 in LDS: 32 KB
#define DT_NONE 0x7fffffff
#define DT_HIST_LDS_BINS 4096
#define DT_HIST_CHUNK (DT_THREADS * 64)  // pixels per LDS copy of the histogram

__global__ __launch_bounds__(DT_THREADS) void dt_column_kernel(const CcDecision d, int sites, int N, int h, int w, int* __restrict__ g) {
  const int strips = (w + DT_THREADS - 1) / DT_THREADS;
  const long long items = (long long)N * strips;
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    const int n = (int)(it / strips), x = (int)(it % strips) * DT_THREADS + (int)threadIdx.x;
    if (x >= w) continue;
    const int base = n * h * w + x;
    int run = DT_NONE, up = 0, cur = cc_decide(d, base);
    for (int y = 0; y < h; ++y) {
      const int i = base + y * w;
      const int down = y + 1 < h ? cc_decide(d, i + w) : 0;
      int site;
      if (sites == 0) site = !cur;
      else if (sites == 1) site = cur;
      else site = cur && !(up && down && x > 0 && cc_decide(d, i - 1) && x + 1 < w && cc_decide(d, i + 1));
      run = site ? 0 : run == DT_NONE ? DT_NONE : run + 1;
      g[i] = run;
      up = cur;
      cur = down;
    }
    run = DT_NONE;
    for (int y = h - 1; y >= 0; --y) {
      const int i = base + y * w, v = g[i];                            // (this thread's own stores)
      run = v == 0 ? 0 : run == DT_NONE ? DT_NONE : run + 1;
      if (run < v) g[i] = run;
    }
  }
}

__global__ __launch_bounds__(DT_THREADS) void dt_row_kernel(int rows, int w, unsigned far, int* __restrict__ d2) {
  __shared__ unsigned f[DT_MAX_W];
  for (long long r = blockIdx.x; r < rows; r += gridDim.x) {           // (uniform per workgroup: the barriers below are safe)
    int* row = d2 + r * w;
    for (int x = threadIdx.x; x < w; x += DT_THREADS) {
      const int v = row[x];
      f[x] = v == DT_NONE ? far : (unsigned)v * (unsigned)v;
    }
    __syncthreads();
    for (int x = threadIdx.x; x < w; x += DT_THREADS) {
      unsigned best = f[x];
      const int reach = max(x, w - 1 - x);
      for (int k = 1; k <= reach; ++k) {
        const unsigned kk = (unsigned)k * (unsigned)k;
        if (kk >= best) break;                                         // no farther column can win
        if (x - k >= 0) best = min(best, f[x - k] + kk);
        if (x + k < w) best = min(best, f[x + k] + kk);
      }
      row[x] = (int)best;                                              // (<= far < 2^31)
    }
    __syncthreads();                                                   // the next row reuses the LDS
  }
}

// ---- a histogram of an int32 map over a selection ------------------------------------------------------------------------------
__device__ __forceinline__ int dt_selected(const void* sel, int kind, int i) {
  return kind == 0 ? reinterpret_cast<const unsigned char*>(sel)[i] != 0 : reinterpret_cast<const int*>(sel)[i] == 0;
}

__device__ __forceinline__ long long dt_wave_items(int N, int per) { return (long long)N * ((per + 63) / 64); }

__global__ __launch_bounds__(DT_THREADS) void dt_select_stats_kernel(const int* __restrict__ values, const void* __restrict__ sel,
                                                                     int sel_kind, int N, int per, int* stats, int stride) {
  const int lane = threadIdx.x & 63, waves = DT_THREADS / 64, chunks = (per + 63) / 64;
  const long long items = dt_wave_items(N, per);
  for (long long it = (long long)blockIdx.x * waves + (threadIdx.x >> 6); it < items; it += (long long)gridDim.x * waves) {
    const int n = (int)(it / chunks), p = (int)(it % chunks) * 64 + lane;
    int v = -1;
    if (p < per && dt_selected(sel, sel_kind, n * per + p)) v = values[n * per + p];
    const int cnt = __popcll(__ballot(v >= 0));
    if (cnt == 0) continue;                                            // (uniform per wave)
    v = hpri_wave_max(v);
    if (lane == 0) {
      atomicAdd(&stats[(long long)n * stride], cnt);
      atomicMax(&stats[(long long)n * stride + 1], v);
    }
  }
}

__global__ __launch_bounds__(DT_THREADS) void dt_select_hist_kernel(const int* __restrict__ values, const void* __restrict__ sel,
                                                                    int sel_kind, int N, int per, int bins, int* hist, long long hist_stride) {
  __shared__ int lh[DT_HIST_LDS_BINS];
  const bool local = bins <= DT_HIST_LDS_BINS;
  const int chunks = (per + DT_HIST_CHUNK - 1) / DT_HIST_CHUNK;
  const long long items = (long long)N * chunks;
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {       // (uniform per workgroup: the barriers below are safe)
    const int n = (int)(it / chunks), lo = (int)(it % chunks) * DT_HIST_CHUNK, hi = min(per, lo + DT_HIST_CHUNK);
    int* gh = hist + n * hist_stride;
    if (local) {
      for (int b = threadIdx.x; b < bins; b += DT_THREADS) lh[b] = 0;
      __syncthreads();
    }
    for (int p = lo + threadIdx.x; p < hi; p += DT_THREADS) {
      const int i = n * per + p;
      if (!dt_selected(sel, sel_kind, i)) continue;
      const int v = values[i];
      if (v < 0 || v >= bins) continue;                                // (a value beyond the histogram is not counted, never written)
      if (local) atomicAdd(&lh[v], 1);
      else atomicAdd(&gh[v], 1);
    }
    if (local) {
      __syncthreads();
      for (int b = threadIdx.x; b < bins; b += DT_THREADS) {
        const int c = lh[b];
        if (c) atomicAdd(&gh[b], c);
      }
      __syncthreads();                                                 // the next chunk reuses the LDS
    }
  }
}

// ---- thinning and links --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DT_THREADS) void dt_decide_kernel(const CcDecision d, int n_pix, unsigned char* __restrict__ out) {
  for (long long it = (long long)blockIdx.x * DT_THREADS + threadIdx.x; it < n_pix; it += (long long)gridDim.x * DT_THREADS)
    out[it] = (unsigned char)cc_decide(d, (int)it);
}

// pixel (y, x) of one image, background outside it
__device__ __forceinline__ int dt_px(const unsigned char* m, int y, int x, int h, int w) {
  return (y >= 0 && y < h && x >= 0 && x < w) ? m[y * w + x] != 0 : 0;
}

__global__ __launch_bounds__(DT_THREADS) void dt_thin_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                                             int N, int h, int w, int sub, int* deleted) {
  const int lane = threadIdx.x & 63, waves = DT_THREADS / 64, per = h * w, chunks = (per + 63) / 64;
  const long long items = dt_wave_items(N, per);
  for (long long it = (long long)blockIdx.x * waves + (threadIdx.x >> 6); it < items; it += (long long)gridDim.x * waves) {
    const int n = (int)(it / chunks), p = (int)(it % chunks) * 64 + lane;
    int del = 0;
    if (p < per) {
      const unsigned char* m = src + (long long)n * per;
      const int y = p / w, x = p % w, c = m[p] != 0;
      if (c) {
        const int p2 = dt_px(m, y - 1, x, h, w), p3 = dt_px(m, y - 1, x + 1, h, w), p4 = dt_px(m, y, x + 1, h, w),
                  p5 = dt_px(m, y + 1, x + 1, h, w), p6 = dt_px(m, y + 1, x, h, w), p7 = dt_px(m, y + 1, x - 1, h, w),
                  p8 = dt_px(m, y, x - 1, h, w), p9 = dt_px(m, y - 1, x - 1, h, w);
        const int B = p2 + p3 + p4 + p5 + p6 + p7 + p8 + p9;
        const int A = (!p2 && p3) + (!p3 && p4) + (!p4 && p5) + (!p5 && p6) + (!p6 && p7) + (!p7 && p8) + (!p8 && p9) + (!p9 && p2);
        const int open = sub == 0 ? (p2 * p4 * p6 == 0 && p4 * p6 * p8 == 0) : (p2 * p4 * p8 == 0 && p2 * p6 * p8 == 0);
        del = B >= 2 && B <= 6 && A == 1 && open;
      }
      dst[(long long)n * per + p] = (unsigned char)(c && !del);
    }
    const int cnt = __popcll(__ballot(del != 0));
    if (cnt && lane == 0) atomicAdd(&deleted[n], cnt);
  }
}

__global__ __launch_bounds__(DT_THREADS) void dt_links_kernel(const unsigned char* __restrict__ skel, int N, int h, int w, int* links) {
  const int lane = threadIdx.x & 63, waves = DT_THREADS / 64, per = h * w, chunks = (per + 63) / 64;
  const long long items = dt_wave_items(N, per);
  for (long long it = (long long)blockIdx.x * waves + (threadIdx.x >> 6); it < items; it += (long long)gridDim.x * waves) {
    const int n = (int)(it / chunks), p = (int)(it % chunks) * 64 + lane;
    int s = 0, e4 = 0, ed = 0;
    if (p < per) {
      const unsigned char* m = skel + (long long)n * per;
      if (m[p] != 0) {                                                 // every pair is met once, at its earlier pixel in raster order
        const int y = p / w, x = p % w;
        const int right = dt_px(m, y, x + 1, h, w), down = dt_px(m, y + 1, x, h, w), left = dt_px(m, y, x - 1, h, w);
        s = 1;
        e4 = right + down;
        ed = (dt_px(m, y + 1, x + 1, h, w) && !right && !down) + (dt_px(m, y + 1, x - 1, h, w) && !left && !down);
      }
    }
    if (__ballot(s != 0) == 0) continue;                               // (uniform per wave)
    s = hpri_wave_sum(s); e4 = hpri_wave_sum(e4); ed = hpri_wave_sum(ed);
    if (lane == 0) {
      atomicAdd(&links[3 * n], s);
      if (e4) atomicAdd(&links[3 * n + 1], e4);
      if (ed) atomicAdd(&links[3 * n + 2], ed);
    }
  }
}

// ---- launchers ------------------------------------------------------------------------------------------------------------------
static inline int dt_grid(long long items, int per_block) { return hpri_grid_per_cu(items, per_block, 8); }      // eight workgroups per CU

extern "C" int hpri_edt_max_width() { return DT_MAX_W; }
extern "C" int hpri_edt_col_threads() { return DT_THREADS; }
extern "C" int hpri_edt_row_threads() { return DT_THREADS; }
extern "C" int hpri_select_hist_lds_bins() { return DT_HIST_LDS_BINS; }

// FAR = h*h + w*w, or -1 where the transform does not exist: a size <= 0, a row beyond hpri_edt_max_width, FAR >= 2^31 (pure host).
extern "C" int hpri_edt_far(int h, int w) {
  if (h <= 0 || w <= 0 || w > DT_MAX_W) return -1;
  const long long far = (long long)h * h + (long long)w * w;
  return far < 2147483648LL ? (int)far : -1;
}

#define DT_REQUIRE_MAP(who)                                                                                         \
  HPRI_REQUIRE(N > 0 && h > 0 && w > 0, who ": bad sizes");                                                         \
  HPRI_REQUIRE((long long)N * h * w < 2147483648LL, who ": N*h*w must be below 2^31")

#define DT_REQUIRE_KIND(who) HPRI_REQUIRE(pred_kind >= 0 && pred_kind <= 2, who ": pred_kind must be 0 (fp32), 1 (uint8) or 2 (fp32 mask)")

extern "C" int hpri_edt(const void* pred, int pred_kind, float threshold, int is_logits, int sites, int N, int h, int w, int* d2,
                        hipStream_t stream) {
  HPRI_REQUIRE(pred && d2, "edt: null pointer");
  DT_REQUIRE_KIND("edt");
  HPRI_REQUIRE(sites >= 0 && sites <= 2, "edt: sites must be 0 (background), 1 (foreground) or 2 (boundary)");
  DT_REQUIRE_MAP("edt");
  HPRI_REQUIRE(w <= DT_MAX_W, "edt: a row does not fit the row pass (hpri_edt_max_width)");
  const int far = hpri_edt_far(h, w);
  HPRI_REQUIRE(far > 0, "edt: h*h + w*w must be below 2^31");
  CcDecision d; d.pred = pred; d.kind = pred_kind; d.threshold = threshold; d.is_logits = is_logits; d.invert = 0;
  hipLaunchKernelGGL(dt_column_kernel, dim3(dt_grid((long long)N * hpri_cdiv(w, DT_THREADS), 1)), dim3(DT_THREADS), 0, stream, d, sites,
                     N, h, w, d2);
  HPRI_CHECK_LAUNCH();
  hipLaunchKernelGGL(dt_row_kernel, dim3(dt_grid((long long)N * h, 1)), dim3(DT_THREADS), 0, stream, N * h, w, (unsigned)far, d2);
  HPRI_CHECK_LAUNCH();
  return HPRI_OK;
}

#define DT_REQUIRE_SELECT(who)                                                                                      \
  HPRI_REQUIRE(N > 0 && per_image > 0 && (long long)N * per_image < 2147483648LL, who ": bad sizes");               \
  HPRI_REQUIRE(sel_kind == 0 || sel_kind == 1, who ": sel_kind must be 0 (uint8, != 0) or 1 (int32, == 0)")

extern "C" int hpri_select_stats(const int* values, const void* selector, int sel_kind, int N, int per_image, int* stats,
                                 int stats_stride, hipStream_t stream) {
  HPRI_REQUIRE(values && selector && stats, "select_stats: null pointer");
  DT_REQUIRE_SELECT("select_stats");
  HPRI_REQUIRE(stats_stride >= 2, "select_stats: stats_stride must be at least 2");
  hipLaunchKernelGGL(dt_select_stats_kernel, dim3(dt_grid((long long)N * hpri_cdiv(per_image, 64), DT_THREADS / 64)), dim3(DT_THREADS), 0,
                     stream, values, selector, sel_kind, N, per_image, stats, stats_stride);
  HPRI_CHECK_LAUNCH();
  return HPRI_OK;
}

extern "C" int hpri_select_hist(const int* values, const void* selector, int sel_kind, int N, int per_image, int bins, int* hist,
                                long long hist_stride, hipStream_t stream) {
  HPRI_REQUIRE(values && selector && hist, "select_hist: null pointer");
  DT_REQUIRE_SELECT("select_hist");
  HPRI_REQUIRE(bins > 0 && hist_stride >= bins, "select_hist: need bins > 0 and hist_stride >= bins");
  hipLaunchKernelGGL(dt_select_hist_kernel, dim3(dt_grid((long long)N * hpri_cdiv(per_image, DT_HIST_CHUNK), 1)), dim3(DT_THREADS), 0,
                     stream, values, selector, sel_kind, N, per_image, bins, hist, hist_stride);
  HPRI_CHECK_LAUNCH();
  return HPRI_OK;
}

extern "C" int hpri_thin(const void* pred, int pred_kind, float threshold, int is_logits, int N, int h, int w, int decide, int pairs,
                         unsigned char* map, unsigned char* other, int* deleted, hipStream_t stream) {
  HPRI_REQUIRE(map && other && map != other, "thin: need two distinct maps");
  HPRI_REQUIRE(pairs >= 0 && (pairs == 0 || deleted), "thin: need pairs >= 0 and, for pairs > 0, the deletion counters");
  HPRI_REQUIRE(decide || pairs > 0, "thin: nothing to do");
  DT_REQUIRE_MAP("thin");
  if (decide) {
    HPRI_REQUIRE(pred, "thin: null pointer");
    DT_REQUIRE_KIND("thin");
    CcDecision d; d.pred = pred; d.kind = pred_kind; d.threshold = threshold; d.is_logits = is_logits; d.invert = 0;
    hipLaunchKernelGGL(dt_decide_kernel, dim3(dt_grid((long long)N * h * w, DT_THREADS)), dim3(DT_THREADS), 0, stream, d, N * h * w, map);
    HPRI_CHECK_LAUNCH();
  }
  const int grid = dt_grid((long long)N * hpri_cdiv(h * w, 64), DT_THREADS / 64);
  for (int j = 0; j < pairs; ++j) {
    hipLaunchKernelGGL(dt_thin_kernel, dim3(grid), dim3(DT_THREADS), 0, stream, map, other, N, h, w, 0, deleted + (long long)j * N);
    HPRI_CHECK_LAUNCH();
    hipLaunchKernelGGL(dt_thin_kernel, dim3(grid), dim3(DT_THREADS), 0, stream, other, map, N, h, w, 1, deleted + (long long)j * N);
    HPRI_CHECK_LAUNCH();
  }
  return HPRI_OK;
}

extern "C" int hpri_skeleton_links(const unsigned char* skeleton, int N, int h, int w, int* links, hipStream_t stream) {
  HPRI_REQUIRE(skeleton && links, "skeleton_links: null pointer");
  DT_REQUIRE_MAP("skeleton_links");
  hipLaunchKernelGGL(dt_links_kernel, dim3(dt_grid((long long)N * hpri_cdiv(h * w, 64), DT_THREADS / 64)), dim3(DT_THREADS), 0, stream,
                     skeleton, N, h, w, links);
  HPRI_CHECK_LAUNCH();
  return HPRI_OK;
}
