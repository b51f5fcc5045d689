// Connected components on the device (hyperpri_amd/components.py): label a binary decision map, measure its components, clean it.
//
// The decision of a pixel is the one seg_counts_kernel / segmap_class take -- p = is_logits ? 1 / (1 + expf(-x)) : x; fg = p > thr --
// or `value != 0` of a uint8 map; `invert` swaps the classes.  A contiguous (N, h, w) map, N*h*w < 2^31, is indexed linearly; images
// never connect.  Labelling is union-find with the invariant parent[i] <= i: an inactive pixel holds -1, the root of a component is
// its smallest linear index.  Two modes share every kernel:
//   * label: only the foreground is active, connectivity 4 or 8;
//   * both (cleaning): the foreground is active with the caller's connectivity and the background with the DUAL one (4 for
//     foreground 8, 8 for foreground 4); a pixel unites only with neighbours of its own class, so one parent array holds both
//     forests.
// The phases are separate launches on the caller's stream, no workgroup ever waits for another (no flags, no spin loops, no
// cooperative launch), every grid is capped with a grid-stride loop:
//   1. cc_tile_kernel     one workgroup labels one CC_TILE_H x CC_TILE_W tile in LDS with a local union-find (LDS atomics and
//                         workgroup barriers only), writes the decision map `dec` and parent[i] = the GLOBAL index of i's tile root
//                         (local and global raster order agree inside a tile, so the tile's smallest local index is its smallest
//                         global one).
//   2. cc_border_kernel   unites equal-class neighbours across tile edges in global memory.  Several workgroups read and write the
//                         same words here, so EVERY access to parent is an agent-scope atomic (relaxed load, atomicMin): per-XCD
//                         L2s are not coherent and a CU's L1 is never refreshed by another CU's stores.
//   3. cc_flatten_kernel  out of place: root[i] = find(i), plain loads (parent was written by earlier launches), and per row of
//                         the map the number of roots.
// Termination: find follows parent, and parent[i] <= i with equality only at a root, so the index strictly decreases; union
// retries atomicMin(&parent[a], b) with b < a on the value the atomic returned, which is smaller than a when it is not a: a value
// strictly decreases in every round.  Integer atomics only, and the result -- the minimum index of the component -- does not depend
// on the order of arrival: the output is bit-reproducible.
//
// Numbering (label mode): labels are 1..counts[n] per image in raster order of each component's first pixel, which is the rank of
// its root among the image's roots (the numbering of scipy.ndimage.label); background 0.  cc_flatten_kernel counts roots per row,
// cc_rowscan_kernel turns the rows of one image into exclusive offsets and the image's count, cc_rank_kernel writes the rank at
// every root (ballot prefix inside a wave, one wave per row), cc_relabel_kernel copies labels[root[i]] to the other pixels (it reads
// only root positions and writes only the others).
//
// Measuring: one pass over labels; a wave owns 64 consecutive pixels of a row, equal neighbouring labels form a run and the run's
// first lane issues the integer atomics (area, box, overlap with `((int)truth) != 0`) for the whole run.
//
// Cleaning (both mode): area and "touches the image edge" accumulate at the root index of each component (the same runs), then one
// pass decides: a foreground component with area < min_area becomes background; a background component that touches no image edge
// (its bounding box does not reach row 0, row h-1, column 0 or column w-1 -- equivalently none of its pixels lies there) and has
// area <= max_hole becomes foreground.  Holes are found in the INPUT decision, not after speck removal: the two edits act on
// disjoint pixels (one on foreground, one on background pixels of the input), so their order is immaterial.
#include "decision.h"                    // CcDecision, cc_decide (shared with distance.hip)
#include "tail_helpers.h"

#define CC_THREADS 256
#define CC_TILE_H 32
#define CC_TILE_W 64
#define CC_TILE (CC_TILE_H * CC_TILE_W)
#define CC_PER_THREAD (CC_TILE / CC_THREADS)
#define CC_OUTSIDE 2                     // class of a tile cell outside the image

// ---- the local union-find of one tile (LDS) ------------------------------------------------------------------------------------
__device__ __forceinline__ int cc_lds_find(int* lp, int i) {
  int p = __hip_atomic_load(&lp[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  while (p != i) {                                                     // p < i: the index strictly decreases
    i = p;
    p = __hip_atomic_load(&lp[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  return i;
}

__device__ __forceinline__ void cc_lds_union(int* lp, int a, int b) {
  for (;;) {
    a = cc_lds_find(lp, a);
    b = cc_lds_find(lp, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }                      // a > b: hang a below b
    const int old = atomicMin(&lp[a], b);
    if (old == a) return;                                              // a was still a root: united
    a = old;                                                           // old < a: retry from a strictly smaller value
  }
}

// act1 / act0: the class is active; diag1 / diag0: its diagonal neighbours connect (8-connectivity)
struct CcMode { int act0, act1, diag0, diag1; };

__device__ __forceinline__ int cc_active(const CcMode& m, int c) { return c == 1 ? m.act1 : c == 0 ? m.act0 : 0; }
__device__ __forceinline__ int cc_diag(const CcMode& m, int c) { return c == 1 ? m.diag1 : m.diag0; }

__global__ __launch_bounds__(CC_THREADS) void cc_tile_kernel(const CcDecision d, const CcMode m, int N, int h, int w,
                                                             unsigned char* __restrict__ dec, int* __restrict__ parent) {
  __shared__ int lp[CC_TILE];
  __shared__ unsigned char lc[CC_TILE];
  const int tiles_x = (w + CC_TILE_W - 1) / CC_TILE_W, tiles_y = (h + CC_TILE_H - 1) / CC_TILE_H;
  const long long tiles = (long long)N * tiles_y * tiles_x;
  for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {          // (uniform per workgroup: the barriers below are safe)
    const int tx = (int)(t % tiles_x);
    const long long tr = t / tiles_x;
    const int ty = (int)(tr % tiles_y), n = (int)(tr / tiles_y);
    const int y0 = ty * CC_TILE_H, x0 = tx * CC_TILE_W;
    const int base = (n * h + y0) * w + x0;                            // global index of the tile's first pixel
#pragma unroll
    for (int k = 0; k < CC_PER_THREAD; ++k) {
      const int l = threadIdx.x + k * CC_THREADS, ly = l / CC_TILE_W, lx = l % CC_TILE_W;
      int c = CC_OUTSIDE;
      if (y0 + ly < h && x0 + lx < w) {
        const int g = base + ly * w + lx;
        c = cc_decide(d, g);
        dec[g] = (unsigned char)c;
      }
      lc[l] = (unsigned char)c;
      lp[l] = cc_active(m, c) ? l : -1;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CC_PER_THREAD; ++k) {
      const int l = threadIdx.x + k * CC_THREADS, ly = l / CC_TILE_W, lx = l % CC_TILE_W;
      const int c = lc[l];
      if (!cc_active(m, c)) continue;
      if (lx > 0 && lc[l - 1] == c) cc_lds_union(lp, l, l - 1);
      if (ly > 0) {
        if (lc[l - CC_TILE_W] == c) cc_lds_union(lp, l, l - CC_TILE_W);
        if (cc_diag(m, c)) {
          if (lx > 0 && lc[l - CC_TILE_W - 1] == c) cc_lds_union(lp, l, l - CC_TILE_W - 1);
          if (lx < CC_TILE_W - 1 && lc[l - CC_TILE_W + 1] == c) cc_lds_union(lp, l, l - CC_TILE_W + 1);
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CC_PER_THREAD; ++k) {
      const int l = threadIdx.x + k * CC_THREADS, ly = l / CC_TILE_W, lx = l % CC_TILE_W;
      if (y0 + ly < h && x0 + lx < w) {
        int r = -1;
        if (cc_active(m, lc[l])) {
          const int lr = cc_lds_find(lp, l);
          r = base + (lr / CC_TILE_W) * w + (lr % CC_TILE_W);
        }
        parent[base + ly * w + lx] = r;
      }
    }
    __syncthreads();                                                   // the next tile reuses the LDS
  }
}

// ---- the global union-find across tile edges: agent-scope atomics on every access ----------------------------------------------
__device__ __forceinline__ int cc_g_load(int* parent, int i) {
  return __hip_atomic_load(&parent[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int cc_g_find(int* parent, int i) {
  int p = cc_g_load(parent, i);
  while (p != i) {                                                     // p < i: the index strictly decreases
    i = p;
    p = cc_g_load(parent, i);
  }
  return i;
}

__device__ __forceinline__ void cc_g_union(int* parent, int a, int b) {
  for (;;) {
    a = cc_g_find(parent, a);
    b = cc_g_find(parent, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&parent[a], b);                          // (device scope)
    if (old == a) return;
    a = old;                                                           // old < a: a value strictly decreases
  }
}

// Every adjacent pair of pixels in different tiles is met once, at its later pixel in raster order, whose "backward" neighbours are
// left, up-left, up and up-right: left crosses an edge only from a tile's first column, up from its first row, up-left from either,
// up-right from the first row or the last column.
__global__ __launch_bounds__(CC_THREADS) void cc_border_kernel(const CcMode m, int N, int h, int w,
                                                               const unsigned char* __restrict__ dec, int* parent) {
  const int n_pix = N * h * w;
  for (long long it = (long long)blockIdx.x * CC_THREADS + threadIdx.x; it < n_pix; it += (long long)gridDim.x * CC_THREADS) {
    const int i = (int)it, x = i % w, y = (i / w) % h;
    const int bx = x % CC_TILE_W, by = y % CC_TILE_H;
    const bool first_col = bx == 0, last_col = bx == CC_TILE_W - 1, first_row = by == 0;
    if (!first_col && !last_col && !first_row) continue;
    const int c = dec[i];
    if (!cc_active(m, c)) continue;
    if (first_col && x > 0 && dec[i - 1] == c) cc_g_union(parent, i, i - 1);
    if (y > 0) {                                                       // (row 0 of an image has no upper neighbour: images never connect)
      if (first_row && dec[i - w] == c) cc_g_union(parent, i, i - w);
      if (cc_diag(m, c)) {
        if (x > 0 && (first_row || first_col) && dec[i - w - 1] == c) cc_g_union(parent, i, i - w - 1);
        if (x < w - 1 && (first_row || last_col) && dec[i - w + 1] == c) cc_g_union(parent, i, i - w + 1);
      }
    }
  }
}

// ---- flatten, out of place; one wave per row, which also counts the row's roots -------------------------------------------------
__global__ __launch_bounds__(CC_THREADS) void cc_flatten_kernel(int rows, int w, const int* __restrict__ parent,
                                                                int* __restrict__ root, int* __restrict__ rowcount) {
  const int lane = threadIdx.x & 63, waves = CC_THREADS / 64;
  for (long long r = (long long)blockIdx.x * waves + (threadIdx.x >> 6); r < rows; r += (long long)gridDim.x * waves) {
    const int base = (int)r * w;
    int cnt = 0;
    for (int x = lane; x < w; x += 64) {
      const int i = base + x;
      int p = parent[i];
      if (p >= 0) {
        int j = i;
        while (p != j) { j = p; p = parent[j]; }                       // p < j: the index strictly decreases
        p = j;
        cnt += p == i;
      }
      root[i] = p;
    }
    cnt = hpri_wave_sum(cnt);
    if (lane == 0 && rowcount) rowcount[r] = cnt;
  }
}

// rowbase[n*h + y] = roots of image n above row y; counts[n] = roots of image n.  One workgroup per image.
__global__ __launch_bounds__(CC_THREADS) void cc_rowscan_kernel(int N, int h, const int* __restrict__ rowcount,
                                                                int* __restrict__ rowbase, int* __restrict__ counts) {
  __shared__ int part[CC_THREADS];
  const int per = (h + CC_THREADS - 1) / CC_THREADS;
  for (int n = blockIdx.x; n < N; n += gridDim.x) {
    const int lo = min(h, (int)threadIdx.x * per), hi = min(h, lo + per);
    int s = 0;
    for (int y = lo; y < hi; ++y) s += rowcount[n * h + y];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int o = 1; o < CC_THREADS; o <<= 1) {                         // inclusive scan of the 256 partial sums
      const int v = threadIdx.x >= o ? part[threadIdx.x - o] : 0;
      __syncthreads();
      part[threadIdx.x] += v;
      __syncthreads();
    }
    int run = part[threadIdx.x] - s;
    for (int y = lo; y < hi; ++y) { rowbase[n * h + y] = run; run += rowcount[n * h + y]; }
    if (threadIdx.x == CC_THREADS - 1) counts[n] = part[CC_THREADS - 1];
    __syncthreads();
  }
}

__global__ __launch_bounds__(CC_THREADS) void cc_rank_kernel(int rows, int w, const int* __restrict__ root,
                                                             const int* __restrict__ rowbase, int* __restrict__ labels) {
  const int lane = threadIdx.x & 63, waves = CC_THREADS / 64;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (long long r = (long long)blockIdx.x * waves + (threadIdx.x >> 6); r < rows; r += (long long)gridDim.x * waves) {
    const int base = (int)r * w;
    int run = rowbase[r];
    for (int x0 = 0; x0 < w; x0 += 64) {                               // (uniform per wave)
      const int x = x0 + lane;
      const bool is_root = x < w && root[base + x] == base + x;
      const unsigned long long b = __ballot(is_root);
      if (is_root) labels[base + x] = run + __popcll(b & below) + 1;
      run += __popcll(b);
    }
  }
}

__global__ __launch_bounds__(CC_THREADS) void cc_relabel_kernel(int n_pix, const int* __restrict__ root, int* labels) {
  for (long long it = (long long)blockIdx.x * CC_THREADS + threadIdx.x; it < n_pix; it += (long long)gridDim.x * CC_THREADS) {
    const int i = (int)it, r = root[i];
    if (r < 0) labels[i] = 0;
    else if (r != i) labels[i] = labels[r];                            // labels[r] was written by cc_rank_kernel; roots are not rewritten here
  }
}

// ---- runs of equal keys inside a wave's 64 consecutive pixels of one row --------------------------------------------------------
// Returns whether this lane starts a run; *len = its length, *mask = its lanes.
__device__ __forceinline__ bool cc_run(int key, int lane, int* len, unsigned long long* mask) {
  const int prev = __shfl_up(key, 1);
  const bool head = lane == 0 || prev != key;
  const unsigned long long heads = __ballot(head);
  const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
  const int next = above ? lane + 1 + (__ffsll((long long)above) - 1) : 64;
  *len = next - lane;
  const unsigned long long upto = next == 64 ? ~0ull : (1ull << next) - 1ull;
  *mask = upto & ~((1ull << lane) - 1ull);
  return head;
}

__device__ __forceinline__ long long cc_row_items(int rows, int w) { return (long long)rows * ((w + 63) / 64); }

// area[root] += pixels, edge[root] |= touches the image edge (both zeroed by the launcher)
__global__ __launch_bounds__(CC_THREADS) void cc_area_kernel(int rows, int h, int w, const int* __restrict__ root, int* area, int* edge) {
  const int lane = threadIdx.x & 63, waves = CC_THREADS / 64, chunks = (w + 63) / 64;
  const long long items = cc_row_items(rows, w);
  for (long long it = (long long)blockIdx.x * waves + (threadIdx.x >> 6); it < items; it += (long long)gridDim.x * waves) {
    const int r = (int)(it / chunks), x = (int)(it % chunks) * 64 + lane, y = r % h;
    const int key = x < w ? root[r * w + x] : -2;
    int len;
    unsigned long long mask;
    if (cc_run(key, lane, &len, &mask) && key >= 0) {
      atomicAdd(&area[key], len);
      if (y == 0 || y == h - 1 || x == 0 || x + len - 1 == w - 1) atomicOr(&edge[key], 1);
    }
  }
}

struct CcCleanArgs {
  int n_pix, min_area, max_hole;
  const unsigned char* dec;
  const int *root, *area, *edge;
  unsigned char* out;
  float* out_logits;                     // nullable: +logit where the cleaned decision is foreground, -logit elsewhere
  float logit;
  unsigned long long* stats;             // components removed, pixels removed, holes filled, pixels filled (accumulated)
};

__global__ __launch_bounds__(CC_THREADS) void cc_clean_kernel(const CcCleanArgs a) {
  hpri_block_count4(a.stats, [&](unsigned int (&c)[4]) {
    for (long long it = (long long)blockIdx.x * CC_THREADS + threadIdx.x; it < a.n_pix; it += (long long)gridDim.x * CC_THREADS) {
      const int i = (int)it, r = a.root[i], ar = a.area[r];
      int fg = a.dec[i];
      if (fg) {
        if (ar < a.min_area) { fg = 0; c[1] += 1; c[0] += r == i; }
      } else if (a.edge[r] == 0 && ar <= a.max_hole) {
        fg = 1; c[3] += 1; c[2] += r == i;
      }
      a.out[i] = (unsigned char)fg;
      if (a.out_logits) a.out_logits[i] = fg ? a.logit : -a.logit;
    }
  });
}

// ---- measuring ------------------------------------------------------------------------------------------------------------------
#define CC_TABLE_COLS 6                  // area, y0, x0, y1, x1, overlap

__global__ void cc_offsets_kernel(int N, const int* __restrict__ counts, int* __restrict__ offsets) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    int run = 0;
    for (int n = 0; n < N; ++n) { offsets[n] = run; run += max(counts[n], 0); }
    offsets[N] = run;
  }
}

__global__ __launch_bounds__(CC_THREADS) void cc_table_init_kernel(int rows, int* __restrict__ table) {
  for (long long it = (long long)blockIdx.x * CC_THREADS + threadIdx.x; it < rows; it += (long long)gridDim.x * CC_THREADS) {
    int* t = table + it * CC_TABLE_COLS;
    t[0] = 0; t[1] = 0x7fffffff; t[2] = 0x7fffffff; t[3] = -1; t[4] = -1; t[5] = 0;
  }
}

__global__ __launch_bounds__(CC_THREADS) void cc_measure_kernel(int rows, int h, int w, const int* __restrict__ labels,
                                                                const int* __restrict__ offsets, const void* __restrict__ truth,
                                                                int truth_kind, int table_rows, int* table) {
  const int lane = threadIdx.x & 63, waves = CC_THREADS / 64, chunks = (w + 63) / 64;
  const long long items = cc_row_items(rows, w);
  for (long long it = (long long)blockIdx.x * waves + (threadIdx.x >> 6); it < items; it += (long long)gridDim.x * waves) {
    const int r = (int)(it / chunks), x = (int)(it % chunks) * 64 + lane, y = r % h, n = r / h;
    int key = 0, hit = 0;
    if (x < w) {
      key = labels[r * w + x];
      if (truth) hit = truth_kind == 0   ? ((int)reinterpret_cast<const float*>(truth)[r * w + x]) != 0
                       : truth_kind == 1 ? reinterpret_cast<const unsigned char*>(truth)[r * w + x] != 0
                                         : reinterpret_cast<const int*>(truth)[r * w + x] != 0;
    }
    const unsigned long long hits = __ballot(hit != 0);
    int len;
    unsigned long long mask;
    if (cc_run(key, lane, &len, &mask) && key > 0) {
      const long long row = (long long)offsets[n] + key - 1;
      if (row < table_rows) {                                          // (a table that does not match the labels is never overrun)
        int* t = table + row * CC_TABLE_COLS;
        atomicAdd(&t[0], len);
        atomicMin(&t[1], y);
        atomicMin(&t[2], x);
        atomicMax(&t[3], y);
        atomicMax(&t[4], x + len - 1);
        const int ov = __popcll(hits & mask);
        if (ov) atomicAdd(&t[5], ov);
      }
    }
  }
}

// ---- launchers ------------------------------------------------------------------------------------------------------------------
static inline int cc_grid(long long items, int per_block) { return hpri_grid_per_cu(items, per_block, 8); }      // eight workgroups per CU

static inline long long cc_dec_ints(long long n) { return (n + 3) / 4; }

// Workspace of either pipeline, in 32-bit words (pure host): parent, root, area, edge (n each), the decision map (n bytes), the
// per-row root counts and offsets (N*h each).
extern "C" size_t hpri_cc_workspace_ints(int N, int h, int w) {
  if (N <= 0 || h <= 0 || w <= 0) return 0;
  const long long n = (long long)N * h * w;
  return (size_t)(4 * n + cc_dec_ints(n) + 2LL * N * h);
}

extern "C" int hpri_cc_tile_h() { return CC_TILE_H; }
extern "C" int hpri_cc_tile_w() { return CC_TILE_W; }

struct CcWorkspace { int *parent, *root, *area, *edge, *rowcount, *rowbase; unsigned char* dec; };

static inline CcWorkspace cc_carve(int* ws, int N, int h, int w) {
  const long long n = (long long)N * h * w;
  CcWorkspace s;
  s.parent = ws; s.root = ws + n; s.area = ws + 2 * n; s.edge = ws + 3 * n;
  s.rowcount = ws + 4 * n; s.rowbase = s.rowcount + (long long)N * h;
  s.dec = reinterpret_cast<unsigned char*>(s.rowbase + (long long)N * h);
  return s;
}

#define CC_REQUIRE_MAP(who)                                                                                         \
  HPRI_REQUIRE(N > 0 && h > 0 && w > 0, who ": bad sizes");                                                         \
  HPRI_REQUIRE((long long)N * h * w < 2147483648LL, who ": N*h*w must be below 2^31");                              \
  HPRI_REQUIRE(connectivity == 4 || connectivity == 8, who ": connectivity must be 4 or 8")

// tile pass, border pass, flatten: root[i] and (rowcount != null) the roots per row
static int cc_forest(const CcDecision& d, const CcMode& m, int N, int h, int w, const CcWorkspace& s, bool count_rows, hipStream_t stream) {
  const long long n = (long long)N * h * w;
  const long long tiles = (long long)N * hpri_cdiv(h, CC_TILE_H) * hpri_cdiv(w, CC_TILE_W);
  hipLaunchKernelGGL(cc_tile_kernel, dim3(cc_grid(tiles, 1)), dim3(CC_THREADS), 0, stream, d, m, N, h, w, s.dec, s.parent);
  HPRI_CHECK_LAUNCH();
  hipLaunchKernelGGL(cc_border_kernel, dim3(cc_grid(n, CC_THREADS)), dim3(CC_THREADS), 0, stream, m, N, h, w, s.dec, s.parent);
  HPRI_CHECK_LAUNCH();
  hipLaunchKernelGGL(cc_flatten_kernel, dim3(cc_grid((long long)N * h, CC_THREADS / 64)), dim3(CC_THREADS), 0, stream, N * h, w,
                     s.parent, s.root, count_rows ? s.rowcount : nullptr);
  HPRI_CHECK_LAUNCH();
  return HPRI_OK;
}

// pred: contiguous (N, h, w); pred_kind 0 = fp32 decided by threshold / is_logits, 1 = uint8 decided by value != 0, 2 = fp32 mask
// decided by ((int)value) != 0 (1, 2: threshold and is_logits unused).  labels (N, h, w) int32, counts (N) int32.  workspace: hpri_cc_workspace_ints(N, h, w) 32-bit words.
extern "C" int hpri_cc_label(const void* pred, int pred_kind, float threshold, int is_logits, int invert, int N, int h, int w,
                             int connectivity, int* labels, int* counts, int* workspace, size_t ws_ints, hipStream_t stream) {
  HPRI_REQUIRE(pred && labels && counts && workspace, "cc_label: null pointer");
  HPRI_REQUIRE(pred_kind >= 0 && pred_kind <= 2, "cc_label: pred_kind must be 0 (fp32), 1 (uint8) or 2 (fp32 mask)");
  CC_REQUIRE_MAP("cc_label");
  if (ws_ints < hpri_cc_workspace_ints(N, h, w)) return hpri_set_error(HPRI_ERR_WORKSPACE, "cc_label: workspace too small");
  const CcWorkspace s = cc_carve(workspace, N, h, w);
  CcDecision d; d.pred = pred; d.kind = pred_kind; d.threshold = threshold; d.is_logits = is_logits; d.invert = invert != 0;
  CcMode m; m.act0 = 0; m.act1 = 1; m.diag0 = 0; m.diag1 = connectivity == 8;
  const int rc = cc_forest(d, m, N, h, w, s, true, stream);
  if (rc != HPRI_OK) return rc;
  const int rows = N * h, n = N * h * w;
  hipLaunchKernelGGL(cc_rowscan_kernel, dim3(cc_grid(N, 1)), dim3(CC_THREADS), 0, stream, N, h, s.rowcount, s.rowbase, counts);
  HPRI_CHECK_LAUNCH();
  hipLaunchKernelGGL(cc_rank_kernel, dim3(cc_grid(rows, CC_THREADS / 64)), dim3(CC_THREADS), 0, stream, rows, w, s.root, s.rowbase, labels);
  HPRI_CHECK_LAUNCH();
  hipLaunchKernelGGL(cc_relabel_kernel, dim3(cc_grid(n, CC_THREADS)), dim3(CC_THREADS), 0, stream, n, s.root, labels);
  HPRI_CHECK_LAUNCH();
  return HPRI_OK;
}

// labels, counts: what hpri_cc_label wrote.  truth (nullable): contiguous (N, h, w), truth_kind 0 = fp32, 1 = uint8, 2 = int32
// (another label map).  table: table_rows rows of six int32 (area, y0, x0, y1, x1, overlap), ordered by (image, label); table_rows >= sum(counts) (rows beyond it are never
// written, rows of the table beyond sum(counts) hold the empty row).  offsets: N + 1 int32 of scratch (the images' first rows).
extern "C" int hpri_cc_measure(const int* labels, const int* counts, const void* truth, int truth_kind, int N, int h, int w,
                               int* table, int table_rows, int* offsets, hipStream_t stream) {
  HPRI_REQUIRE(labels && counts && offsets, "cc_measure: null pointer");
  HPRI_REQUIRE(N > 0 && h > 0 && w > 0, "cc_measure: bad sizes");
  HPRI_REQUIRE((long long)N * h * w < 2147483648LL, "cc_measure: N*h*w must be below 2^31");
  HPRI_REQUIRE(table_rows >= 0 && (table || table_rows == 0), "cc_measure: bad table");
  HPRI_REQUIRE(truth_kind >= 0 && truth_kind <= 2, "cc_measure: truth_kind must be 0 (fp32), 1 (uint8) or 2 (int32)");
  if (table_rows == 0) return HPRI_OK;
  hipLaunchKernelGGL(cc_offsets_kernel, dim3(1), dim3(64), 0, stream, N, counts, offsets);
  HPRI_CHECK_LAUNCH();
  hipLaunchKernelGGL(cc_table_init_kernel, dim3(cc_grid(table_rows, CC_THREADS)), dim3(CC_THREADS), 0, stream, table_rows, table);
  HPRI_CHECK_LAUNCH();
  const long long items = (long long)N * h * ((w + 63) / 64);
  hipLaunchKernelGGL(cc_measure_kernel, dim3(cc_grid(items, CC_THREADS / 64)), dim3(CC_THREADS), 0, stream, N * h, h, w, labels, offsets,
                     truth, truth_kind, table_rows, table);
  HPRI_CHECK_LAUNCH();
  return HPRI_OK;
}

// pred, pred_kind, threshold, is_logits: as hpri_cc_label.  out: (N, h, w) uint8, the cleaned decision; out_logits (nullable):
// (N, h, w) fp32, +logit where it is foreground and -logit elsewhere.  stats: four int64 on the device, ACCUMULATED (as
// hpri_seg_counts' buffer): components removed, pixels removed, holes filled, pixels filled.
extern "C" int hpri_cc_clean(const void* pred, int pred_kind, float threshold, int is_logits, int N, int h, int w, int connectivity,
                             int min_area, int max_hole, unsigned char* out, float* out_logits, float logit, long long* stats,
                             int* workspace, size_t ws_ints, hipStream_t stream) {
  HPRI_REQUIRE(pred && out && stats && workspace, "cc_clean: null pointer");
  HPRI_REQUIRE(pred_kind >= 0 && pred_kind <= 2, "cc_clean: pred_kind must be 0 (fp32), 1 (uint8) or 2 (fp32 mask)");
  CC_REQUIRE_MAP("cc_clean");
  HPRI_REQUIRE(min_area >= 0 && max_hole >= 0, "cc_clean: min_area and max_hole must not be negative");
  if (ws_ints < hpri_cc_workspace_ints(N, h, w)) return hpri_set_error(HPRI_ERR_WORKSPACE, "cc_clean: workspace too small");
  const CcWorkspace s = cc_carve(workspace, N, h, w);
  CcDecision d; d.pred = pred; d.kind = pred_kind; d.threshold = threshold; d.is_logits = is_logits; d.invert = 0;
  CcMode m; m.act0 = 1; m.act1 = 1; m.diag1 = connectivity == 8; m.diag0 = !m.diag1;
  const int rc = cc_forest(d, m, N, h, w, s, false, stream);
  if (rc != HPRI_OK) return rc;
  const int n = N * h * w;
  if (hipMemsetAsync(s.area, 0, 2 * sizeof(int) * (size_t)n, stream) != hipSuccess)                  // area and edge lie side by side
    return hpri_set_error(HPRI_ERR_LAUNCH, "cc_clean: hipMemsetAsync failed");
  const long long items = (long long)N * h * ((w + 63) / 64);
  hipLaunchKernelGGL(cc_area_kernel, dim3(cc_grid(items, CC_THREADS / 64)), dim3(CC_THREADS), 0, stream, N * h, h, w, s.root, s.area, s.edge);
  HPRI_CHECK_LAUNCH();
  CcCleanArgs a;
  a.n_pix = n; a.min_area = min_area; a.max_hole = max_hole; a.dec = s.dec; a.root = s.root; a.area = s.area; a.edge = s.edge;
  a.out = out; a.out_logits = out_logits; a.logit = logit; a.stats = reinterpret_cast<unsigned long long*>(stats);
  hipLaunchKernelGGL(cc_clean_kernel, dim3(cc_grid(n, CC_THREADS)), dim3(CC_THREADS), 0, stream, a);
  HPRI_CHECK_LAUNCH();
  return HPRI_OK;
}
