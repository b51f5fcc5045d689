// A stable, grouped LSD radix sort of fp32 keys, and its two consumers: the Lovasz hinge loss and the ranking metrics (AP, ROC AUC).
//
// The sort.  G groups of L keys, contiguous (G, L).  perm[g][r] is the index inside group g of the key of rank r, in the order of
// torch.sort(keys[g], descending, stable=True): by numeric value, NaN above +inf, -0.0 == +0.0, denormals in their order, ties in
// ascending index order.  A key becomes an order-preserving uint32 (sort_encode: NaN and -0.0 canonicalised first; descending = the
// complement), sorted ascending by four 8-bit digits, least significant first.  Launches:
//   memset + sort_hist_kernel      the digit histograms of all four passes per group (LDS counts, then integer atomics)
//   per pass  sort_count_kernel    the digit counts of every tile of SORT_TILE keys            counts[g][digit][tile]
//             sort_scan_kernel     one workgroup per (digit, group): counts -> the tile's first position of that digit in the group
//                                  (digits below it from the histogram, tiles before it by an exclusive scan), in place
//             sort_scatter_kernel  position = counts[g][digit][tile] + rank inside the tile
// The rank inside a tile is STABLE by construction: an element is (round k, wave, lane) = index k * 256 + wave * 64 + lane of its
// tile; eight ballots give the mask of the wave's lanes that hold the same digit, the popcount of the lanes below is the rank among
// them, the lowest lane stores the count of slot (k, wave) and digit, and the thread that owns a digit scans its 32 slots in order.
// No atomic decides a position.  A pass whose histogram has one occupied bin is the identity for that group: every workgroup of
// its three launches reads that from the histogram and leaves (sort_plan), and the later launches find the data where the last
// pass that ran left it -- pass 0 reads the caller's keys, so there is no initial copy either.  Between workgroups there is no
// synchronisation but the kernel boundary: no chained scan, no look-back, no flag (a predecessor that is not resident would hang it).
//
// Lovasz hinge (Berman et al., CVPR 2018).  s = y >= 0.5 ? +1 : -1, e = 1 - x s (fp32; x s is exact), a group's pixels ordered by e
// descending with the sort (the keys are formed as they are read; an ignored pixel reads as -inf and counts for nothing), then
//   lz_count_kernel   positives per tile of ranks
//   lz_weight_kernel  G1 and the positives before the tile (sums over the tile counts), an integer scan inside the tile, and per rank
//                     w_r = 1 / U_r (positive) or I_r / ((U_r - 1) U_r) (negative), I_r = G1 - P_r, U_r = G1 + r + 1 - P_r; G1 == 0: w_0 = 1
//                     in fp64 from the integer counts, rounded once; an fp64 partial sum of relu(e) w per tile; the coefficient
//                     -s w / groups (0 where e <= 0) scattered back through the permutation
//   lz_finish_kernel  one workgroup adds the partial sums in a fixed order: the mean over the groups
// The backward is one elementwise launch: the coefficient times the upstream scalar.
//
// Ranking metrics.  One descending sort of the scores, then runs of equal scores: rk_tile_kernel (positives and the last run start
// per tile), rk_run_kernel (at every run end: p_run tp / (r + 1) in fp64 and p_run (2 negatives below + n_run) in uint64),
// rk_finish_kernel; n_run: the negatives of the run (ties count half).  The divisions by P and by 2 P N are the caller's.
#include "tail_helpers.h"
#include <math.h>

#define SORT_THREADS 256
#define SORT_WAVES (SORT_THREADS / 64)
#define SORT_ITEMS 8                              // keys of one thread
#define SORT_TILE (SORT_THREADS * SORT_ITEMS)     // keys one workgroup ranks per pass
#define SORT_SLOTS (SORT_ITEMS * SORT_WAVES)      // (round, wave) pairs of a tile, in index order
#define SORT_BINS 256
#define SORT_PASSES 4
#define SORT_MAX_GROUPS 65535                     // the groups are a grid dimension

// where a launch finds its keys: the caller's (hinge == 0), or the hinge errors of (x, y) formed on the fly
struct SortKeys {
  const float* keys;
  const float* x; const float* y;
  int hinge, use_ignore;
  float ignore;
  int descending;
};

struct SortWs {
  unsigned* hist;                 // [G][SORT_PASSES][SORT_BINS]
  unsigned* counts;               // [G][SORT_BINS][tiles]
  unsigned* key[2]; int* idx[2];  // ping and pong, [G][L] each
};

// e = 1 - x s; an ignored pixel sorts behind everything and has no error
__device__ __forceinline__ float lz_error(float x, float y, int use_ignore, float ignore) {
  if (use_ignore && y == ignore) return -INFINITY;
  return 1.f - x * (y >= 0.5f ? 1.f : -1.f);
}

// ascending order of the result = the order of the contract (descending: the complement, which keeps ties in index order)
__device__ __forceinline__ unsigned sort_encode(float v, int descending) {
  unsigned b = __float_as_uint(v);
  if (b == 0x80000000u) b = 0;                                   // -0.0 == +0.0
  unsigned u = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  if (v != v) u = 0xFFFFFFFFu;                                   // every NaN, whatever its sign and payload, above +inf
  return descending ? ~u : u;
}

__device__ __forceinline__ unsigned sort_source_key(const SortKeys& s, size_t i) {
  const float v = s.hinge ? lz_error(s.x[i], s.y[i], s.use_ignore, s.ignore) : s.keys[i];
  return sort_encode(v, s.descending);
}

// ---- workgroup helpers (every thread of the SORT_THREADS calls them; red: SORT_WAVES entries of LDS) ------------------------------
template <typename T> __device__ __forceinline__ T sort_block_sum(T v, T* red) {
  v = hpri_wave_sum(v);
  __syncthreads();                                               // the last use of red is over
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  T s = red[0];
#pragma unroll
  for (int w = 1; w < SORT_WAVES; ++w) s += red[w];
  return s;
}

__device__ __forceinline__ int sort_block_max(int v, int* red) {
  v = hpri_wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int s = red[0];
#pragma unroll
  for (int w = 1; w < SORT_WAVES; ++w) s = max(s, red[w]);
  return s;
}

// exclusive prefix sum over the threads in thread order; total: the sum of all
__device__ __forceinline__ unsigned sort_block_scan(unsigned v, unsigned* red, unsigned& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned n = __shfl_up(inc, o);
    if (lane >= o) inc += n;
  }
  __syncthreads();
  if (lane == 63) red[wave] = inc;
  __syncthreads();
  unsigned off = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < SORT_WAVES; ++w) {
    if (w < wave) off += red[w];
    total += red[w];
  }
  return off + inc - v;
}

// exclusive prefix maximum over the threads in thread order (-1: nothing before)
__device__ __forceinline__ int sort_block_scan_max(int v, int* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int n = __shfl_up(inc, o);
    if (lane >= o) inc = max(inc, n);
  }
  __syncthreads();
  if (lane == 63) red[wave] = inc;
  __syncthreads();
  int ex = __shfl_up(inc, 1);
  if (lane == 0) ex = -1;
#pragma unroll
  for (int w = 0; w < SORT_WAVES; ++w)
    if (w < wave) ex = max(ex, red[w]);
  return ex;
}

// The passes below `upto` that are no identity for this group (the return value: where the data lies), and whether pass `upto` is
// one (skip; upto == SORT_PASSES: not asked).  Read from the group's histograms by every workgroup itself: no host read.
__device__ __forceinline__ int sort_plan(const unsigned* __restrict__ hist_g, int L, int upto, bool& skip) {
  int done = 0;
  skip = false;
  for (int q = 0; q <= upto && q < SORT_PASSES; ++q) {
    const int single = __syncthreads_or(hist_g[q * SORT_BINS + threadIdx.x] == (unsigned)L);
    if (q < upto) done += single ? 0 : 1;
    else skip = single != 0;
  }
  return done;
}

// The index of rank r in the final order (from: the half sort_plan names, null = no pass ran, the identity).  A permutation, so
// always inside the group; the clamp keeps an order that is not one from leaving the caller's buffers.
__device__ __forceinline__ int sort_index_at(const int* __restrict__ from, size_t base, long long r, int L) {
  if (!from) return (int)r;
  const unsigned j = (unsigned)from[base + r];
  return (int)(j < (unsigned)L ? j : (unsigned)L - 1u);
}

// ------------------------------------------------------------------------------------------------
// The sort
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SORT_THREADS) void sort_hist_kernel(SortKeys src, unsigned* __restrict__ hist, int L) {
  __shared__ unsigned h[SORT_PASSES * SORT_BINS];
  const size_t base = (size_t)blockIdx.y * L;
  for (int i = threadIdx.x; i < SORT_PASSES * SORT_BINS; i += SORT_THREADS) h[i] = 0;
  __syncthreads();
  for (long long i = (long long)blockIdx.x * SORT_THREADS + threadIdx.x; i < L; i += (long long)gridDim.x * SORT_THREADS) {
    const unsigned u = sort_source_key(src, base + i);
#pragma unroll
    for (int q = 0; q < SORT_PASSES; ++q) atomicAdd(&h[q * SORT_BINS + ((u >> (8 * q)) & 255)], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < SORT_PASSES * SORT_BINS; i += SORT_THREADS)
    if (h[i]) atomicAdd(&hist[(size_t)blockIdx.y * SORT_PASSES * SORT_BINS + i], h[i]);
}

__global__ __launch_bounds__(SORT_THREADS) void sort_count_kernel(SortKeys src, SortWs ws, int L, int tiles, int pass) {
  __shared__ unsigned h[SORT_BINS];
  const int g = blockIdx.y, tile = blockIdx.x;
  bool skip;
  const int done = sort_plan(ws.hist + (size_t)g * SORT_PASSES * SORT_BINS, L, pass, skip);
  if (skip) return;
  const size_t base = (size_t)g * L;
  const unsigned* from = done ? ws.key[(done - 1) & 1] : nullptr;
  h[threadIdx.x] = 0;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < SORT_ITEMS; ++k) {
    const long long i = (long long)tile * SORT_TILE + k * SORT_THREADS + threadIdx.x;
    if (i < L) {
      const unsigned u = from ? from[base + i] : sort_source_key(src, base + i);
      atomicAdd(&h[(u >> (8 * pass)) & 255], 1u);
    }
  }
  __syncthreads();
  ws.counts[((size_t)g * SORT_BINS + threadIdx.x) * tiles + tile] = h[threadIdx.x];
}

__global__ __launch_bounds__(SORT_THREADS) void sort_scan_kernel(SortWs ws, int L, int tiles, int pass) {
  __shared__ unsigned red[SORT_WAVES];
  const int g = blockIdx.y, digit = blockIdx.x;
  const unsigned* hist_g = ws.hist + (size_t)g * SORT_PASSES * SORT_BINS;
  bool skip;
  (void)sort_plan(hist_g, L, pass, skip);
  if (skip) return;
  unsigned carry = sort_block_sum((int)threadIdx.x < digit ? hist_g[pass * SORT_BINS + threadIdx.x] : 0u, red);
  unsigned* c = ws.counts + ((size_t)g * SORT_BINS + digit) * tiles;
  for (int b = 0; b < tiles; b += SORT_THREADS) {
    const int j = b + threadIdx.x;
    const unsigned v = j < tiles ? c[j] : 0u;
    unsigned total;
    const unsigned ex = sort_block_scan(v, red, total);
    if (j < tiles) c[j] = carry + ex;
    carry += total;
  }
}

__global__ __launch_bounds__(SORT_THREADS) void sort_scatter_kernel(SortKeys src, SortWs ws, int L, int tiles, int pass) {
  __shared__ unsigned cnt[SORT_SLOTS][SORT_BINS];
  const int g = blockIdx.y, tile = blockIdx.x;
  bool skip;
  const int done = sort_plan(ws.hist + (size_t)g * SORT_PASSES * SORT_BINS, L, pass, skip);
  if (skip) return;
  const size_t base = (size_t)g * L;
  const unsigned* from_key = done ? ws.key[(done - 1) & 1] : nullptr;
  const int* from_idx = done ? ws.idx[(done - 1) & 1] : nullptr;
  unsigned* to_key = ws.key[done & 1];
  int* to_idx = ws.idx[done & 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;

  for (int i = threadIdx.x; i < SORT_SLOTS * SORT_BINS; i += SORT_THREADS) (&cnt[0][0])[i] = 0;
  __syncthreads();

  unsigned key[SORT_ITEMS];
  int idx[SORT_ITEMS], rank[SORT_ITEMS];
#pragma unroll
  for (int k = 0; k < SORT_ITEMS; ++k) {
    const long long i = (long long)tile * SORT_TILE + k * SORT_THREADS + threadIdx.x;
    const bool valid = i < L;
    key[k] = 0; idx[k] = 0;
    if (valid) {
      key[k] = from_key ? from_key[base + i] : sort_source_key(src, base + i);
      idx[k] = from_idx ? from_idx[base + i] : (int)i;
    }
    const unsigned d = (key[k] >> (8 * pass)) & 255;
    unsigned long long peers = __ballot(valid);                // the lanes of this wave that hold the same digit
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1;
      const unsigned long long m = __ballot(bit);
      peers &= bit ? m : ~m;
    }
    rank[k] = __popcll(peers & below);
    if (valid && rank[k] == 0) cnt[k * SORT_WAVES + wave][d] = (unsigned)__popcll(peers);
  }
  __syncthreads();
  {                                                            // thread = digit: its slots in index order, after the tiles before
    unsigned run = ws.counts[((size_t)g * SORT_BINS + threadIdx.x) * tiles + tile];
#pragma unroll 8
    for (int s = 0; s < SORT_SLOTS; ++s) {
      const unsigned c = cnt[s][threadIdx.x];
      cnt[s][threadIdx.x] = run;
      run += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < SORT_ITEMS; ++k) {
    const long long i = (long long)tile * SORT_TILE + k * SORT_THREADS + threadIdx.x;
    if (i < L) {
      const unsigned d = (key[k] >> (8 * pass)) & 255;
      const unsigned pos = cnt[k * SORT_WAVES + wave][d] + (unsigned)rank[k];
      if (pos < (unsigned)L) {                                 // (always, with the counts of the same keys)
        to_key[base + pos] = key[k];
        to_idx[base + pos] = idx[k];
      }
    }
  }
}

__global__ __launch_bounds__(SORT_THREADS) void sort_finish_kernel(const float* __restrict__ keys, SortWs ws, int L, int* __restrict__ perm,
                                                                   float* __restrict__ sorted) {
  bool skip;
  const int done = sort_plan(ws.hist + (size_t)blockIdx.y * SORT_PASSES * SORT_BINS, L, SORT_PASSES, skip);
  const size_t base = (size_t)blockIdx.y * L;
  const int* from = done ? ws.idx[(done - 1) & 1] : nullptr;
  for (long long i = (long long)blockIdx.x * SORT_THREADS + threadIdx.x; i < L; i += (long long)gridDim.x * SORT_THREADS) {
    const int j = sort_index_at(from, base, i, L);
    perm[base + i] = j;
    if (sorted) sorted[base + i] = keys[base + j];
  }
}

// ------------------------------------------------------------------------------------------------
// Lovasz hinge
// ------------------------------------------------------------------------------------------------
struct LzArgs {
  const float* x; const float* y;
  SortWs ws;
  unsigned* tsum;                 // [G][tiles] positives of a tile of ranks
  double* partial;                // [G][tiles]
  float* coef;                    // [G][L]: -s w / groups where e > 0, else 0
  int L, tiles, use_ignore;
  float ignore;
  double inv_groups;
};

__global__ __launch_bounds__(SORT_THREADS) void lz_count_kernel(LzArgs a) {
  __shared__ unsigned red[SORT_WAVES];
  const int g = blockIdx.y, tile = blockIdx.x;
  bool skip;
  const int done = sort_plan(a.ws.hist + (size_t)g * SORT_PASSES * SORT_BINS, a.L, SORT_PASSES, skip);
  const int* from = done ? a.ws.idx[(done - 1) & 1] : nullptr;
  const size_t base = (size_t)g * a.L;
  unsigned c = 0;
#pragma unroll
  for (int k = 0; k < SORT_ITEMS; ++k) {
    const long long r = (long long)tile * SORT_TILE + k * SORT_THREADS + threadIdx.x;
    if (r < a.L) {
      const float yv = a.y[base + sort_index_at(from, base, r, a.L)];
      c += (yv >= 0.5f && !(a.use_ignore && yv == a.ignore)) ? 1u : 0u;
    }
  }
  c = sort_block_sum(c, red);
  if (threadIdx.x == 0) a.tsum[(size_t)g * a.tiles + tile] = c;
}

__global__ __launch_bounds__(SORT_THREADS) void lz_weight_kernel(LzArgs a) {
  __shared__ unsigned red[SORT_WAVES];
  __shared__ double dred[1][SORT_THREADS];
  const int g = blockIdx.y, tile = blockIdx.x;
  bool skip;
  const int done = sort_plan(a.ws.hist + (size_t)g * SORT_PASSES * SORT_BINS, a.L, SORT_PASSES, skip);
  const int* from = done ? a.ws.idx[(done - 1) & 1] : nullptr;
  const size_t base = (size_t)g * a.L;

  unsigned before = 0, all = 0;                                // positives of the tiles before this one, and of the group
  for (int j = threadIdx.x; j < a.tiles; j += SORT_THREADS) {
    const unsigned v = a.tsum[(size_t)g * a.tiles + j];
    all += v;
    if (j < tile) before += v;
  }
  const long long G1 = sort_block_sum(all, red);
  before = sort_block_sum(before, red);

  const long long r0 = (long long)tile * SORT_TILE + (long long)threadIdx.x * SORT_ITEMS;       // this thread's consecutive ranks
  float e[SORT_ITEMS];
  int id[SORT_ITEMS];
  unsigned lab = 0;
#pragma unroll
  for (int k = 0; k < SORT_ITEMS; ++k) {
    e[k] = -INFINITY; id[k] = 0;
    if (r0 + k < a.L) {
      id[k] = sort_index_at(from, base, r0 + k, a.L);
      const float yv = a.y[base + id[k]];
      e[k] = lz_error(a.x[base + id[k]], yv, a.use_ignore, a.ignore);
      if (yv >= 0.5f && !(a.use_ignore && yv == a.ignore)) lab |= 1u << k;
    }
  }
  unsigned total;
  long long P = (long long)before + sort_block_scan((unsigned)__popc(lab), red, total);
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < SORT_ITEMS; ++k) {
    const long long r = r0 + k;
    if (r < a.L) {
      const bool pos = (lab >> k) & 1;
      P += pos ? 1 : 0;
      float c = 0.f;
      if (e[k] > 0.f) {
        const double U = (double)(G1 + (r + 1 - P)), I = (double)(G1 - P);
        const double w = G1 == 0 ? (r == 0 ? 1.0 : 0.0) : (pos ? 1.0 / U : I / ((U - 1.0) * U));
        acc += (double)e[k] * w;
        c = (float)((pos ? -w : w) * a.inv_groups);
      }
      a.coef[base + id[k]] = c;
    }
  }
  const double s1[1] = {acc};
  hpri_block_sum(dred, s1);
  if (threadIdx.x == 0) a.partial[(size_t)g * a.tiles + tile] = dred[0][0];
}

// one workgroup: wave w takes groups w, w + 4, ...; its lanes stride over the group's tiles, a xor butterfly adds them
__global__ __launch_bounds__(SORT_THREADS) void lz_finish_kernel(const double* __restrict__ partial, int groups, int tiles,
                                                                 float* __restrict__ loss) {
  __shared__ double wsum[SORT_WAVES];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double acc = 0.0;
  for (int g = wave; g < groups; g += SORT_WAVES) {
    double v = 0.0;
    for (int j = lane; j < tiles; j += 64) v += partial[(size_t)g * tiles + j];
    acc += hpri_wave_sum(v);
  }
  if (lane == 0) wsum[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double l = 0.0;
    for (int w = 0; w < SORT_WAVES; ++w) l += wsum[w];
    loss[0] = (float)(l / (double)groups);
  }
}

__global__ __launch_bounds__(SORT_THREADS) void lz_bwd_kernel(const float* __restrict__ coef, long long n, const float* __restrict__ gout,
                                                              float* __restrict__ dx) {
  const float g = gout ? gout[0] : 1.f;
  for (long long i = (long long)blockIdx.x * SORT_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * SORT_THREADS) dx[i] = coef[i] * g;
}

// ------------------------------------------------------------------------------------------------
// Ranking metrics over the runs of equal scores of one descending order
// ------------------------------------------------------------------------------------------------
struct RkArgs {
  const float* scores; const void* target;
  int kind;                        // 0: fp32, 1: uint8; non-zero = positive
  SortWs ws;
  int L, tiles;
  unsigned* tsum;                  // [tiles] positives
  int* tstart;                     // [tiles] the last rank of the tile that begins a run (-1: none)
  unsigned* texcl;                 // [tiles] positives of the tile before that rank
  double* pap;                     // [tiles]
  unsigned long long* pu;          // [tiles]
};

// this thread's SORT_ITEMS consecutive ranks from r0: bit k of lab / st / en = rank r0 + k is positive / begins / ends a run
__device__ __forceinline__ void rk_load(const RkArgs& a, int done, long long r0, unsigned& lab, unsigned& st, unsigned& en) {
  const unsigned* keys = done ? a.ws.key[(done - 1) & 1] : nullptr;
  const int* from = done ? a.ws.idx[(done - 1) & 1] : nullptr;
  lab = st = en = 0;
  unsigned prev = 0;
  if (r0 > 0 && r0 <= a.L) prev = keys ? keys[r0 - 1] : sort_encode(a.scores[r0 - 1], 1);
#pragma unroll
  for (int k = 0; k <= SORT_ITEMS; ++k) {
    const long long r = r0 + k;
    bool begins = false;
    if (r < a.L) {
      const unsigned u = keys ? keys[r] : sort_encode(a.scores[r], 1);
      begins = r == 0 || u != prev;
      prev = u;
      if (k < SORT_ITEMS) {
        const int i = sort_index_at(from, 0, r, a.L);
        const bool pos = a.kind ? reinterpret_cast<const unsigned char*>(a.target)[i] != 0 : reinterpret_cast<const float*>(a.target)[i] != 0.f;
        if (pos) lab |= 1u << k;
      }
    }
    if (k < SORT_ITEMS && begins) st |= 1u << k;
    if (k > 0 && r - 1 < a.L && (begins || r == a.L)) en |= 1u << (k - 1);
  }
}

__global__ __launch_bounds__(SORT_THREADS) void rk_tile_kernel(RkArgs a) {
  __shared__ unsigned red[SORT_WAVES];
  __shared__ int ired[SORT_WAVES];
  const int tile = blockIdx.x;
  bool skip;
  const int done = sort_plan(a.ws.hist, a.L, SORT_PASSES, skip);
  const long long r0 = (long long)tile * SORT_TILE + (long long)threadIdx.x * SORT_ITEMS;
  unsigned lab, st, en;
  rk_load(a, done, r0, lab, st, en);
  const unsigned sum = sort_block_sum((unsigned)__popc(lab), red);
  const int mine = st ? (int)(r0 + (31 - __clz((int)st))) : -1;
  const int last = sort_block_max(mine, ired);
  unsigned c = 0;
#pragma unroll
  for (int k = 0; k < SORT_ITEMS; ++k)
    if (((lab >> k) & 1) && r0 + k < last) ++c;
  c = sort_block_sum(c, red);
  if (threadIdx.x == 0) { a.tsum[tile] = sum; a.tstart[tile] = last; a.texcl[tile] = c; }
}

__global__ __launch_bounds__(SORT_THREADS) void rk_run_kernel(RkArgs a) {
  __shared__ unsigned red[SORT_WAVES];
  __shared__ int ired[SORT_WAVES];
  __shared__ unsigned long long ured[SORT_WAVES];
  __shared__ unsigned at_start[SORT_THREADS];
  __shared__ double dred[1][SORT_THREADS];
  const int tile = blockIdx.x;
  bool skip;
  const int done = sort_plan(a.ws.hist, a.L, SORT_PASSES, skip);

  unsigned before = 0, all = 0;
  int tp = -1;                                                 // the last earlier tile in which a run begins
  for (int j = threadIdx.x; j < a.tiles; j += SORT_THREADS) {
    const unsigned v = a.tsum[j];
    all += v;
    if (j < tile) {
      before += v;
      if (a.tstart[j] >= 0) tp = j;
    }
  }
  const long long positives = sort_block_sum(all, red);
  before = sort_block_sum(before, red);
  tp = sort_block_max(tp, ired);
  long long carry_start = -1, carry_P = 0;                     // the run that reaches into this tile: its first rank, the positives before it
  if (tp >= 0) {
    unsigned c = 0;
    for (int j = threadIdx.x; j < tp; j += SORT_THREADS) c += a.tsum[j];
    carry_P = (long long)sort_block_sum(c, red) + a.texcl[tp];
    carry_start = a.tstart[tp];
  }

  const long long tile0 = (long long)tile * SORT_TILE, r0 = tile0 + (long long)threadIdx.x * SORT_ITEMS;
  unsigned lab, st, en;
  rk_load(a, done, r0, lab, st, en);
  unsigned total;
  const long long P0 = (long long)before + sort_block_scan((unsigned)__popc(lab), red, total);
  int mine = -1;                                               // this thread's last run start, and the positives before it
  {
    long long P = P0;
    unsigned pb = 0;
#pragma unroll
    for (int k = 0; k < SORT_ITEMS; ++k) {
      if ((st >> k) & 1) { mine = (int)(r0 + k); pb = (unsigned)P; }
      P += (lab >> k) & 1;
    }
    at_start[threadIdx.x] = pb;
  }
  const int ex = sort_block_scan_max(mine, ired);              // (its barriers publish at_start)
  long long cur_start = carry_start, cur_P = carry_P;
  if (ex >= 0) { cur_start = ex; cur_P = at_start[(ex - tile0) / SORT_ITEMS]; }

  const long long negatives = (long long)a.L - positives;
  double ap = 0.0;
  unsigned long long u = 0;
  long long P = P0;
#pragma unroll
  for (int k = 0; k < SORT_ITEMS; ++k) {
    const long long r = r0 + k;
    if ((st >> k) & 1) { cur_start = r; cur_P = P; }
    P += (lab >> k) & 1;
    if ((en >> k) & 1) {
      const long long p_run = P - cur_P, n_run = (r - cur_start + 1) - p_run, fp = r + 1 - P;      // n_run: the run's negatives
      ap += (double)p_run * ((double)P / (double)(r + 1));
      u += (unsigned long long)p_run * (unsigned long long)(2 * (negatives - fp) + n_run);
    }
  }
  const double s1[1] = {ap};
  hpri_block_sum(dred, s1);
  u = sort_block_sum(u, ured);
  if (threadIdx.x == 0) { a.pap[tile] = dred[0][0]; a.pu[tile] = u; }
}

// out: the fp64 sum of p_run tp / (r + 1), then as 64-bit integers the sum of p_run (2 negatives below + n_run) and the positives
__global__ __launch_bounds__(SORT_THREADS) void rk_finish_kernel(RkArgs a, unsigned long long* __restrict__ out) {
  __shared__ unsigned long long ured[SORT_WAVES];
  __shared__ double dred[1][SORT_THREADS];
  double ap = 0.0;
  unsigned long long u = 0, p = 0;
  for (int j = threadIdx.x; j < a.tiles; j += SORT_THREADS) { ap += a.pap[j]; u += a.pu[j]; p += a.tsum[j]; }
  const double s1[1] = {ap};
  hpri_block_sum(dred, s1);
  u = sort_block_sum(u, ured);
  p = sort_block_sum(p, ured);
  if (threadIdx.x == 0) { out[0] = (unsigned long long)__double_as_longlong(dred[0][0]); out[1] = u; out[2] = p; }
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
struct SortLayout { size_t hist, counts, key[2], idx[2], bytes; int tiles; };

static inline size_t sort_up16(size_t v) { return (v + 15) & ~(size_t)15; }

static SortLayout sort_layout(int G, int L) {
  SortLayout s;
  const size_t n = (size_t)G * (size_t)L;
  s.tiles = (int)hpri_cdiv64(L, SORT_TILE);
  size_t at = 0;
  s.hist = at;   at += sort_up16((size_t)G * SORT_PASSES * SORT_BINS * sizeof(unsigned));
  s.counts = at; at += sort_up16((size_t)G * SORT_BINS * (size_t)s.tiles * sizeof(unsigned));
  for (int b = 0; b < 2; ++b) { s.key[b] = at; at += sort_up16(n * sizeof(unsigned)); }
  for (int b = 0; b < 2; ++b) { s.idx[b] = at; at += sort_up16(n * sizeof(int)); }
  s.bytes = at;
  return s;
}

static inline bool sort_sizes_ok(long long G, long long L) {
  return G >= 1 && L >= 1 && G <= SORT_MAX_GROUPS && G * L < (1ll << 31);
}

static SortWs sort_ws(const SortLayout& s, void* workspace) {
  char* p = reinterpret_cast<char*>(workspace);
  SortWs w;
  w.hist = reinterpret_cast<unsigned*>(p + s.hist);
  w.counts = reinterpret_cast<unsigned*>(p + s.counts);
  for (int b = 0; b < 2; ++b) { w.key[b] = reinterpret_cast<unsigned*>(p + s.key[b]); w.idx[b] = reinterpret_cast<int*>(p + s.idx[b]); }
  return w;
}

// the 14 launches that leave the order in the workspace (sort_plan says in which half)
static int sort_core(const SortKeys& src, const SortLayout& s, const SortWs& w, int G, int L, hipStream_t stream) {
  if (hipMemsetAsync(w.hist, 0, (size_t)G * SORT_PASSES * SORT_BINS * sizeof(unsigned), stream) != hipSuccess) {
    (void)hipGetLastError();
    return hpri_set_error(HPRI_ERR_LAUNCH, "sort: clearing the histograms failed");
  }
  const int hist_blocks = s.tiles < 128 ? s.tiles : 128;
  hipLaunchKernelGGL(sort_hist_kernel, dim3(hist_blocks, G), dim3(SORT_THREADS), 0, stream, src, w.hist, L);
  HPRI_CHECK_LAUNCH();
  for (int pass = 0; pass < SORT_PASSES; ++pass) {
    hipLaunchKernelGGL(sort_count_kernel, dim3(s.tiles, G), dim3(SORT_THREADS), 0, stream, src, w, L, s.tiles, pass);
    HPRI_CHECK_LAUNCH();
    hipLaunchKernelGGL(sort_scan_kernel, dim3(SORT_BINS, G), dim3(SORT_THREADS), 0, stream, w, L, s.tiles, pass);
    HPRI_CHECK_LAUNCH();
    hipLaunchKernelGGL(sort_scatter_kernel, dim3(s.tiles, G), dim3(SORT_THREADS), 0, stream, src, w, L, s.tiles, pass);
    HPRI_CHECK_LAUNCH();
  }
  return HPRI_OK;
}

extern "C" int hpri_sort_tile(void) { return SORT_TILE; }

extern "C" size_t hpri_sort_workspace_bytes(int G, int L) {
  if (!sort_sizes_ok(G, L)) return 0;
  return sort_layout(G, L).bytes;
}

extern "C" int hpri_sort_keys_f32(const float* keys, int G, int L, int descending, int* perm, float* sorted_keys, void* workspace,
                                  size_t workspace_bytes, hipStream_t stream) {
  HPRI_REQUIRE(keys && perm && workspace, "sort_keys_f32: null pointer");
  HPRI_REQUIRE(G >= 1 && L >= 1, "sort_keys_f32: G and L must be at least 1");
  HPRI_REQUIRE(sort_sizes_ok(G, L), "sort_keys_f32: G beyond 65535 or G*L beyond 2^31");
  HPRI_REQUIRE(hpri_aligned16(workspace), "sort_keys_f32: workspace not 16-byte aligned");
  const SortLayout s = sort_layout(G, L);
  if (workspace_bytes < s.bytes) return hpri_set_error(HPRI_ERR_WORKSPACE, "sort_keys_f32: workspace too small");
  const SortWs w = sort_ws(s, workspace);
  SortKeys src = {};
  src.keys = keys; src.descending = descending ? 1 : 0;
  if (int rc = sort_core(src, s, w, G, L, stream)) return rc;
  hipLaunchKernelGGL(sort_finish_kernel, dim3(hpri_grid_per_cu(L, SORT_THREADS, 8), G), dim3(SORT_THREADS), 0, stream, keys, w, L, perm,
                     sorted_keys);
  HPRI_CHECK_LAUNCH();
  return HPRI_OK;
}

// ---- Lovasz hinge -------------------------------------------------------------------------------
struct LzLayout { SortLayout sort; size_t partial, order, tsum, bytes; int G, L; };

static bool lz_layout(int N, long long per_image, int per_image_groups, LzLayout& z) {
  if (N < 1 || per_image < 1) return false;
  const long long G = per_image_groups ? N : 1, L = per_image_groups ? per_image : (long long)N * per_image;
  if (per_image >= (1ll << 31) || !sort_sizes_ok(G, L) || (long long)N * per_image >= (1ll << 31)) return false;
  z.G = (int)G; z.L = (int)L;
  z.sort = sort_layout(z.G, z.L);
  size_t at = 0;
  z.partial = at; at += sort_up16((size_t)z.G * z.sort.tiles * sizeof(double));
  z.order = at;   at += z.sort.bytes;
  z.tsum = at;    at += sort_up16((size_t)z.G * z.sort.tiles * sizeof(unsigned));
  z.bytes = at;
  return true;
}

extern "C" size_t hpri_lovasz_hinge_workspace_bytes(int N, long long per_image, int per_image_groups) {
  LzLayout z;
  return lz_layout(N, per_image, per_image_groups, z) ? z.bytes : 0;
}

extern "C" int hpri_lovasz_hinge_fwd(const float* logits, const float* target, int N, long long per_image, int per_image_groups,
                                     int use_ignore, int ignore_index, float* loss, float* coef, void* workspace, size_t workspace_bytes,
                                     hipStream_t stream) {
  HPRI_REQUIRE(logits && target && loss && coef && workspace, "lovasz_hinge_fwd: null pointer");
  HPRI_REQUIRE(N >= 1 && per_image >= 1, "lovasz_hinge_fwd: N and the pixels of an image must be at least 1");
  LzLayout z;
  HPRI_REQUIRE(lz_layout(N, per_image, per_image_groups, z), "lovasz_hinge_fwd: more than 65535 groups or N*pixels beyond 2^31");
  HPRI_REQUIRE(hpri_aligned16(workspace), "lovasz_hinge_fwd: workspace not 16-byte aligned");
  if (workspace_bytes < z.bytes) return hpri_set_error(HPRI_ERR_WORKSPACE, "lovasz_hinge_fwd: workspace too small");
  char* p = reinterpret_cast<char*>(workspace);
  const SortWs w = sort_ws(z.sort, p + z.order);
  SortKeys src = {};
  src.x = logits; src.y = target; src.hinge = 1; src.use_ignore = use_ignore ? 1 : 0; src.ignore = (float)ignore_index; src.descending = 1;
  if (int rc = sort_core(src, z.sort, w, z.G, z.L, stream)) return rc;
  LzArgs a = {};
  a.x = logits; a.y = target; a.ws = w;
  a.tsum = reinterpret_cast<unsigned*>(p + z.tsum); a.partial = reinterpret_cast<double*>(p + z.partial); a.coef = coef;
  a.L = z.L; a.tiles = z.sort.tiles; a.use_ignore = src.use_ignore; a.ignore = src.ignore; a.inv_groups = 1.0 / (double)z.G;
  hipLaunchKernelGGL(lz_count_kernel, dim3(a.tiles, z.G), dim3(SORT_THREADS), 0, stream, a);
  HPRI_CHECK_LAUNCH();
  hipLaunchKernelGGL(lz_weight_kernel, dim3(a.tiles, z.G), dim3(SORT_THREADS), 0, stream, a);
  HPRI_CHECK_LAUNCH();
  hipLaunchKernelGGL(lz_finish_kernel, dim3(1), dim3(SORT_THREADS), 0, stream, a.partial, z.G, a.tiles, loss);
  HPRI_CHECK_LAUNCH();
  return HPRI_OK;
}

extern "C" int hpri_lovasz_hinge_bwd(const float* coef, long long n, const float* grad_out, float* dlogits, hipStream_t stream) {
  HPRI_REQUIRE(coef && dlogits, "lovasz_hinge_bwd: null pointer");
  HPRI_REQUIRE(n >= 1 && n < (1ll << 31), "lovasz_hinge_bwd: n must lie in [1, 2^31)");
  hipLaunchKernelGGL(lz_bwd_kernel, dim3(hpri_grid_per_cu(n, SORT_THREADS, 8)), dim3(SORT_THREADS), 0, stream, coef, n, grad_out, dlogits);
  HPRI_CHECK_LAUNCH();
  return HPRI_OK;
}

// ---- ranking metrics ----------------------------------------------------------------------------
struct RkLayout { SortLayout sort; size_t pap, pu, order, tsum, tstart, texcl, bytes; };

static RkLayout rk_layout(int n) {
  RkLayout k;
  k.sort = sort_layout(1, n);
  const size_t t = (size_t)k.sort.tiles;
  size_t at = 0;
  k.pap = at;    at += sort_up16(t * sizeof(double));
  k.pu = at;     at += sort_up16(t * sizeof(unsigned long long));
  k.order = at;  at += k.sort.bytes;
  k.tsum = at;   at += sort_up16(t * sizeof(unsigned));
  k.tstart = at; at += sort_up16(t * sizeof(int));
  k.texcl = at;  at += sort_up16(t * sizeof(unsigned));
  k.bytes = at;
  return k;
}

extern "C" size_t hpri_ranking_workspace_bytes(long long n) {
  if (n < 1 || n >= (1ll << 31)) return 0;
  return rk_layout((int)n).bytes;
}

extern "C" int hpri_ranking_sums(const float* scores, const void* target, int target_kind, long long n, unsigned long long* out,
                                 void* workspace, size_t workspace_bytes, hipStream_t stream) {
  HPRI_REQUIRE(scores && target && out && workspace, "ranking_sums: null pointer");
  HPRI_REQUIRE(n >= 1 && n < (1ll << 31), "ranking_sums: n must lie in [1, 2^31)");
  HPRI_REQUIRE(target_kind == 0 || target_kind == 1, "ranking_sums: target_kind must be 0 (fp32) or 1 (uint8)");
  HPRI_REQUIRE(hpri_aligned16(workspace), "ranking_sums: workspace not 16-byte aligned");
  const RkLayout k = rk_layout((int)n);
  if (workspace_bytes < k.bytes) return hpri_set_error(HPRI_ERR_WORKSPACE, "ranking_sums: workspace too small");
  char* p = reinterpret_cast<char*>(workspace);
  const SortWs w = sort_ws(k.sort, p + k.order);
  SortKeys src = {};
  src.keys = scores; src.descending = 1;
  if (int rc = sort_core(src, k.sort, w, 1, (int)n, stream)) return rc;
  RkArgs a = {};
  a.scores = scores; a.target = target; a.kind = target_kind; a.ws = w; a.L = (int)n; a.tiles = k.sort.tiles;
  a.tsum = reinterpret_cast<unsigned*>(p + k.tsum); a.tstart = reinterpret_cast<int*>(p + k.tstart);
  a.texcl = reinterpret_cast<unsigned*>(p + k.texcl); a.pap = reinterpret_cast<double*>(p + k.pap);
  a.pu = reinterpret_cast<unsigned long long*>(p + k.pu);
  hipLaunchKernelGGL(rk_tile_kernel, dim3(a.tiles), dim3(SORT_THREADS), 0, stream, a);
  HPRI_CHECK_LAUNCH();
  hipLaunchKernelGGL(rk_run_kernel, dim3(a.tiles), dim3(SORT_THREADS), 0, stream, a);
  HPRI_CHECK_LAUNCH();
  hipLaunchKernelGGL(rk_finish_kernel, dim3(1), dim3(SORT_THREADS), 0, stream, a, out);
  HPRI_CHECK_LAUNCH();
  return HPRI_OK;
}
