// What the cube cache's launchers (cache.hip, cache_warp.hip, cache_deform.hip) require of their arguments and how they size
// their grids: every rule once.  A failed requirement is reported as "<entry>: <rule>", in the order the checks are written.
#pragma once
#include <stdio.h>
#include "tail_helpers.h"            // hpri_aligned16, hpri_grid_per_cu

typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

// one pass over an (N, h, w) window of (slots, Hs, Ws) frames; fit: the window must lie inside the frame (the copying gather --
// the resampling passes fill what lies outside with zeros and take any window up to 4096 pixels a side)
struct CachePass { const char* who; int slots, Hs, Ws, N, h, w; bool fit; };

static inline int cache_fail(const char* who, const char* rule) {
  char msg[200];
  snprintf(msg, sizeof(msg), "%s: %s", who, rule);
  return hpri_set_error(HPRI_ERR_ARG, msg);
}

#define CACHE_REQUIRE(who, cond, rule) do { if (!(cond)) return cache_fail(who, rule); } while (0)

// the slots a cube pass reads: element type (0 = float32, 1 = float16), channel stride, bands held (the copying gather: the stride)
struct CacheSlots { int dtype, cs, C; };

// What a pass requires of its sizes, in the order it is reported.  Without `c`: one thread per output pixel (masks, the elastic
// field).  (u = x - (w-1)/2 is exact in fp32 up to 4096; rows (n, y) and the channel quads of a row are indexed by an int.)
static inline int cache_check(const CachePass& p, const CacheSlots* c = nullptr) {
  if (c) CACHE_REQUIRE(p.who, c->dtype == 0 || c->dtype == 1, "cache_dtype must be 0 (f32) or 1 (f16)");
  CACHE_REQUIRE(p.who, p.slots > 0 && p.Hs > 0 && p.Ws > 0 && p.N > 0, "bad sizes");
  if (c) CACHE_REQUIRE(p.who, c->cs > 0 && c->cs % 8 == 0, "the channel stride must be a multiple of 8");
  if (c) CACHE_REQUIRE(p.who, c->C > 0 && c->C <= c->cs, "the band count must lie in (0, cs]");
  if (p.fit) CACHE_REQUIRE(p.who, p.h > 0 && p.w > 0 && p.h <= p.Hs && p.w <= p.Ws, "the window does not fit the frame");
  else CACHE_REQUIRE(p.who, p.h > 0 && p.w > 0 && p.h <= 4096 && p.w <= 4096, "the window must be 1 .. 4096 pixels a side");
  CACHE_REQUIRE(p.who, (long long)p.N * p.h < 0x7FFFFFFFLL && (!c || (long long)p.w * (c->cs / 4) < 0x40000000LL), "window too large");
  return HPRI_OK;
}

// blocks = min(items, per_cu x CUs): the kernels stride over the rest (items >= 1 after cache_check and the launchers' own checks)
static inline dim3 cache_grid(long long items, int per_cu) { return dim3(hpri_grid_per_cu(items, 1, per_cu)); }
// work items of `item` consecutive channel quads of one window row / workgroups of 256 pixels
static inline long long cache_row_items(const CachePass& p, int q, int item) { return (long long)p.N * p.h * (((long long)p.w * q + item - 1) / item); }
static inline long long cache_pixel_blocks(const CachePass& p) { return ((long long)p.N * p.h * p.w + 255) / 256; }
