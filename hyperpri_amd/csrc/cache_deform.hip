// Cube cache, deforming gather (hyperpri_amd/cache.py: CubeDeform, plan_epoch_deformed): the warp kernels' pass (cache_warp.hip)
// with one more input to the coordinate -- an elastic displacement field --, one more term in the value -- Gaussian noise from a
// counter-based generator -- and one choice of which sample a pixel belongs to -- a CutMix rectangle.
//
// Deform entry: 64 bytes = 16 32-bit words per sample, 16-byte aligned, in DEVICE memory, parallel to the warp entries:
//     word  0      int32  mix_from     batch index in [0, N) of the sample that owns the rectangle's pixels; anything else, or the
//                                      sample's own index: no CutMix
//     words 1..4   int32  ry0, ry1, rx0, rx1   the rectangle [ry0, ry1) x [rx0, rx1) in window coordinates, clamped into the window
//                                      by the kernels; empty: none
//     word  5      int32  nodes_off    offset in floats of this sample's lattice in the node table; negative: no elastic field
//     words 6, 7   int32  gy, gx       lattice rows and columns
//     word  8      fp32   inv_pitch    1 / node spacing in output pixels (both axes)
//     word  9      fp32   noise_sigma  noise is applied only when sigma > 0 (a NaN or a negative value: none)
//     words 10,11  uint32 k0, k1       the Philox key of this sample's noise
//     words 12..15 reserved, 0
//
// Field (hpri_elastic_field): (N, h, w, 2) fp32 = (dx, dy) in output pixels, the cubic B-spline of a coarse lattice of random
// displacements (Ronneberger et al., U-Net, 2015, section 3.1).  Per pixel ty = y * inv_pitch, iy = clamp(floor ty, 0, gy - 4),
// fy = ty - iy (x alike), d = sum_a sum_b B_a(fy) B_b(fx) node[iy + a][ix + b] with
//     B0 = (1-f)^3 / 6,  B1 = (3f^3 - 6f^2 + 4) / 6,  B2 = (-3f^3 + 3f^2 + 3f + 1) / 6,  B3 = f^3 / 6.
// A sample without a lattice, with gy < 4 or gx < 4, or whose [nodes_off, nodes_off + 2 gy gx) leaves [0, nodes_len), gets +0.
// The field is materialised (8 bytes per pixel against the 960 the gather writes) so that the cube and the mask kernel read the
// very same coordinates and the cube kernel's 60 lanes per pixel do not each walk sixteen nodes.
//
// Output pixel (y, x) of sample s (hpri_cube_deform / hpri_mask_deform):
//     owner   o = mix_from[s] when CutMix is on for s and (y, x) lies in its rectangle, else s (o's own CutMix words are ignored)
//     u = (x + field[o, y, x, 0]) - (w-1)/2,  v = (y + field[o, y, x, 1]) - (h-1)/2     (a null field counts as zeros)
//     sx, sy, bilinear / nearest sampling, gain, offset, band drop: cache_warp.hip's, with o's WARP entry
//     out = base, or fmaf(sigma[s], z, base) when sigma[s] > 0: the noise and its key are ALWAYS those of s.  Dropped channels and
//     pad channels [C, cs) stay exactly 0; the mask is never touched by noise.
// Noise: z from Philox4x32-10 (deform_math.h) under the key (k0, k1) at the counter (lo32 e, hi32 e, 0, 0),
// e = (y * w + x) * (cs / 4) + c0 / 4: one call per channel quad, words r0..r3 for channels c0..c0+3, (r0, r1) and (r2, r3) through
// Box-Muller.  No fast intrinsics, and this file must not be built with -ffast-math: the stream is documented bit for bit.
//
// The launchers cannot see the entries, so the kernels clamp as the warp kernels do, and the field kernel checks the lattice
// descriptor against nodes_len: a bad entry gives a wrong picture, never an access outside the allocations.
#include "cache_warp.h"
#include "deform_math.h"

struct DeformEntry { int mix_from, ry0, ry1, rx0, rx1; float sigma; unsigned k0, k1; };

// s's deform words as the cube / mask kernels use them: mix_from = -1 when there is no CutMix, the rectangle inside the window,
// sigma = 0 when there is no noise
__device__ __forceinline__ DeformEntry deform_entry(const int* __restrict__ deform, int s, int N, int h, int w) {
  const int4* e = reinterpret_cast<const int4*>(deform + 16 * (size_t)s);
  const int4 a = e[0], b = e[1], c = e[2];
  DeformEntry d;
  d.ry0 = max(a.y, 0); d.ry1 = min(a.z, h); d.rx0 = max(a.w, 0); d.rx1 = min(b.x, w);
  d.mix_from = (a.x >= 0 && a.x < N && a.x != s && d.ry0 < d.ry1 && d.rx0 < d.rx1) ? a.x : -1;
  const float sg = __int_as_float(c.y);
  d.sigma = sg > 0.f ? sg : 0.f;                                       // (a NaN compares false)
  d.k0 = (unsigned)c.z; d.k1 = (unsigned)c.w;
  return d;
}

// ---- the field: one output pixel per thread --------------------------------------------------------------------------
__device__ __forceinline__ void bspline4(float f, float B[4]) {
  const float g = 1.f - f, f2 = f * f, f3 = f2 * f;
  B[0] = g * g * g * (1.f / 6.f);
  B[1] = (3.f * f3 - 6.f * f2 + 4.f) * (1.f / 6.f);
  B[2] = (-3.f * f3 + 3.f * f2 + 3.f * f + 1.f) * (1.f / 6.f);
  B[3] = f3 * (1.f / 6.f);
}

__global__ __launch_bounds__(256) void elastic_field_kernel(const float* __restrict__ nodes, long long nodes_len, const int* __restrict__ deform,
                                                             int N, int h, int w, float* __restrict__ field) {
  const long long total = (long long)N * h * w;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int r = (int)(i / w), x = (int)(i - (long long)r * w);
    const int n = r / h, y = r - n * h;
    const int4* e = reinterpret_cast<const int4*>(deform + 16 * (size_t)n);
    const int4 b = e[1];
    const int off = b.y, gy = b.z, gx = b.w;
    const float inv_pitch = __int_as_float(e[2].x);
    float dx = 0.f, dy = 0.f;
    // (gy * gx <= nodes_len / 2 without forming the product: the descriptor is not trusted)
    if (nodes != nullptr && off >= 0 && gy >= 4 && gx >= 4 && (long long)gy <= nodes_len / 2 / gx &&
        (long long)off + 2LL * gy * gx <= nodes_len) {
      const float ty = (float)y * inv_pitch, tx = (float)x * inv_pitch;
      // clamped in floating point before the conversion (a NaN becomes 0), and once more as integers ((float)(g - 4) may round up)
      const int iy = min((int)fminf(fmaxf(floorf(ty), 0.f), (float)(gy - 4)), gy - 4);
      const int ix = min((int)fminf(fmaxf(floorf(tx), 0.f), (float)(gx - 4)), gx - 4);
      float By[4], Bx[4];
      bspline4(ty - (float)iy, By);
      bspline4(tx - (float)ix, Bx);
      const float2* nd = reinterpret_cast<const float2*>(nodes + off) + ((long long)iy * gx + ix);
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float wgt = By[a] * Bx[c];
          const float2 v = nd[(long long)a * gx + c];
          dx = fmaf(wgt, v.x, dx);
          dy = fmaf(wgt, v.y, dy);
        }
    }
    reinterpret_cast<float2*>(field)[i] = make_float2(dx, dy);
  }
}

// nodes: the flat fp32 node table of nodes_len floats (may be null when nodes_len is 0: every sample then gets zeros);
// deform: N deform entries on the device; field: (N, h, w, 2) fp32.
extern "C" int hpri_elastic_field(const float* nodes, long long nodes_len, const int* deform, int N, int h, int w, float* field,
                                  hipStream_t stream) {
  HPRI_REQUIRE(nodes_len >= 0, "elastic_field: nodes_len must not be negative");
  HPRI_REQUIRE(deform && field && (nodes || nodes_len == 0), "elastic_field: null pointer");
  HPRI_REQUIRE(N > 0, "elastic_field: bad sizes");
  HPRI_REQUIRE(h > 0 && w > 0 && h <= 4096 && w <= 4096, "elastic_field: the window must be 1 .. 4096 pixels a side");
  HPRI_REQUIRE((long long)N * h < 0x7FFFFFFFLL, "elastic_field: window too large");
  // (the node table is read as (dx, dy) pairs: 8 bytes)
  HPRI_REQUIRE(((uintptr_t)deform & 15) == 0 && ((uintptr_t)field & 15) == 0 && ((uintptr_t)nodes & 7) == 0,
               "elastic_field: buffers must be 16-byte aligned (the node table: 8)");
  long long blocks = ((long long)N * h * w + 255) / 256;
  const long long cap = 8LL * hpri_cu_count();
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(elastic_field_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, nodes, nodes_len, deform, N, h, w, field);
  HPRI_CHECK_LAUNCH();
  return HPRI_OK;
}

// ---- the cube: cube_warp_kernel's work items ---------------------------------------------------------------------------
// A workgroup takes WARP_ITEM consecutive channel quads of one window row (s, y).  The row's deform entry is uniform, and so are
// the two warp entries a lane can belong to -- s's own and its CutMix partner's --: the choice between them is per lane (a row
// that crosses a rectangle edge), made by selects, not by branches.  Order inside an item: the field loads of both unroll steps,
// the coordinates and all 4 * WARP_UNROLL neighbour loads, then -- while those are in flight -- Philox and Box-Muller for a noisy
// sample (a uniform branch), then the conversion, the bilinear sum and the store.  Only loads and the store depend on the row tail.
// Registers: the per-lane owner choice and the four normals per unroll step do not fit cube_warp_kernel's 64 (eight waves per
// SIMD); this kernel is built for six waves per SIMD (80 registers): the compiler's report shows 77 for fp32 slots, 71 for fp16, no spill.
template <typename T>
__global__ __launch_bounds__(WARP_THREADS) __attribute__((amdgpu_waves_per_eu(6, 6))) void cube_deform_kernel(
    const T* __restrict__ cache, int slots, int Hs, int Ws, int q, int C, const int* __restrict__ entries, const int* __restrict__ deform,
    const float* __restrict__ field, int N, int h, int w, float* __restrict__ dst) {
  const int rowq = w * q;                                             // quads per window row (< 2^30: checked by the launcher)
  const int pieces = (rowq + WARP_ITEM - 1) / WARP_ITEM;
  const long long items = (long long)N * h * pieces;
  const long long slot_elems = (long long)Hs * Ws * (4LL * q);
  const float uc = 0.5f * (float)(w - 1), vc = 0.5f * (float)(h - 1);
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    const int r = (int)(it / pieces), piece = (int)(it - (long long)r * pieces);
    const int n = r / h, y = r - n * h;
    const DeformEntry de = deform_entry(deform, n, N, h, w);
    const bool rowin = de.mix_from >= 0 && y >= de.ry0 && y < de.ry1;
    const int p = rowin ? de.mix_from : n;                            // the only other owner this row can have
    const WarpEntry gs = warp_entry(entries, n, slots, 4 * q), gp = warp_entry(entries, p, slots, 4 * q);
    const long long row_s = ((long long)n * h + y) * w, row_p = ((long long)p * h + y) * w;   // pixels before this row, per owner
    float* d = dst + (long long)r * rowq * 4LL;
    const int j0 = piece * WARP_ITEM + threadIdx.x;
    typedef typename WarpRaw<T>::type raw_t;
    raw_t t[WARP_UNROLL][4];
    float wt[WARP_UNROLL][4];
    float2 disp[WARP_UNROLL];
    float z[WARP_UNROLL][4];
    // the displacement of every lane's pixel, from its owner's field
#pragma unroll
    for (int k = 0; k < WARP_UNROLL; ++k) {
      const int j = j0 + k * WARP_THREADS;
      const int x = j / q;
      const bool mine = rowin && x >= de.rx0 && x < de.rx1;
      disp[k] = make_float2(0.f, 0.f);
      if (field != nullptr && j < rowq) disp[k] = reinterpret_cast<const float2*>(field)[(mine ? row_p : row_s) + x];
    }
#pragma unroll
    for (int k = 0; k < WARP_UNROLL; ++k) {
      const int j = j0 + k * WARP_THREADS;
      const bool live = j < rowq;
      const int x = j / q, c0 = 4 * (j - x * q);
      const bool mine = rowin && x >= de.rx0 && x < de.rx1;
      const float a00 = mine ? gp.a00 : gs.a00, a01 = mine ? gp.a01 : gs.a01, cx = mine ? gp.cx : gs.cx;
      const float a10 = mine ? gp.a10 : gs.a10, a11 = mine ? gp.a11 : gs.a11, cy = mine ? gp.cy : gs.cy;
      const T* s = cache + (mine ? gp.slot : gs.slot) * slot_elems;
      const float u = ((float)x + disp[k].x) - uc, v = ((float)y + disp[k].y) - vc;
      const float sx = warp_coord(a00, a01, cx, u, v, Ws), sy = warp_coord(a10, a11, cy, u, v, Hs);
      const float fx0 = floorf(sx), fy0 = floorf(sy);
      const float fx = sx - fx0, fy = sy - fy0;
      const int x0 = (int)fx0, y0 = (int)fy0;                        // in [-1, Ws] x [-1, Hs]
      wt[k][0] = (1.f - fy) * (1.f - fx); wt[k][1] = (1.f - fy) * fx; wt[k][2] = fy * (1.f - fx); wt[k][3] = fy * fx;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int xi = x0 + (b & 1), yi = y0 + (b >> 1);
        t[k][b] = raw_t{0, 0, 0, 0};
        if (live && wt[k][b] != 0.f && xi >= 0 && xi < Ws && yi >= 0 && yi < Hs) t[k][b] = *reinterpret_cast<const raw_t*>(s + ((long long)yi * Ws + xi) * (4LL * q) + c0);
      }
    }
    // the noise of s, while the loads are in flight: e = (y * w + x) * q + c0 / 4 = y * rowq + j
    const bool noisy = de.sigma > 0.f;
#pragma unroll
    for (int k = 0; k < WARP_UNROLL; ++k) {
      z[k][0] = z[k][1] = z[k][2] = z[k][3] = 0.f;
      if (noisy) {
        uint32_t bits[4];
        hpri_deform_bits(de.k0, de.k1, (uint64_t)((long long)y * rowq + (j0 + k * WARP_THREADS)), bits);
        hpri_deform_normals(bits, z[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < WARP_UNROLL; ++k) {
      const int j = j0 + k * WARP_THREADS;
      const int x = j / q, c0 = 4 * (j - x * q);
      const bool mine = rowin && x >= de.rx0 && x < de.rx1;
      const float gain = mine ? gp.gain : gs.gain, offset = mine ? gp.offset : gs.offset;
      const int drop_lo = mine ? gp.drop_lo : gs.drop_lo, drop_hi = mine ? gp.drop_hi : gs.drop_hi;
      const f32x4 t0 = warp_widen(t[k][0]), t1 = warp_widen(t[k][1]), t2 = warp_widen(t[k][2]), t3 = warp_widen(t[k][3]);
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float acc = wt[k][0] * t0[e];
        acc = fmaf(wt[k][1], t1[e], acc);
        acc = fmaf(wt[k][2], t2[e], acc);
        acc = fmaf(wt[k][3], t3[e], acc);
        const int c = c0 + e;
        const float base = fmaf(gain, acc, offset);
        const float val = noisy ? fmaf(de.sigma, z[k][e], base) : base;
        o[e] = (c >= C || (c >= drop_lo && c < drop_hi)) ? 0.f : val;
      }
      if (j < rowq) *reinterpret_cast<f32x4*>(d + 4LL * j) = o;
    }
  }
}

// hpri_cube_warp's arguments plus deform (N deform entries on the device) and field ((N, h, w, 2) fp32 from hpri_elastic_field,
// or null: no displacement).
extern "C" int hpri_cube_deform(const void* cache, int cache_dtype, int slots, int Hs, int Ws, int cs, int C, const int* entries,
                                const int* deform, const float* field, int N, int h, int w, float* dst, hipStream_t stream) {
  HPRI_REQUIRE(cache && entries && deform && dst, "cube_deform: null pointer");
  HPRI_REQUIRE(cache_dtype == 0 || cache_dtype == 1, "cube_deform: cache_dtype must be 0 (f32) or 1 (f16)");
  HPRI_REQUIRE(slots > 0 && Hs > 0 && Ws > 0 && N > 0, "cube_deform: bad sizes");
  HPRI_REQUIRE(cs > 0 && cs % 8 == 0, "cube_deform: the channel stride must be a multiple of 8");
  HPRI_REQUIRE(C > 0 && C <= cs, "cube_deform: the band count must lie in (0, cs]");
  HPRI_REQUIRE(h > 0 && w > 0 && h <= 4096 && w <= 4096, "cube_deform: the window must be 1 .. 4096 pixels a side");
  HPRI_REQUIRE((long long)w * (cs / 4) < 0x40000000LL && (long long)N * h < 0x7FFFFFFFLL, "cube_deform: window too large");
  HPRI_REQUIRE(((uintptr_t)cache & 15) == 0 && ((uintptr_t)dst & 15) == 0 && ((uintptr_t)entries & 15) == 0 &&
                   ((uintptr_t)deform & 15) == 0 && ((uintptr_t)field & 15) == 0, "cube_deform: buffers must be 16-byte aligned");
  const int q = cs / 4;
  const long long pieces = ((long long)w * q + WARP_ITEM - 1) / WARP_ITEM;
  long long blocks = (long long)N * h * pieces;
  const long long cap = 6LL * hpri_cu_count();                      // six workgroups per CU (the kernel's occupancy), grid-stride over the rest
  if (blocks > cap) blocks = cap;
  if (cache_dtype == 0)
    hipLaunchKernelGGL(cube_deform_kernel<float>, dim3((unsigned)blocks), dim3(WARP_THREADS), 0, stream, (const float*)cache, slots,
                       Hs, Ws, q, C, entries, deform, field, N, h, w, dst);
  else
    hipLaunchKernelGGL(cube_deform_kernel<_Float16>, dim3((unsigned)blocks), dim3(WARP_THREADS), 0, stream, (const _Float16*)cache,
                       slots, Hs, Ws, q, C, entries, deform, field, N, h, w, dst);
  HPRI_CHECK_LAUNCH();
  return HPRI_OK;
}

// ---- the mask: one output pixel per thread, the image's owner and coordinates, nearest neighbour ------------------------
__global__ __launch_bounds__(256) void mask_deform_kernel(const unsigned char* __restrict__ masks, int slots, int Hs, int Ws,
                                                           const int* __restrict__ entries, const int* __restrict__ deform,
                                                           const float* __restrict__ field, int N, int h, int w, float* __restrict__ dst) {
  const long long total = (long long)N * h * w;
  const float uc = 0.5f * (float)(w - 1), vc = 0.5f * (float)(h - 1);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int r = (int)(i / w), x = (int)(i - (long long)r * w);
    const int n = r / h, y = r - n * h;
    const DeformEntry de = deform_entry(deform, n, N, h, w);
    const bool mine = de.mix_from >= 0 && y >= de.ry0 && y < de.ry1 && x >= de.rx0 && x < de.rx1;
    const int o = mine ? de.mix_from : n;
    const WarpEntry g = warp_entry(entries, o, slots, 8);
    float2 disp = make_float2(0.f, 0.f);
    if (field != nullptr) disp = reinterpret_cast<const float2*>(field)[((long long)o * h + y) * w + x];
    const float u = ((float)x + disp.x) - uc, v = ((float)y + disp.y) - vc;
    const float sx = warp_coord(g.a00, g.a01, g.cx, u, v, Ws), sy = warp_coord(g.a10, g.a11, g.cy, u, v, Hs);
    const int xs = (int)floorf(sx + 0.5f), ys = (int)floorf(sy + 0.5f);       // in [-1, Ws] x [-1, Hs]
    float out = 0.f;
    if (xs >= 0 && xs < Ws && ys >= 0 && ys < Hs) out = (float)masks[((long long)g.slot * Hs + ys) * Ws + xs];
    dst[i] = out;
  }
}

// masks: uint8 (slots, Hs, Ws); dst: fp32 (N, 1, h, w); entries, deform and field of hpri_cube_deform.
extern "C" int hpri_mask_deform(const unsigned char* masks, int slots, int Hs, int Ws, const int* entries, const int* deform,
                                const float* field, int N, int h, int w, float* dst, hipStream_t stream) {
  HPRI_REQUIRE(masks && entries && deform && dst, "mask_deform: null pointer");
  HPRI_REQUIRE(slots > 0 && Hs > 0 && Ws > 0 && N > 0, "mask_deform: bad sizes");
  HPRI_REQUIRE(h > 0 && w > 0 && h <= 4096 && w <= 4096, "mask_deform: the window must be 1 .. 4096 pixels a side");
  HPRI_REQUIRE((long long)N * h < 0x7FFFFFFFLL, "mask_deform: window too large");
  HPRI_REQUIRE(((uintptr_t)entries & 15) == 0 && ((uintptr_t)deform & 15) == 0 && ((uintptr_t)field & 15) == 0,
               "mask_deform: the entries and the field must be 16-byte aligned");
  long long blocks = ((long long)N * h * w + 255) / 256;
  const long long cap = 8LL * hpri_cu_count();
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(mask_deform_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, masks, slots, Hs, Ws, entries, deform, field, N, h,
                     w, dst);
  HPRI_CHECK_LAUNCH();
  return HPRI_OK;
}

// ---- host: the generator of deform_math.h through the C ABI (tests pin the stream without a GPU) -------------------------
// bits4: the four Philox words of counter (lo32 e, hi32 e, 0, 0) under the key (k0, k1); z4: their four normals (either may be null).
extern "C" int hpri_deform_noise_host(unsigned int k0, unsigned int k1, unsigned long long e, unsigned int* bits4, float* z4) {
  HPRI_REQUIRE(bits4 || z4, "deform_noise_host: null pointer");
  uint32_t r[4];
  hpri_deform_bits(k0, k1, e, r);
  if (bits4) for (int i = 0; i < 4; ++i) bits4[i] = r[i];
  if (z4) hpri_deform_normals(r, z4);
  return HPRI_OK;
}
