// Cube cache, deforming gather: what is the deformation's alone -- the displacement field the deforming kernels of cache_warp.hip
// read (the deform entry's layout is documented there), and the host entry of their noise generator.
//
// Field (hpri_elastic_field): (N, h, w, 2) fp32 = (dx, dy) in output pixels, the cubic B-spline of a coarse lattice of random
// displacements (Ronneberger et al., U-Net, 2015, section 3.1).  Per pixel ty = y * inv_pitch, iy = clamp(floor ty, 0, gy - 4),
// fy = ty - iy (x alike), d = sum_a sum_b B_a(fy) B_b(fx) node[iy + a][ix + b] with
//     B0 = (1-f)^3 / 6,  B1 = (3f^3 - 6f^2 + 4) / 6,  B2 = (-3f^3 + 3f^2 + 3f + 1) / 6,  B3 = f^3 / 6.
// A sample without a lattice, with gy < 4 or gx < 4, or whose [nodes_off, nodes_off + 2 gy gx) leaves [0, nodes_len), gets +0.
// The field is materialised (8 bytes per pixel against the 960 the gather writes) so that the cube and the mask kernel read the
// very same coordinates and the cube kernel's 60 lanes per pixel do not each walk sixteen nodes.  The launcher cannot see the
// entries, so the kernel checks the lattice descriptor against nodes_len: a bad entry gives a wrong picture, never an access
// outside the allocations.
#include "cache_launch.h"
#include "deform_math.h"

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
  const CachePass p = {"elastic_field", 1, 1, 1, N, h, w, false};      // (no slots are read)
  CACHE_REQUIRE(p.who, nodes_len >= 0, "nodes_len must not be negative");
  CACHE_REQUIRE(p.who, deform && field && (nodes || nodes_len == 0), "null pointer");
  if (int e = cache_check(p)) return e;
  // (the node table is read as (dx, dy) pairs: 8 bytes)
  CACHE_REQUIRE(p.who, hpri_aligned16(deform, field) && ((uintptr_t)nodes & 7) == 0, "buffers must be 16-byte aligned (the node table: 8)");
  hipLaunchKernelGGL(elastic_field_kernel, cache_grid(cache_pixel_blocks(p), 8), dim3(256), 0, stream, nodes, nodes_len, deform, N, h, w,
                     field);
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
