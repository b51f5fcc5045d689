// The noise generator of the deforming gather (cache_warp.hip), shared by the device kernel and the host entry
// hpri_deform_noise_host: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123
// constants) and the Box-Muller transform of its four output words.  Plain integer and fp32 arithmetic, no fast intrinsics: the
// integer stream is the same on both sides bit for bit, the normals differ by the few ulps the two math libraries differ by.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define HPRI_HD __host__ __device__
#else
#define HPRI_HD
#endif

#define HPRI_PHILOX_M0 0xD2511F53u
#define HPRI_PHILOX_M1 0xCD9E8D57u
#define HPRI_PHILOX_W0 0x9E3779B9u
#define HPRI_PHILOX_W1 0xBB67AE85u

// ctr[0..3] -> ten rounds under the key (k0, k1), in place
HPRI_HD inline void hpri_philox4x32_10(uint32_t ctr[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)HPRI_PHILOX_M0 * ctr[0], p1 = (uint64_t)HPRI_PHILOX_M1 * ctr[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ ctr[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ ctr[3] ^ k1;
    ctr[0] = n0; ctr[1] = (uint32_t)p1; ctr[2] = n2; ctr[3] = (uint32_t)p0;
    k0 += HPRI_PHILOX_W0; k1 += HPRI_PHILOX_W1;
  }
}

// the counter of one channel quad: (lo32(e), hi32(e), 0, 0)
HPRI_HD inline void hpri_deform_bits(uint32_t k0, uint32_t k1, uint64_t e, uint32_t out[4]) {
  out[0] = (uint32_t)e; out[1] = (uint32_t)(e >> 32); out[2] = 0u; out[3] = 0u;
  hpri_philox4x32_10(out, k0, k1);
}

// a word's upper 23 bits as a point of (0, 1): ((r >> 9) + 1/2) * 2^-23, exact in fp32, in [2^-24, 1 - 2^-24]
HPRI_HD inline float hpri_unit(uint32_t r) { return ((float)(r >> 9) + 0.5f) * 1.1920928955078125e-07f; }

#if defined(__HIP_DEVICE_COMPILE__)
#define HPRI_COSPIF(x_) cospif(x_)
#define HPRI_SINPIF(x_) sinpif(x_)
#else                                            // (no cospif / sinpif in every host libm: through fp64, rounded once)
#define HPRI_COSPIF(x_) ((float)cos(3.14159265358979323846 * (double)(x_)))
#define HPRI_SINPIF(x_) ((float)sin(3.14159265358979323846 * (double)(x_)))
#endif

// Box-Muller of a pair of words: |z| <= sqrt(-2 ln 2^-24) < 5.77
HPRI_HD inline void hpri_box_muller(uint32_t ra, uint32_t rb, float* za, float* zb) {
  const float ua = hpri_unit(ra), ub = hpri_unit(rb);
  const float rad = sqrtf(-2.f * logf(ua));
  *za = rad * HPRI_COSPIF(2.f * ub);
  *zb = rad * HPRI_SINPIF(2.f * ub);
}

// the four normals of one channel quad: words (r0, r1) and (r2, r3) pair up
HPRI_HD inline void hpri_deform_normals(const uint32_t r[4], float z[4]) {
  hpri_box_muller(r[0], r[1], &z[0], &z[1]);
  hpri_box_muller(r[2], r[3], &z[2], &z[3]);
}
