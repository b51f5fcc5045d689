// Winograd F(2x2, 3x3) in exact fp32 on the CDNA4 matrix cores (v_mfma_f32_32x32x2_f32): the WEIGHT GRADIENT of the 3x3 / pad-1 /
// stride-1 convolutions of DoubleConv (reference model_parts.py:22,25; models.py:169,177 and their autograd) and the fixed-order
// reductions of its partial slabs.  Forward and data gradient of the same transform: conv_wino4.hip.
//
// The direct implicit GEMM spends 36 multiplies per 2x2 outputs and channel pair; Winograd's minimal filtering spends 16:
//     V = B^T d B   (4x4 input tile d, per input channel)         B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1]
//     U = G g G^T   (3x3 filter g, per channel pair; packed once) G   = [1 0 0; .5 .5 .5; .5 -.5 .5; 0 0 1]
//     M[xi] = sum_cin V[xi] * U[xi]   for the 16 frequencies xi   (16 GEMMs: [tiles x Cin] x [Cin x Cout])
//     Y = A^T M A   (2x2 outputs)                                 A^T = [1 1 1 0; 0 1 -1 -1]
// i.e. 2.25x fewer MFMAs in the same arithmetic type (cuDNN runs the reference's fp32 convolutions the same way);
// results differ from the direct sum by fp32 rounding of the transforms only (measured: profiles/r02_precision_error.json).
#include "common.h"

typedef float f32x2 __attribute__((ext_vector_type(2)));

// Floats of a packed transformed filter U: 16 frequencies x (K rounded up to 8) x Ncols_pad (layout: hpri_wino4_pack, conv_wino4.hip).
extern "C" size_t hpri_wino_packed_floats(int K, int Ncols_pad) { return (size_t)hpri_cdiv(K, 8) * 16 * 8 * Ncols_pad; }

// =====================================================================================================================
// Winograd weight gradient.  With M = U (.) V and Y = A^T M A, the gradient of the transformed filter is
//     dU[xi][cin][cout] = sum over tiles  V[xi][tile][cin] * dM[xi][tile][cout],   dM = A dY A^T   (A = [1 0; 1 1; 1 -1; 0 -1])
// and dg = G^T dU G: again 16 instead of 36 multiplies per 2x2 output pixels and channel pair.  Sixteen GEMMs whose
// reduction runs over the TILES: MFMA rows = cin, columns = cout, k = tile; both operands are transformed in registers.
//
//   workgroup  8 waves, wave (a, b) owns frequencies (a, 2b), (a, 2b+1) of one 64 (cin) x 64 (cout) block:
//              2 x 2 x 2 accumulator tiles = 128 VGPRs; it walks a contiguous run of strips ("split-K" over the tiles) and
//              writes ONE partial slab ws[split][xi][cin][cout]; hpri_wino_wgrad_reduce sums the slabs in a fixed order
//              (deterministic) and applies G^T . G on the way into the OIHW gradient.
//   stage      one strip of 16 tiles (2 output rows x 32 columns): input halo 4 x 34 pixels x 64 cin and dY 2 x 32 pixels
//              x 64 cout, both [pixel][channel] by LDS-DMA (lanes index the channel PAIR: every ds_read_b64 is a pixel's 256
//              consecutive bytes), double buffered; 64 MFMAs per wave, one barrier.
//   edge       the last strip of a strip row hangs over the right image edge; its dY beyond W is zero-filled, so dM = A 0 A^T = 0
//              there.  MFMA k-step kk multiplies the pixel columns x0 + 4 kk .. + 3: a strip runs kend = min(8, ceil((W - x0) / 4))
//              k-steps (wave-uniform; a k-step is left out only when ALL four of its columns are >= W).  Accumulators start at
//              +0 and a left-out k-step would have added va * (+-0) = +-0, which leaves every bit of a round-to-nearest sum as
//              it is: slabs and gradients are bit-identical to running all 8 -- for FINITE activations.  A non-finite x in the
//              halo column right of the edge-most valid one (Inf * 0) gave NaN when all 8 ran and does not now.
//              Option wgrad_skip_edge = 0 (api.cpp) sets the bound to the strips' own width: 8 k-steps everywhere.
struct WinoWgradArgs {
  const float* x; int x_cs, x_coff, x_cvalid;
  const float* dy; int dy_cs, dy_coff, dy_cvalid;
  float* ws;                    // [splits][16][Cr][Nr]
  int N, H, W, Cr, Nr, cblk;
  int strips_x, strips_y, total, per_split;
  int ntile, items, per_xcd;    // (c, n) tiles per split; work items; items per XCD band
  int kw;                       // image columns that bound a strip's k-steps: W (option wgrad_skip_edge) or strips_x * 32 (all 8)
};

#define WG_XROW 36               // staged halo pixels per row (34 used)
#define WG_X_BYTES (4 * WG_XROW * 256)
#define WG_Y_BYTES (2 * 32 * 256)
#define WG_STAGE_BYTES (WG_X_BYTES + WG_Y_BYTES)

__global__ __launch_bounds__(512, 2) void conv_wino_wgrad_kernel(WinoWgradArgs a) {
  __shared__ __attribute__((aligned(1024))) unsigned char smem[2 * WG_STAGE_BYTES];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lh = lane >> 5;
  const int fa = wave >> 1, fb = wave & 1;
  // XCD-aware order (round 3): workgroup id mod 8 labels the XCD (round-robin dispatch; speed only); XCD x owns the items
  // [x * per_xcd, (x+1) * per_xcd), an item = (pixel split, (c, n) tile) with the TILE fastest: the cblk x nblk tiles that read the
  // same pixel strips run back to back on ONE XCD and share its L2.  (Before: grid (splits, tiles) -- the tiles of a split were
  // `splits` workgroups apart in dispatch order and re-read x and dy from beyond L2: 515 MB read per launch against ~300 MB.)
  const int item = (int)(blockIdx.x & 7) * a.per_xcd + (int)(blockIdx.x >> 3);
  if (item >= a.items) return;
  const int split = item / a.ntile, tile = item - split * a.ntile;
  const int cb = tile % a.cblk, nbk = tile / a.cblk;
  const int c_blk = cb * 64, n_blk = nbk * 64;
  const int u0 = split * a.per_split, u1 = min(a.total, u0 + a.per_split);

  // input-transform roles (as the forward kernel): V row fa = s1 (d[r1] + s1 s2 d[r2]) with r1 = 0 1 1 1, r2 = 2 2 2 3, s1 = + + - +,
  // s2 = - + + -, columns fb .. fb + 2.  Rows and s1 s2 are compile-time in K_STEP; s1 is applied when the slab is written.
  const float s1 = (fa == 2) ? -1.f : 1.f;

  f32x16 acc[2][2][2];                              // [frequency e][cin tile ct][cout tile nt]
#pragma unroll
  for (int e = 0; e < 2; ++e)
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[e][ct][nt][r] = 0.f;

  // DMA pieces of a stage: x rows 4 x 9 pieces (4 pixels x 256 B each), dy 2 x 8 pieces; piece p of this wave = p*8 + wave.
  // buffer_load ... lds: the descriptor base is the unit's first (halo) pixel -- a wave-uniform pointer that may lie before the
  // tensor for border units --, the piece's row / pixel-group offset goes in as the scalar offset, and the lane part is ONE
  // per-lane constant; lanes outside the image, beyond the valid channels or in the unused tail of a staged row get an
  // out-of-range offset, which the hardware range check turns into zeros in LDS (tools/lds_dma_oob.hip).
  // NOTHING of that is worked out per unit (before: ~150 scalar and ~45 vector instructions and 7 s_nop 4 per wave between a
  // unit's barrier and its first MFMA, with all eight waves of the CU -- one workgroup, no partner -- issuing at once and every
  // matrix pipe idle meanwhile; profiles/wgrad_units_isa_census.json):
  //   piece      wave, piece index, row, pixel group, LDS destination: compile-time per wave variant; the scalar offset
  //              (row * W + pixel group) * cs * 4: one SGPR per piece, set before the unit loop
  //   lanes      one offset register per piece and strip-COLUMN CLASS -- first (pixel -1 is left of the image), middle (every
  //              pixel of the strip and its halo is inside), last (hangs over the right edge; with one strip per row it is also
  //              the first and its offsets say so) -- with channel validity and the tail of a staged row folded in; a unit
  //              picks the class by a wave-uniform branch, no lane compares
  //   rows       a row above or below the image (or the second dY row of an odd H) is wave-uniform: its pieces go through a
  //              descriptor of ZERO records, so every lane is out of range whatever its offset
  //   pointers   the two base pointers are carried from unit to unit by one of three constant steps (next strip, next strip
  //              row, next image); what describes a unit (class, record counts, pointers, k-steps) is prepared one unit ahead
  //   issue      the pieces of unit u + 1 go into the gaps between the 8 MFMAs of unit u's FIRST k-step (peeled out of the
  //              runtime-trip loop: every unit has one); its buffer is free from the barrier at the top of unit u on
    constexpr int NPX = 4 * (WG_XROW / 4), NPY = 2 * 8, NPW = (NPX + NPY + 7) / 8;
  constexpr unsigned OOB = 0xFFFFFFF0u;
  constexpr int NREC = 0x7FFFFF00;
  const int l4 = lane >> 4;                          // pixel of the piece's group of four
  const unsigned xlane = (c_blk + (lane & 15) * 4 < a.x_cvalid) ? (unsigned)(l4 * a.x_cs * 4 + (lane & 15) * 16) : OOB;
  const unsigned ylane = (n_blk + (lane & 15) * 4 < a.dy_cvalid) ? (unsigned)(l4 * a.dy_cs * 4 + (lane & 15) * 16) : OOB;
  const unsigned xfirst = l4 >= 1 ? xlane : OOB;     // first column class, pixel group 0: pixel -1
  const unsigned xtail = l4 < 2 ? xlane : OOB;       // pixel group 32: halo pixels 32, 33 of the 36 staged
  const int sxl = a.strips_x - 1, syl = a.strips_y - 1, x0l = sxl * 32;
  const int kend_last = min(8, (a.kw - x0l + 3) >> 2);          // k-steps of the last strip of a strip row (wave-uniform)
  // units are loaded in order, u0, u0 + 1, ...: the (strip column, strip row) of the next one and its two base pointers are
  // carried along and wrapped, not divided or multiplied out of the unit index every time
  int ld_sx = u0 % a.strips_x, ld_sy = (u0 / a.strips_x) % a.strips_y;
  const char *ld_x, *ld_y;
  {
    const int img_ = u0 / (a.strips_x * a.strips_y), y0_ = ld_sy * 2, x0_ = ld_sx * 32;
    ld_x = (const char*)(a.x + ((long long)(img_ * a.H + y0_ - 1) * a.W + x0_ - 1) * a.x_cs + a.x_coff + c_blk);
    ld_y = (const char*)(a.dy + ((long long)(img_ * a.H + y0_) * a.W + x0_) * a.dy_cs + a.dy_coff + n_blk);
  }
  // pixels from a unit's first pixel to the next unit's: next strip | next strip row | first strip row of the next image
  const int px_row = 2 * a.W - x0l, px_img = (a.H - 2 * syl) * a.W - x0l;
  const int xd_step = 32 * a.x_cs * 4, xd_row = px_row * a.x_cs * 4, xd_img = px_img * a.x_cs * 4;
  const int yd_step = 32 * a.dy_cs * 4, yd_row = px_row * a.dy_cs * 4, yd_img = px_img * a.dy_cs * 4;
  // the unit that is loaded next, prepared one unit ahead (WG_PREPARE): column class 0 first | 1 middle | 2 last, the records of
  // the descriptors of halo row 0, of halo row 3, and of halo row 2 = dY row 1, base pointers, k-steps
  int pr_cls, pr_top, pr_bot, pr_bot1, pr_kend;
  const char *pr_x, *pr_y;
#define WG_PREPARE                                                                                                     \
  {                                                                                                                    \
    const bool lastx_ = ld_sx == sxl, lasty_ = ld_sy == syl;                                                           \
    pr_cls = lastx_ ? 2 : min(ld_sx, 1);       /* (min: a select of a compare went through a vector register) */      \
    pr_kend = lastx_ ? kend_last : 8;                                                                                  \
    pr_top = ld_sy == 0 ? 0 : NREC;                                                                                    \
    pr_bot = lasty_ ? 0 : NREC;                                                                                        \
    pr_bot1 = (lasty_ && (a.H & 1)) ? 0 : NREC;                                                                        \
    pr_x = ld_x; pr_y = ld_y;                                                                                          \
    const int xd_ = lastx_ ? (lasty_ ? xd_img : xd_row) : xd_step, yd_ = lastx_ ? (lasty_ ? yd_img : yd_row) : yd_step; \
    ld_x += xd_; ld_y += yd_;                                                                                          \
    ld_sx = lastx_ ? 0 : ld_sx + 1;                                                                                    \
    ld_sy = lastx_ ? (lasty_ ? 0 : ld_sy + 1) : ld_sy;                                                                 \
  }
// piece p_ of wave variant WV_ of the prepared unit, column class CLS_ (both compile-time), into stage buffer lb_
#define WG_PIECE(p_, CLS_)                                                                                             \
  if ((p_) * 8 + WV_ < NPX + NPY) {                                                                                    \
    constexpr int piece_ = (p_) * 8 + WV_;                                                                             \
    constexpr bool isx_ = piece_ < NPX;                                                                                \
    constexpr int row_ = isx_ ? piece_ / (WG_XROW / 4) : (piece_ - NPX) >> 3;                                          \
    constexpr int pxb_ = isx_ ? (piece_ % (WG_XROW / 4)) * 4 : ((piece_ - NPX) & 7) * 4;                               \
    const unsigned vo_ = (CLS_) == 2 ? vlast[p_] : !isx_ ? ylane : pxb_ == 32 ? xtail : ((CLS_) == 0 && pxb_ == 0) ? xfirst : xlane; \
    const int nrec_ = isx_ ? (row_ == 0 ? pr_top : row_ == 2 ? pr_bot1 : row_ == 3 ? pr_bot : NREC) : (row_ == 1 ? pr_bot1 : NREC); \
    HPRI_LDS_DMA16(HPRI_MAKE_RSRC(isx_ ? pr_x : pr_y, nrec_), lb_ + piece_ * 1024, vo_, soff[p_]);                     \
  }
// the per-(wave, piece) constants: scalar offsets, and the lane offsets of the last column class (x0 = x0l; with one strip per
// row the strip is also the first: the unsigned compare covers pixel -1)
#define WG_PIECE_SETUP                                                                                                 \
  int soff[NPW]; unsigned vlast[NPW];                                                                                  \
  _Pragma("unroll") for (int p = 0; p < NPW; ++p) {                                                                    \
    const int piece_ = p * 8 + WV_;                                                                                    \
    soff[p] = 0; vlast[p] = OOB;                                                                                       \
    if (piece_ < NPX) {                                                                                                \
      const int row_ = piece_ / (WG_XROW / 4), pxb_ = (piece_ % (WG_XROW / 4)) * 4;                                    \
      soff[p] = (row_ * a.W + pxb_) * a.x_cs * 4;                                                                      \
      vlast[p] = ((pxb_ + l4) < 34 && (unsigned)(x0l + pxb_ + l4 - 1) < (unsigned)a.W) ? xlane : OOB;                  \
    } else if (piece_ < NPX + NPY) {                                                                                   \
      const int row_ = (piece_ - NPX) >> 3, pxb_ = ((piece_ - NPX) & 7) * 4;                                           \
      soff[p] = (row_ * a.W + pxb_) * a.dy_cs * 4;                                                                     \
      vlast[p] = (x0l + pxb_ + l4) < a.W ? ylane : OOB;                                                                \
    }                                                                                                                  \
  }

// The loop body is compiled per (frequency row, column pair): the row part of dM = A dY A^T multiplies by constants that are
// 0 or +-1 -- a = 0: dY[0], a = 1: dY[0] + dY[1], a = 2: dY[0] - dY[1], a = 3: -dY[1] -- so rows 0 and 3 need no arithmetic at
// all and rows 1, 2 one add per column; the column part for b = 2 fb + e is t0 | t0 + t1 (fb = 0), t0 - t1 | -t1 (fb = 1).  The
// two minus signs (row 3, and b = 3) are left out here and applied once to the accumulators when the slab is written.
// ONE loop with the unit's trip count kend (odd at W = 121 and W = 60: exact, no remainder step), not unrolled.  A second copy of
// the loop for short strips (constant-trip loop for kend = 8, runtime loop otherwise) inside the unit loop spills 2044 registers,
// with or without an opaque lane id: rejected.  Two k-steps per trip plus a straight-line odd step measured no faster than
// running all 8 (experiments/README.md).
// Every vector or LDS instruction of the k-step is paid in matrix-pipe time, so the step holds the transform and
// nothing else: 13 (rows 0, 3) or 17 (rows 1, 2) vector and 8 or 10 LDS instructions per 8 MFMAs
// (profiles/wgrad_kstep_isa_census.json; before: 19-29 and 8-10); the kernel takes 164 registers (185 before the k-step was cut down).
//   operands   lane li holds input channels 2 li, 2 li + 1 (its cin tiles ct = 0, 1) and output channels 2 li, 2 li + 1 (its cout
//              tiles nt = 0, 1): both tiles' operands of a pixel are ONE ds_read_b64 (conflict-free: 32 lanes x 8 bytes are the
//              pixel's 256 bytes).  Which channel sits in which MFMA row or column changes no sum; the slab write puts them back.
//   address    ONE register, kp = stage + lh * 512 + li * 8, + 1024 per k-step; rows, columns and the dY block are immediates
//              (the stage is 52 KB, a ds_read offset reaches 64 KB).  The reads are volatile so that hipcc leaves them single:
//              merged into ds_read2_b64 pairs each pair got a base register of its own and an add per k-step (3-6 adds).
//   transform  scalar adds and subtracts; WG_PIN (an empty asm on the value) keeps hipcc's SLP vectoriser from pairing them into
//              v_pk_add_f32 / v_pk_fma_f32, which cost more per flop and took 6-12 v_mov_b32 to pack their operands.  The row
//              signs s1 s2 are compile-time per variant: d1 + s1 s2 d2 is one add or one subtract, the same bits as the FMA.
//   schedule   sched_barrier: operands first, then the 8 MFMAs back to back (left alone hipcc spread the transform between the
//              MFMAs and re-used operand registers: 7-8 s_nop per k-step).
#define K_STEP(FA_, FB_, GAP_, END_)        /* MFMA k-step kk: tiles 2 kk + lh of the strip; what goes between its MFMAs */ \
    {                                                                                                                  \
      constexpr int R1_ = (FA_ == 0) ? 0 : 1, R2_ = (FA_ == 3) ? 3 : 2;             /* halo rows of the row transform */ \
      constexpr int YR_ = (FA_ == 3) ? 1 : 0, YROWS_ = (FA_ == 1 || FA_ == 2) ? 2 : 1;                                 \
      asm("" : "+v"(kp));                           /* the ONE address register; everything else is an immediate */    \
      f32x2 d[2][3], y[2][2];                       /* x [row r1 | r2][column c], dY [row][pixel] */                   \
      _Pragma("unroll") for (int c = 0; c < 3; ++c) {                                                                  \
        d[0][c] = WG_LDS2(kp + (R1_ * WG_XROW + FB_ + c) * 256);                                                       \
        d[1][c] = WG_LDS2(kp + (R2_ * WG_XROW + FB_ + c) * 256);                                                       \
      }                                                                                                                \
      _Pragma("unroll") for (int r = 0; r < YROWS_; ++r)                                                               \
        _Pragma("unroll") for (int px = 0; px < 2; ++px) y[r][px] = WG_LDS2(kp + WG_X_BYTES + ((YR_ + r) * 32 + px) * 256); \
      float va[2][2], vb[2][2];                     /* [frequency e][cin tile | cout tile] */                          \
      float P[3][2];                                                                                                   \
      _Pragma("unroll") for (int c = 0; c < 3; ++c)                                                                    \
        _Pragma("unroll") for (int ct = 0; ct < 2; ++ct) {                                                             \
          float d1_ = d[0][c][ct], d2_ = d[1][c][ct];                                                                  \
          WG_PIN(d1_) WG_PIN(d2_)                                                                                      \
          P[c][ct] = (FA_ == 1) ? (d1_ + d2_) : (d1_ - d2_);            /* d1 + s1 s2 d2 */                            \
          WG_PIN(P[c][ct])                                                                                             \
        }                                                                                                              \
      _Pragma("unroll") for (int ct = 0; ct < 2; ++ct) {                                                               \
        va[0][ct] = FB_ ? (P[1][ct] - P[0][ct]) : (P[0][ct] - P[2][ct]);                                               \
        va[1][ct] = FB_ ? (P[0][ct] - P[2][ct]) : (P[1][ct] + P[2][ct]);                                               \
                                                                                                                       \
      }                                                                                                                \
      float t[2][2];                                /* [pixel of the tile][cout tile] */                               \
      _Pragma("unroll") for (int px = 0; px < 2; ++px)                                                                 \
        _Pragma("unroll") for (int nt = 0; nt < 2; ++nt) {                                                             \
          float y0_ = y[0][px][nt];                                                                                    \
          WG_PIN(y0_)                                                                                                  \
          if (YROWS_ == 2) {                                                                                           \
            float y1_ = y[1][px][nt];                                                                                  \
            WG_PIN(y1_)                                                                                                \
            y0_ = (FA_ == 1) ? (y0_ + y1_) : (y0_ - y1_);                                                              \
            WG_PIN(y0_)                                                                                                \
          }                                                                                                            \
          t[px][nt] = y0_;                                                                                             \
        }                                                                                                              \
      _Pragma("unroll") for (int nt = 0; nt < 2; ++nt) {                                                               \
        vb[0][nt] = FB_ ? (t[0][nt] - t[1][nt]) : t[0][nt];                                                            \
        vb[1][nt] = FB_ ? t[1][nt] : (t[0][nt] + t[1][nt]);                                                            \
                                                                                                                       \
      }                                                                                                                \
      /* (volatile pins: the branches in the gaps of a unit's first k-step end the basic block, and hipcc sinks */     \
      /* an operand's last subtract to its first use between the MFMAs otherwise, with an s_nop 1 each) */             \
      _Pragma("unroll") for (int e = 0; e < 2; ++e)                                                                    \
        _Pragma("unroll") for (int q = 0; q < 2; ++q) { asm volatile("" : "+v"(va[e][q])); asm volatile("" : "+v"(vb[e][q])); } \
      __builtin_amdgcn_sched_barrier(0);            /* operands first, then the 8 MFMAs back to back */                \
      WG_MFMA(0, 0, 0) GAP_(0) WG_MFMA(0, 0, 1) GAP_(1) WG_MFMA(0, 1, 0) GAP_(2) WG_MFMA(0, 1, 1) GAP_(3)              \
      WG_MFMA(1, 0, 0) GAP_(4) WG_MFMA(1, 0, 1) GAP_(5) WG_MFMA(1, 1, 0) GAP_(6) WG_MFMA(1, 1, 1) END_                 \
      kp += 1024;                                   /* four pixel columns on */                                        \
    }
#define WG_MFMA(e_, ct_, nt_) \
  acc[e_][ct_][nt_] = __builtin_amdgcn_mfma_f32_32x32x2f32(va[e_][ct_], vb[e_][nt_], acc[e_][ct_][nt_], 0, 0, 0);
  // the gaps of a unit's first k-step: piece i of the next unit behind MFMA i (6 or 7 pieces for 7 gaps), and behind the last
  // MFMA the scalar work that describes the unit after that; sched_barrier keeps each where it stands
#define WG_NOGAP(i_)
#define WG_GAP(i_) __builtin_amdgcn_sched_barrier(0); WG_PIECE_IN_LOOP(i_) __builtin_amdgcn_sched_barrier(0);
#define WG_END __builtin_amdgcn_sched_barrier(0); kend_next = pr_kend; WG_PREPARE
  // the variant is chosen once per wave, outside the unit loop (eight copies of the loop, no selects inside); so are a wave's
  // pieces.  A unit that has a successor runs its first k-step in the copy that issues the successor's pieces, the rest in the
  // loop.  (One copy of that k-step per column class, each with its own MFMAs, spilled 252 bytes: the class branches lie in the gaps.)
#define UNIT_LOOP(FA_, FB_)                                                                                            \
  {                                                                                                                    \
    constexpr int WV_ = 2 * FA_ + FB_;                                                                                 \
    WG_PIECE_SETUP                                                                                                     \
    if (u0 < u1) {                                                                                                     \
      unsigned char* lb_ = smem;                                                                                       \
      WG_PREPARE                                                                                                       \
      kend_next = pr_kend;                                                                                             \
      WG_PIECE_ANY(0) WG_PIECE_ANY(1) WG_PIECE_ANY(2) WG_PIECE_ANY(3) WG_PIECE_ANY(4) WG_PIECE_ANY(5) WG_PIECE_ANY(6)  \
      WG_PREPARE                                                                                                       \
    }                                                                                                                  \
    for (int u = u0; u < u1; ++u) {                                                                                    \
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                                 \
      __builtin_amdgcn_s_barrier();        /* this unit has landed for everyone; the other buffer is free */           \
      const int kend = kend_next;                                                                                      \
      unsigned kp = WG_BUF_OF(u - u0) * WG_STAGE_BYTES + klane;                                                        \
      int kk = 0;                                                                                                      \
      if (u + 1 < u1) {                                                                                                \
        unsigned char* lb_ = smem + ((u + 1 - u0) & 1) * WG_STAGE_BYTES;                                               \
        K_STEP(FA_, FB_, WG_GAP, WG_END)                                                                               \
        kk = 1;                                                                                                        \
      }                                                                                                                \
      for (; kk < kend; ++kk) K_STEP(FA_, FB_, WG_NOGAP, )                                                             \
    }                                                                                                                  \
  }
// ... of the prepared unit's column class: a wave-uniform branch around the copies that differ (the first class differs from
// the middle one in the pieces of pixel group 0 only).  The asm comments make the arms differ behind the load: hipcc otherwise
// sinks the load below the branch and selects its lane offset per lane (v_cndmask) on a class it keeps in a vector register
#define WG_PIECE_ANY(p_)                                                                                               \
  if (pr_cls == 2) { WG_PIECE(p_, 2) asm volatile("; last column class"); }                                            \
  else if (pr_cls == 0 && (p_) * 8 + WV_ < NPX && ((p_) * 8 + WV_) % (WG_XROW / 4) == 0) {                             \
    WG_PIECE(p_, 0) asm volatile("; first column class");                                                              \
  } else { WG_PIECE(p_, 1) asm volatile("; middle column class"); }
  const unsigned klane = (unsigned)(lh * 512 + li * 8);
  typedef __attribute__((address_space(3))) const unsigned char* wg_lds_bytes;
  typedef __attribute__((address_space(3))) const volatile f32x2* wg_lds_f32x2;
  const wg_lds_bytes lds = (wg_lds_bytes)smem;
#define WG_LDS2(off_) (*(wg_lds_f32x2)(lds + (off_)))
#define WG_PIN(v_) asm("" : "+v"(v_));
  int kend_next = 8;
#ifdef WGRAD_DIAG_NO_UNIT_LOAD
  // timing-only build (tools/build_wgrad_diag.sh): the unit loop issues no loads, every unit multiplies the first unit's data;
  // results are meaningless, the time is what is left when loading the next unit costs nothing
#define WG_PIECE_IN_LOOP(i_)
#define WG_BUF_OF(i_) 0
#else
#define WG_PIECE_IN_LOOP(i_) WG_PIECE_ANY(i_)
#define WG_BUF_OF(i_) ((i_) & 1)
#endif
  switch (wave) {                          // wave = 2 fa + fb
    case 0: UNIT_LOOP(0, 0) break;
    case 1: UNIT_LOOP(0, 1) break;
    case 2: UNIT_LOOP(1, 0) break;
    case 3: UNIT_LOOP(1, 1) break;
    case 4: UNIT_LOOP(2, 0) break;
    case 5: UNIT_LOOP(2, 1) break;
    case 6: UNIT_LOOP(3, 0) break;
    default: UNIT_LOOP(3, 1) break;
  }
#undef UNIT_LOOP
#undef K_STEP
#undef WG_MFMA
#undef WG_NOGAP
#undef WG_GAP
#undef WG_END
#undef WG_PIECE_ANY
#undef WG_PIECE_IN_LOOP
#undef WG_PIECE
#undef WG_PIECE_SETUP
#undef WG_PREPARE
#undef WG_BUF_OF
#undef WG_LDS2
#undef WG_PIN
  // slab: ws[split][xi][c][n]; accumulator rows = cin (register index), columns = cout (lane)
  float* slab = a.ws + (size_t)split * 16 * a.Cr * a.Nr;
  const float sdy = (fa == 3) ? -s1 : s1;                              // input-transform row sign x dY row sign
  const float sgn[2] = {sdy, (fb == 1) ? -sdy : sdy};                  // ... x the sign of column frequency b = 3
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int xi = fa * 4 + 2 * fb + e;
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int c = c_blk + 2 * ((r & 3) + 8 * (r >> 2) + 4 * lh) + ct;
        f32x2 o;                                                            // cout 2 li (nt = 0) and 2 li + 1 (nt = 1)
        o[0] = sgn[e] * acc[e][ct][0][r];                                   // the transform signs left out of the loop
        o[1] = sgn[e] * acc[e][ct][1][r];
        *reinterpret_cast<f32x2*>(&slab[((size_t)xi * a.Cr + c) * a.Nr + n_blk + 2 * li]) = o;
      }
  }
}

// dW[n][c][3][3] (+)= G^T (sum over splits of dU[.][c][n]) G, fixed summation order.  One thread per (c, n).
__global__ void wino_wgrad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dw, int splits, int Cr, int Nr,
                                         int Cin, int Cout, int accumulate) {
  const int n = blockIdx.x * 64 + (threadIdx.x & 63), c = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (n >= Cout || c >= Cin) return;
  float u[16];
#pragma unroll
  for (int xi = 0; xi < 16; ++xi) u[xi] = 0.f;
  const size_t slab = (size_t)16 * Cr * Nr;
  for (int k = 0; k < splits; ++k) {
    const float* p = ws + (size_t)k * slab + (size_t)c * Nr + n;
#pragma unroll
    for (int xi = 0; xi < 16; ++xi) u[xi] += p[(size_t)xi * Cr * Nr];
  }
  // t = G^T u (3x4 . 4x4), G^T = [1 .5 .5 0; 0 .5 -.5 0; 0 .5 .5 1]
  float t[3][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    t[0][j] = u[0 * 4 + j] + 0.5f * (u[1 * 4 + j] + u[2 * 4 + j]);
    t[1][j] = 0.5f * (u[1 * 4 + j] - u[2 * 4 + j]);
    t[2][j] = 0.5f * (u[1 * 4 + j] + u[2 * 4 + j]) + u[3 * 4 + j];
  }
  float* o = dw + ((size_t)n * Cin + c) * 9;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float g0 = t[i][0] + 0.5f * (t[i][1] + t[i][2]), g1 = 0.5f * (t[i][1] - t[i][2]), g2 = 0.5f * (t[i][1] + t[i][2]) + t[i][3];
    o[i * 3 + 0] = accumulate ? o[i * 3 + 0] + g0 : g0;
    o[i * 3 + 1] = accumulate ? o[i * 3 + 1] + g1 : g1;
    o[i * 3 + 2] = accumulate ? o[i * 3 + 2] + g2 : g2;
  }
}

// The same for MANY slabs (the 608 x 968 layers: 256 slabs of 16 x 64 x 64, 67 MB, which the kernel above reads with 16
// workgroups): S slab slices x NC columns per workgroup and ONE input channel; slice s sums slabs s, s + S, ... in order, the
// slices meet in LDS in order (deterministic).
// Co-residency: the S = 16 form runs on the side stream while conv_wino4_kernel (two workgroups per CU, one wave of 248
// registers per SIMD and 78 KB of LDS each) fills the machine on the main stream.  With NC = 32 columns it is a 512-thread
// workgroup: two waves per SIMD (144 registers) and 30 KB of LDS, which fits on a CU as soon as ONE of the two data-gradient
// workgroups has left it (264 registers per SIMD and 82 KB free).  As 1024 threads x 64 columns (288 registers per SIMD, 60 KB)
// it had to wait for both to leave at the same moment.  (A cap of 64 registers per wave on the 1024-thread form spills.)
// The column count changes which workgroup holds a column, not the order in which its slabs are added.
constexpr int wino_wide_cols(int S) { return S >= 16 ? 32 : 64; }   // workgroup = S slices x this many columns: 512 threads for S = 8, 16

template <int S>
__global__ __launch_bounds__(wino_wide_cols(S) * S) void wino_wgrad_reduce_wide_kernel(const float* __restrict__ ws,
                                                                                       float* __restrict__ dw, int splits, int Cr,
                                                                                       int Nr, int Cin, int Cout, int accumulate) {
  constexpr int NC = wino_wide_cols(S);
  __shared__ float red[S - 1][16][NC];
  const int ln = threadIdx.x % NC, sl = threadIdx.x / NC;
  const int n = blockIdx.x * NC + ln, c = blockIdx.y;            // n < Nr (a multiple of 64), c < Cin <= Cr
  float u[16];
#pragma unroll
  for (int xi = 0; xi < 16; ++xi) u[xi] = 0.f;
  const size_t slab = (size_t)16 * Cr * Nr;
  // (one slab = 16 independent loads in flight per thread, 16 k per workgroup; unrolled by hipcc, the S = 16 form -- 1024
  // threads, 128 registers -- spilled 50 of them)
#pragma unroll 1
  for (int k = sl; k < splits; k += S) {
    const float* p = ws + (size_t)k * slab + (size_t)c * Nr + n;
#pragma unroll
    for (int xi = 0; xi < 16; ++xi) u[xi] += p[(size_t)xi * Cr * Nr];
  }
  if (sl > 0) {
#pragma unroll
    for (int xi = 0; xi < 16; ++xi) red[sl - 1][xi][ln] = u[xi];
  }
  __syncthreads();
  if (sl > 0 || n >= Cout) return;
#pragma unroll 2
  for (int q = 0; q < S - 1; ++q)
#pragma unroll
    for (int xi = 0; xi < 16; ++xi) u[xi] += red[q][xi][ln];
  float t[3][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    t[0][j] = u[0 * 4 + j] + 0.5f * (u[1 * 4 + j] + u[2 * 4 + j]);
    t[1][j] = 0.5f * (u[1 * 4 + j] - u[2 * 4 + j]);
    t[2][j] = 0.5f * (u[1 * 4 + j] + u[2 * 4 + j]) + u[3 * 4 + j];
  }
  float* o = dw + ((size_t)n * Cin + c) * 9;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float g0 = t[i][0] + 0.5f * (t[i][1] + t[i][2]), g1 = 0.5f * (t[i][1] - t[i][2]), g2 = 0.5f * (t[i][1] + t[i][2]) + t[i][3];
    o[i * 3 + 0] = accumulate ? o[i * 3 + 0] + g0 : g0;
    o[i * 3 + 1] = accumulate ? o[i * 3 + 1] + g1 : g1;
    o[i * 3 + 2] = accumulate ? o[i * 3 + 2] + g2 : g2;
  }
}

extern "C" int hpri_wino_wgrad_plan(int N, int H, int W, int Cin_pad, int Cout_pad, int* splits, int* Cr, int* Nr) {
  const int cblk = hpri_cdiv(Cin_pad, 64), nblk = hpri_cdiv(Cout_pad, 64);
  const int total = N * hpri_cdiv(H, 2) * hpri_cdiv(W, 32);
  *Cr = cblk * 64; *Nr = nblk * 64;
  const int tiles = cblk * nblk;
  // one workgroup per CU: splits such that tiles * splits is close to a multiple of 256, with >= 8 strips per split
  auto plan = [&](int cus, int kmax, double tol) {
    int best = 1; double best_eff = 0.0;
    for (int k = 1; k <= kmax; ++k) {
      if (k > 1 && total / k < 8) break;
      const double per_cu = (double)tiles * k / (double)cus;
      double eff = per_cu / (double)((long long)(per_cu + 0.999999));
      if (per_cu < 1.0) eff = per_cu;
      if (eff > best_eff + tol + 1e-9) { best_eff = eff; best = k; }
    }
    return best;
  };
  int best = plan(256, 512, 0.0);
  // option wgrad_cu_reserve (api.cpp): plan for that many fewer CUs, so that a few CUs held by another kernel do not push the last
  // workgroups into a second wave -- with at most twice the slabs of the plain plan, and a smaller split preferred unless a larger
  // one fills the CUs at least 5 % better
  const int reserve = hpri_option(5);
  if (reserve > 0) best = plan(256 - (reserve < 192 ? reserve : 192), 2 * best, 0.05);
  *splits = best;
  return HPRI_OK;
}

// Weight gradient of a 3x3 / pad 1 convolution by Winograd: slabs in ws (splits*16*Cr*Nr floats, hpri_wino_wgrad_plan),
// then hpri_wino_wgrad_reduce into dW (OIHW).
extern "C" int hpri_conv_wino_wgrad(const float* x, int x_cs, int x_coff, int x_cvalid, const float* dy, int dy_cs, int dy_coff,
                                    int dy_cvalid, float* ws, size_t ws_floats, int N, int H, int W, int Cin_pad, int Cout_pad,
                                    hipStream_t stream) {
  HPRI_REQUIRE(x && dy && ws, "conv_wino_wgrad: null pointer");
  HPRI_REQUIRE(N > 0 && H > 0 && W > 0 && Cin_pad > 0 && Cout_pad > 0, "conv_wino_wgrad: bad sizes");
  HPRI_REQUIRE(x_cs % 4 == 0 && x_coff % 4 == 0 && dy_cs % 4 == 0 && dy_coff % 4 == 0 && x_cvalid % 4 == 0 && dy_cvalid % 4 == 0,
               "conv_wino_wgrad: channel strides / offsets / valid counts must be multiples of 4");
  HPRI_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)dy & 15) == 0, "conv_wino_wgrad: pointers must be 16-byte aligned");
  HPRI_REQUIRE((long long)5 * W * x_cs * 4 < (1ll << 31) && (long long)3 * W * dy_cs * 4 < (1ll << 31),
               "conv_wino_wgrad: image rows too long for 32-bit buffer offsets");
  WinoWgradArgs a;
  a.x = x; a.x_cs = x_cs; a.x_coff = x_coff; a.x_cvalid = x_cvalid; a.dy = dy; a.dy_cs = dy_cs; a.dy_coff = dy_coff; a.dy_cvalid = dy_cvalid;
  a.ws = ws; a.N = N; a.H = H; a.W = W;
  int splits;
  hpri_wino_wgrad_plan(N, H, W, Cin_pad, Cout_pad, &splits, &a.Cr, &a.Nr);
  if ((size_t)splits * 16 * a.Cr * a.Nr > ws_floats) return hpri_set_error(HPRI_ERR_WORKSPACE, "conv_wino_wgrad: workspace too small");
  a.cblk = a.Cr / 64;
  a.strips_x = hpri_cdiv(W, 32); a.strips_y = hpri_cdiv(H, 2); a.total = N * a.strips_x * a.strips_y;
  a.per_split = hpri_cdiv(a.total, splits);
  a.ntile = a.cblk * (a.Nr / 64);
  a.items = splits * a.ntile; a.per_xcd = hpri_cdiv(a.items, 8);
  a.kw = hpri_option(6) != 0 ? W : a.strips_x * 32;           // wgrad_skip_edge: no MFMAs for pixel columns right of the image
  dim3 grid((unsigned)(a.per_xcd * 8), 1u, 1u);
  hipLaunchKernelGGL(conv_wino_wgrad_kernel, grid, dim3(512), 0, stream, a);
  HPRI_CHECK_LAUNCH();
  return HPRI_OK;
}

extern "C" int hpri_wino_wgrad_reduce(const float* ws, float* dw, int N, int H, int W, int Cin, int Cin_pad, int Cout, int Cout_pad,
                                      int accumulate, hipStream_t stream) {
  HPRI_REQUIRE(ws && dw && Cin > 0 && Cout > 0, "wino_wgrad_reduce: bad arguments");
  int splits, Cr, Nr;
  hpri_wino_wgrad_plan(N, H, W, Cin_pad, Cout_pad, &splits, &Cr, &Nr);
  if (splits >= 64) {                               // many slabs, few (c, n) pairs: spread the slabs over the workgroup too
    dim3 grid((unsigned)hpri_cdiv(Cout, wino_wide_cols(16)), (unsigned)Cin);
    hipLaunchKernelGGL(wino_wgrad_reduce_wide_kernel<16>, grid, dim3(wino_wide_cols(16) * 16), 0, stream, ws, dw, splits, Cr, Nr, Cin, Cout, accumulate);
  } else if (splits >= 8) {
    dim3 grid((unsigned)hpri_cdiv(Cout, 64), (unsigned)Cin);
    hipLaunchKernelGGL(wino_wgrad_reduce_wide_kernel<8>, grid, dim3(512), 0, stream, ws, dw, splits, Cr, Nr, Cin, Cout, accumulate);
  } else {
    dim3 grid((unsigned)hpri_cdiv(Cout, 64), (unsigned)hpri_cdiv(Cin, 4));
    hipLaunchKernelGGL(wino_wgrad_reduce_kernel, grid, dim3(256), 0, stream, ws, dw, splits, Cr, Nr, Cin, Cout, accumulate);
  }
  HPRI_CHECK_LAUNCH();
  return HPRI_OK;
}
