// The binary decision of one pixel, as every kernel of the device tail takes it (components.hip, distance.hip).
#pragma once
#include "common.h"

struct CcDecision {
  const void* pred;
  int kind;                              // 0: fp32 with threshold, 1: uint8 (value != 0), 2: fp32 mask (((int)value) != 0)
  float threshold;
  int is_logits, invert;
};

#ifdef __HIPCC__
__device__ __forceinline__ int cc_decide(const CcDecision& d, int i) {
  int fg;
  if (d.kind == 0) {
    const float x = reinterpret_cast<const float*>(d.pred)[i];
    const float p = d.is_logits ? 1.f / (1.f + expf(-x)) : x;          // (= sigmoid_f32 of step.hip, segmap_class of segmap.hip)
    fg = p > d.threshold;
  } else if (d.kind == 1) {
    fg = reinterpret_cast<const unsigned char*>(d.pred)[i] != 0;
  } else {
    fg = ((int)reinterpret_cast<const float*>(d.pred)[i]) != 0;          // (how every kernel of the tail reads a mask)
  }
  return d.invert ? !fg : fg;
}
#endif
