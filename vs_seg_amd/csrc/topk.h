// What the top-k cross-entropy term shares between its kernels (topk.hip: the radix select; loss.hip: the finalize and the backward): the device record, the value of a
// voxel and the key it is ranked by.  include/vsseg_hip.h states the definition.
#pragma once
#include "common.h"

// Radix digits, most significant first: 11 + 11 + 10 bits = three histogram passes (surface.hip's 4 x 8 cost one pass more over 25 M voxels).
constexpr int TOPK_PASSES = 3;
constexpr int TOPK_MAX_BINS = 2048;
__host__ __device__ constexpr int topk_shift(int pass) { return pass == 0 ? 21 : (pass == 1 ? 10 : 0); }
__host__ __device__ constexpr int topk_bins(int pass) { return pass == 2 ? 1024 : 2048; }
__host__ __device__ constexpr int topk_hist_at(int pass) { return pass == 0 ? 0 : (pass == 1 ? 2048 : 4096); }

// The record in the caller's scratch (vsseg_topk_scratch_bytes(), zeroed by the caller).  Its first 32 bytes are ABI (include/vsseg_hip.h); the rest is the state
// that goes from one kernel into the next: the host reads nothing between them.
struct TopkRec {
  unsigned threshold_bits;       //  0: key of the K-th largest element, complete after the last scan
  unsigned passes_done;          //  4: scans finished (3: the record is complete)
  unsigned long long n_gt;       //  8: elements with a key above the threshold
  unsigned long long n_eq;       // 16: elements with the threshold's key
  unsigned long long k;          // 24: K, as given
  unsigned long long rank;       // 32: 1-based rank of the K-th largest among the elements that share `prefix`
  unsigned prefix, pad;          // 40: the digits found so far
  double s_above;                // 48: fixed-point (VSSEG_FX_STAT) sum of the values whose first two digits are above the threshold's (last histogram pass)
  double s_tail;                 // 56: fp64 sum of the values that share the threshold's first two digits and lie above it: sum over bins of count * value (last scan)
  unsigned long long hist[2048 + 2048 + 1024];  // 64: one histogram per pass
};
static_assert(sizeof(TopkRec) == 64 + 5120 * 8, "TopkRec layout");

// Key of a value: the uint32 bit pattern of a non-negative float orders like the float.  -0 counts as 0; a NaN takes the largest key, so that it is always selected
// and poisons the sum.
__device__ __forceinline__ unsigned topk_key(float v) {
  const unsigned u = __float_as_uint(v);
  return v != v ? 0xFFFFFFFFu : (u == 0x80000000u ? 0u : u);
}

// v = w[y] * softplus(x[1-y] - x[y]): the value of a voxel in the top-k term, with ce_terms' (loss.hip) cast of the label and its softplus.  The three histogram passes
// (the last one sums as well) and the backward must get the SAME BITS, or a voxel is counted on one side of the threshold and treated on the other: the one definition
// is here and floating-point contraction is off inside it — inlined into different kernels, e * (1 - 0.5 e) could otherwise become an fma in one and not in another.
__device__ __forceinline__ float ce_topk_value(float l0, float l1, float lab, float wfg) {
#pragma clang fp contract(off)
  const bool fg = (int)(long long)lab == 1;
  const float z = fg ? l0 - l1 : l1 - l0;
  const float e = __expf(-fabsf(z));
  const float h = 0.5f * e;
  const float q = 1.f - h;
  const float sp = (z > 0.f ? z : 0.f) + (e < 0x1p-12f ? e * q : __logf(1.f + e));
  return fg ? wfg * sp : sp;
}
