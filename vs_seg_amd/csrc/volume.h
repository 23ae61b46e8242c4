// What the whole-volume analysis calls share (components.hip, surface.hip, measure.hip): the rule that turns logits and labels into masks, 64-lane integer
// reductions, the "count + bounding box" record that a pass leaves in device memory for the passes after it, and the argument checks of a launcher.
#pragma once
#include <limits.h>
#include "common.h"

// The masks of a two-class segmentation, wherever the library forms them: the prediction is the argmax of the two logits (ties and NaN are background, like
// torch.argmax), the label is foreground where its value truncates to 1.
__device__ __forceinline__ bool vsseg_pred_fg(float2 logits) { return logits.y > logits.x; }
__device__ __forceinline__ bool vsseg_label_fg(float label) { return ((int)(long long)label) == 1; }

template <typename T, typename F>
__device__ __forceinline__ T wave_reduce(T v, F f) {  // every lane of the 64 gets the result
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = f(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_min_i(int v) { return wave_reduce(v, [](int a, int b) { return min(a, b); }); }
__device__ __forceinline__ int wave_max_i(int v) { return wave_reduce(v, [](int a, int b) { return max(a, b); }); }
__device__ __forceinline__ unsigned wave_sum_u(unsigned v) { return wave_reduce(v, [](unsigned a, unsigned b) { return a + b; }); }
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) { return wave_reduce(v, [](unsigned long long a, unsigned long long b) { return a + b; }); }
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) { return wave_reduce(v, [](unsigned long long a, unsigned long long b) { return a > b ? a : b; }); }

// NC voxel counts and the bounding box, over AXES axes, of the voxels counted.  In device memory the record is NC 64-bit counts, bmin[AXES] and bmax[AXES], reset to
// 0, INT_MAX and -1 (an empty box); only integer atomics merge into it, so it does not depend on the order in which waves and workgroups finish.  A thread counts in
// n[] itself and grows the box by what it counted, so that all counts 0 <=> the box is empty.
template <int AXES, int NC = 1>
struct CountBox {
  unsigned n[NC];
  int lo[AXES], hi[AXES];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int c = 0; c < NC; ++c) n[c] = 0;
#pragma unroll
    for (int a = 0; a < AXES; ++a) lo[a] = INT_MAX, hi[a] = -1;
  }
  __device__ __forceinline__ void grow(const int (&l)[AXES], const int (&h)[AXES]) {  // by the box l .. h (a voxel: l = h)
#pragma unroll
    for (int a = 0; a < AXES; ++a) lo[a] = min(lo[a], l[a]), hi[a] = max(hi[a], h[a]);
  }
  __device__ __forceinline__ bool empty() const {
    unsigned any = 0;
#pragma unroll
    for (int c = 0; c < NC; ++c) any |= n[c];
    return !any;
  }
  __device__ __forceinline__ void wave_reduce() {  // every lane gets the record of the wave; the box of a wave that counted nothing is empty already
#pragma unroll
    for (int c = 0; c < NC; ++c) n[c] = wave_sum_u(n[c]);
    if (empty()) return;  // (the same in every lane)
#pragma unroll
    for (int a = 0; a < AXES; ++a) lo[a] = wave_min_i(lo[a]), hi[a] = wave_max_i(hi[a]);
  }
  __device__ __forceinline__ void join(const CountBox& o) {
#pragma unroll
    for (int c = 0; c < NC; ++c) n[c] += o.n[c];
    grow(o.lo, o.hi);
  }
  // One thread merges into the device record.  LOOK: the box only ever grows, so a bound that a (possibly stale) look already shows as reached needs no atomic: a
  // pass that merges once per wave over an all-foreground volume would otherwise queue 2 * AXES atomics per wave on 2 * AXES addresses.
  template <bool LOOK = false>
  __device__ __forceinline__ void merge(unsigned long long* cnt, int* bmin, int* bmax) const {
    if (empty()) return;
    for (int c = 0; c < NC; ++c)
      if (n[c]) atomicAdd(cnt + c, (unsigned long long)n[c]);
    for (int a = 0; a < AXES; ++a) {
      if (!LOOK || lo[a] < __hip_atomic_load(bmin + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(bmin + a, lo[a]);
      if (!LOOK || hi[a] > __hip_atomic_load(bmax + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(bmax + a, hi[a]);
    }
  }
};
// the record of a workgroup of four waves from red[wave], which lane 0 of each wave has stored after its wave_reduce()
template <int AXES, int NC>
__device__ __forceinline__ CountBox<AXES, NC> joined(const CountBox<AXES, NC> (&red)[4]) {
  CountBox<AXES, NC> b = red[0];
  for (int w = 1; w < 4; ++w) b.join(red[w]);
  return b;
}
// the empty box of an init kernel: threads 0 .. n - 1 reset one bound each (n = AXES, or the bounds of several boxes that lie one after another)
__device__ __forceinline__ void box_reset(int* bmin, int* bmax, int n) {
  if (threadIdx.x < n) bmin[threadIdx.x] = INT_MAX, bmax[threadIdx.x] = -1;
}

inline int64_t align256(int64_t v) { return (v + 255) & ~(int64_t)255; }
inline bool dims_ok(const int32_t* dims, int max_extent) {
  if (!dims) return false;
  for (int a = 0; a < 3; ++a)
    if (dims[a] < 1 || dims[a] > max_extent) return false;
  return true;
}
inline bool aligned_to(const void* p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

// The checks that every launcher of the three files starts with, in this order; `name` is the entry point.  pointers_ok / dims_also / aligned_ok are the caller's
// conditions (dims_also: beyond 1 .. max_extent per axis), the *_note strings end their messages; spacing may be null (no spacing argument); `needed` is evaluated
// after the dims have passed, and needed_from names the entry point that reports it.
#define VOLUME_CHECK_ARGS(name, pointers_ok, pointers_note, pitch, dims, max_extent, dims_also, dims_note, spacing, aligned_ok, aligned_note, scratch_bytes, needed, needed_from) \
  do {                                                                                                                                                                             \
    VSSEG_CHECK(pointers_ok, "%s: null pointer%s", name, pointers_note);                                                                                                           \
    VSSEG_CHECK((pitch) == 2, "%s: pitch must be 2 (channels-last two-class logits), got %d", name, pitch);                                                                        \
    VSSEG_CHECK(dims_ok(dims, max_extent) && (dims_also), "%s: dims must be 1 .. %d on every axis%s", name, max_extent, dims_note);                                                \
    for (int a_ = 0; (spacing) && a_ < 3; ++a_)                                                                                                                                    \
      VSSEG_CHECK((spacing)[a_] > 0.f && (spacing)[a_] < __builtin_inff(), "%s: spacing[%d] = %g is not a positive finite value", name, a_, (double)(spacing)[a_]);                \
    VSSEG_CHECK(aligned_ok, "%s: misaligned operand (%s)", name, aligned_note);                                                                                                    \
    VSSEG_CHECK((scratch_bytes) >= (needed), "%s: %lld bytes of scratch, %lld needed (%s)", name, (long long)(scratch_bytes), (long long)(needed), needed_from);                   \
  } while (0)
