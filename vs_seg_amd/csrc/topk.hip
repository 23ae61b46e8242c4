// The K largest of N non-negative fp32 values without sorting and without a host read: a radix select over their uint32 bit patterns (topk.h), written once over
// a "values of element i" functor and instantiated for an array (vsseg_topk_select: the machinery, testable bit for bit) and for the cross-entropy values of the
// voxels computed on the fly from logits and label (vsseg_ce_topk_select: the Dice + top-k loss, include/vsseg_hip.h).
//   hist x3   one pass over the elements per digit, most significant first: a per-workgroup LDS histogram of the digit of every element that shares the digits
//             found so far, flushed with integer atomics (order-independent).  The last pass also sums, in fixed point, the values already known to lie above the
//             threshold — those whose first two digits are above the threshold's — so there is no pass for the sum.
//   scan x3   one workgroup: the bin that holds the remaining rank, counted from the top; the elements of the bins above it go to n_gt.  After the last digit the
//             bin's count is n_eq, and the values between the threshold and the first two digits' upper end are summed FROM THE HISTOGRAM (a bin of the last pass
//             is one bit pattern: count * value, exact in fp64).
// Everything is HBM-bound streaming; the elements are read three times.
#include "topk.h"

constexpr int TOPK_THREADS = 512;
constexpr int TOPK_MAX_BLOCKS = 512;

// One element into the workgroup's histogram.  Well-classified background collapses into a few bins (every voxel with exp(-|z|) = 0 has the value 0), and 64 lanes
// adding to one LDS word serialise: the lanes that share the first counted lane's bin add once, by their number; the others add for themselves.
__device__ __forceinline__ void topk_hist_add(unsigned* h, unsigned bin, bool counted) {
  const unsigned long long act = __ballot(counted);
  if (act == 0ull) return;
  const int leader = __ffsll((long long)act) - 1;
  const unsigned lbin = (unsigned)__shfl((int)bin, leader, 64);
  const bool same = counted && bin == lbin;
  const unsigned long long sm = __ballot(same);
  if ((int)(threadIdx.x & 63) == leader) atomicAdd(&h[lbin], (unsigned)__popcll(sm));
  else if (counted && !same) atomicAdd(&h[bin], 1u);
}

// values of an array
struct TopkArray {
  const float* v;
  static constexpr bool SUM = false;
  __device__ __forceinline__ bool vec_ok(int64_t n) const { return (n & 3) == 0 && (reinterpret_cast<uintptr_t>(v) & 15) == 0; }
  __device__ __forceinline__ void load4(int64_t i, float* o) const {
    const float4 a = reinterpret_cast<const float4*>(v)[i];
    o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w;
  }
  __device__ __forceinline__ float load1(int64_t i) const { return v[i]; }
};
// cross-entropy values of the voxels of a batch: logits [n * nvox][pitch], label [n * nvox]; ce_sums_kernel's two load paths
struct TopkCE {
  const float* logits;
  const float* label;
  int pitch;
  int nvox4;  // nvox % 4 == 0
  float wfg;
  static constexpr bool SUM = true;
  __device__ __forceinline__ bool vec_ok(int64_t) const {
    return pitch == 2 && nvox4 && (reinterpret_cast<uintptr_t>(logits) & 15) == 0 && (reinterpret_cast<uintptr_t>(label) & 15) == 0;
  }
  __device__ __forceinline__ void load4(int64_t i, float* o) const {
    const float4 a = reinterpret_cast<const float4*>(logits)[2 * i], c = reinterpret_cast<const float4*>(logits)[2 * i + 1], g = reinterpret_cast<const float4*>(label)[i];
    o[0] = ce_topk_value(a.x, a.y, g.x, wfg);
    o[1] = ce_topk_value(a.z, a.w, g.y, wfg);
    o[2] = ce_topk_value(c.x, c.y, g.z, wfg);
    o[3] = ce_topk_value(c.z, c.w, g.w, wfg);
  }
  __device__ __forceinline__ float load1(int64_t i) const {
    const float2 l = *reinterpret_cast<const float2*>(logits + i * pitch);
    return ce_topk_value(l.x, l.y, label[i], wfg);
  }
};

template <class F> __global__ __launch_bounds__(TOPK_THREADS) void topk_hist_kernel(const F f, int64_t n, int pass, TopkRec* __restrict__ rec, unsigned* fxflag) {
  __shared__ unsigned h[TOPK_MAX_BINS];
  __shared__ double red[TOPK_THREADS / 64];
  const int nb = topk_bins(pass), shift = topk_shift(pass);
  for (int i = threadIdx.x; i < nb; i += TOPK_THREADS) h[i] = 0u;
  __syncthreads();
  const unsigned hmask = pass == 0 ? 0u : ~((1u << (shift + (pass == 1 ? 11 : 10))) - 1u);  // the digits already found (none in pass 0)
  const unsigned pre = pass == 0 ? 0u : rec->prefix;
  const unsigned bmask = (unsigned)nb - 1u;
  double sum = 0.0;
  auto take = [&](float v) {
    const unsigned u = topk_key(v);
    topk_hist_add(h, (u >> shift) & bmask, (u & hmask) == pre);
    if constexpr (F::SUM) {
      if (pass == TOPK_PASSES - 1 && (u & hmask) > pre) sum += (double)v;
    }
  };
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
  if (f.vec_ok(n)) {
    for (int64_t i = tid; i < (n >> 2); i += nthr) {
      float v[4];
      f.load4(i, v);
#pragma unroll
      for (int j = 0; j < 4; ++j) take(v[j]);
    }
  } else {
    for (int64_t i = tid; i < n; i += nthr) take(f.load1(i));
  }
  __syncthreads();
  unsigned long long* gh = rec->hist + topk_hist_at(pass);
  for (int i = threadIdx.x; i < nb; i += TOPK_THREADS) {
    const unsigned c = h[i];
    if (c) atomicAdd(&gh[i], (unsigned long long)c);
  }
  if constexpr (F::SUM) {
    if (pass == TOPK_PASSES - 1) {  // (block-uniform)
      const double w = wave_sum_d(sum);
      if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
      __syncthreads();
      if (threadIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < TOPK_THREADS / 64; ++i) t += red[i];
        if (t != 0.0) vsseg_fx_add(&rec->s_above, t, VSSEG_FX_STAT, fxflag);  // (a NaN is != 0: it sets the flag)
      }
    }
  }
}

// After histogram pass `pass`: the bin that holds the remaining rank, counted from the top.  One workgroup of 1024 threads, two bins a thread.
template <bool SUM> __global__ __launch_bounds__(1024) void topk_scan_kernel(TopkRec* __restrict__ rec, int pass, unsigned long long k, unsigned* fxflag) {
  __shared__ unsigned long long sc[2][1024];
  __shared__ double red[1024];
  __shared__ int found;
  const int t = threadIdx.x, nb = topk_bins(pass), shift = topk_shift(pass);
  const unsigned long long* gh = rec->hist + topk_hist_at(pass);
  const unsigned long long rank = pass == 0 ? k : rec->rank;
  const unsigned prefix = pass == 0 ? 0u : rec->prefix;
  // r = 2t, 2t + 1 count the bins from the top: bin = nb - 1 - r
  const int b0 = nb - 1 - 2 * t, b1 = nb - 2 - 2 * t;
  const unsigned long long c0 = b0 >= 0 ? gh[b0] : 0ull, c1 = b1 >= 0 ? gh[b1] : 0ull;
  if (t == 0) found = -1;
  int cur = 0;
  sc[0][t] = c0 + c1;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {  // inclusive scan
    sc[cur ^ 1][t] = sc[cur][t] + (t >= o ? sc[cur][t - o] : 0ull);
    cur ^= 1;
    __syncthreads();
  }
  const unsigned long long above0 = sc[cur][t] - (c0 + c1), above1 = above0 + c0;  // elements in the bins above b0 / b1
  // one bin at most holds the rank (exactly one: 1 <= rank <= the number of elements that share the prefix)
  if (b0 >= 0 && above0 < rank && rank <= above0 + c0) {
    found = b0;
    rec->prefix = prefix | ((unsigned)b0 << shift);
    rec->rank = rank - above0;
    rec->n_gt += above0;
    if (pass == TOPK_PASSES - 1) rec->n_eq = c0, rec->threshold_bits = prefix | (unsigned)b0;
  } else if (b1 >= 0 && above1 < rank && rank <= above1 + c1) {
    found = b1;
    rec->prefix = prefix | ((unsigned)b1 << shift);
    rec->rank = rank - above1;
    rec->n_gt += above1;
    if (pass == TOPK_PASSES - 1) rec->n_eq = c1, rec->threshold_bits = prefix | (unsigned)b1;
  }
  if (t == 0) {
    if (pass == 0) rec->k = k;
    rec->passes_done = (unsigned)pass + 1u;
  }
  if constexpr (SUM) {
    if (pass == TOPK_PASSES - 1) {
      __syncthreads();
      const int b = found;
      // the values that share the threshold's first two digits and lie above it: a bin of this pass is ONE bit pattern (an empty bin may be Inf or NaN: skipped)
      double s = 0.0;
      if (b >= 0 && b0 > b && c0) s += (double)c0 * (double)__uint_as_float(prefix | (unsigned)b0);
      if (b >= 0 && b1 > b && c1) s += (double)c1 * (double)__uint_as_float(prefix | (unsigned)b1);
      red[t] = s;
      __syncthreads();
      for (int o = 512; o > 0; o >>= 1) {  // a fixed tree: the same bits every time
        if (t < o) red[t] += red[t + o];
        __syncthreads();
      }
      if (t == 0) {
        rec->s_tail = red[0];
        const float thr = __uint_as_float(b >= 0 ? (prefix | (unsigned)b) : 0xFFFFFFFFu);
        if (!(fabs(red[0]) < (double)INFINITY) || !(fabsf(thr) < INFINITY)) atomicOr(fxflag, 1u);  // a NaN / Inf among the selected: the loss is NaN (vsseg_fx_poison)
      }
    }
  }
}

template <class F> static int topk_select_launch(const F& f, int64_t n, int64_t k, void* scratch, void* stream, const char* who) {
  VSSEG_FX_FLAG(fxflag, "vsseg_topk_select");
  TopkRec* rec = reinterpret_cast<TopkRec*>(scratch);
  const int64_t want = (n / 4 + TOPK_THREADS * 2 - 1) / (TOPK_THREADS * 2);
  const int blocks = (int)(want < 1 ? 1 : (want > TOPK_MAX_BLOCKS ? TOPK_MAX_BLOCKS : want));
  hipStream_t s = as_stream(stream);
  for (int pass = 0; pass < TOPK_PASSES; ++pass) {
    hipLaunchKernelGGL(topk_hist_kernel<F>, dim3(blocks), dim3(TOPK_THREADS), 0, s, f, n, pass, rec, fxflag);
    hipLaunchKernelGGL(topk_scan_kernel<F::SUM>, dim3(1), dim3(1024), 0, s, rec, pass, (unsigned long long)k, fxflag);
  }
  VSSEG_LAUNCH_CHECK(who);
  return VSSEG_OK;
}

extern "C" int64_t vsseg_topk_scratch_bytes(void) { return (int64_t)sizeof(TopkRec); }

extern "C" int vsseg_topk_select(const float* values, int64_t n, int64_t k, void* scratch, void* stream) {
  VSSEG_CHECK(values && scratch && n >= 1, "vsseg_topk_select: bad arguments");
  VSSEG_CHECK(k >= 1 && k <= n, "vsseg_topk_select: k = %lld is not in [1, n = %lld]", (long long)k, (long long)n);
  VSSEG_CHECK((reinterpret_cast<uintptr_t>(scratch) & 7) == 0, "vsseg_topk_select: scratch must be 8-byte aligned");
  return topk_select_launch(TopkArray{values}, n, k, scratch, stream, "vsseg_topk_select");
}

extern "C" int vsseg_ce_topk_select(const float* logits, int32_t pitch, const float* label, int32_t n, int64_t nvox, double ce_foreground_weight, int64_t k, void* scratch, void* stream) {
  VSSEG_CHECK(logits && label && scratch && pitch >= 2 && pitch % 2 == 0 && n >= 1 && nvox >= 1, "vsseg_ce_topk_select: bad arguments");
  VSSEG_CHECK(ce_foreground_weight > 0.0 && ce_foreground_weight < INFINITY, "vsseg_ce_topk_select: ce_foreground_weight must be finite and > 0");
  VSSEG_CHECK(k >= 1 && k <= (int64_t)n * nvox, "vsseg_ce_topk_select: k = %lld is not in [1, n * nvox = %lld]", (long long)k, (long long)n * (long long)nvox);
  VSSEG_CHECK((reinterpret_cast<uintptr_t>(scratch) & 7) == 0, "vsseg_ce_topk_select: scratch must be 8-byte aligned");
  return topk_select_launch(TopkCE{logits, label, pitch, (nvox & 3) == 0 ? 1 : 0, (float)ce_foreground_weight}, (int64_t)n * nvox, k, scratch, stream, "vsseg_ce_topk_select");
}
