// Surface-distance metrics of a two-class segmentation against its label: 95th-percentile (any percentile) Hausdorff distance and average
// symmetric surface distance, for one volume per call, as a sequence of launches on the caller's stream (no host synchronisation, no allocation):
//
//   init      zero the record in scratch (counts, bounding box, radix-select state, histograms)
//   edge      one pass over the volume: P = argmax of the two logits (ties -> class 0), G = ((int)label == 1); E(M) = M AND NOT erode(M) with the
//             6-connected cross, outside = background.  One byte per voxel (bit 0: E(P), bit 1: E(G)), |E(P)|, |E(G)| and the bounding box of
//             E(P) u E(G) into the record.  Reads 12 B and writes 1 B per voxel: the only pass whose cost grows with the volume.
//   edt x3    exact squared Euclidean distance transform to E(G) and to E(P) (both fields in one float2 per voxel), restricted to the bounding
//             box (every feature and every query voxel is inside it, so the restriction is exact): three separable per-axis passes
//             out[a] = min_a' (s * (a - a'))^2 + in[a'], each line staged in LDS and minimised by brute force (no envelope: the exact minimum up to
//             fp32 rounding).  The grids are sized for the whole volume; workgroups outside the box (which lives in device memory) exit at once.
//   hist/select x4   an 8-bit radix select over the fp32 bit patterns of the distances at the edge voxels (non-negative floats order like their
//             uint32 bits), both directions and both order statistics of the percentile at once; the first histogram pass also forms each
//             workgroup's partial sums of the distances (combined in a fixed order: the result does not depend on workgroup timing).
//   finalize  [hd, assd] as numpy.percentile (linear) and the mean over both edge sets; empty masks: NaN (both) / +inf (one).
//
// vsseg_surface_metrics is the same sequence with two additions, neither of which costs a launch or a byte of traffic: its first histogram pass,
// which already holds every edge voxel's squared field value, also counts per direction and tolerance the edge voxels with field <= tau^2 (integer
// atomics: LDS per workgroup, then one 64-bit add per non-zero counter), and its finalize also writes masd from the two per-direction sums and the
// normalised surface Dice, surface precision and surface recall of every tolerance.  vsseg_surface_distances runs the kernels it always ran.
#include <math.h>
#include "volume.h"

namespace {

constexpr int SURF_RB = 1024;                     // workgroups of the histogram passes: fixed, so that the partial sums are combined in one order
constexpr int ET_Y = 16, ET_Z = 64, ET_X = 16;    // edge pass: a workgroup owns ET_Y rows x ET_Z voxels of ET_X consecutive x planes
constexpr int EW_Y = ET_Y + 2, EW_Z = ET_Z + 2;   // ... and stages each plane with a one-voxel halo
constexpr int EDT_J = 4;                          // distance-transform outputs per thread and sweep over a line
constexpr int SURF_MAX_EXTENT = 8192;             // a line of the transform fits 64 KiB of LDS
constexpr int SURF_MAX_TOL = 8;                   // tolerances of one vsseg_surface_metrics call

struct SurfRec {
  unsigned long long cnt[2];   // |E(P)|, |E(G)|
  int bmin[3], bmax[3];        // bounding box of E(P) u E(G); bmax = -1: no edge voxel
  unsigned long long rank[4];  // selection s = 2 * direction + (0: lower, 1: upper order statistic of the percentile): rank among the values with its prefix
  unsigned prefix[4];          // ... bits of the selected value found so far, most significant byte first
  double gamma[2];             // interpolation weight between the two order statistics of a direction
  unsigned hist[4][4][256];    // radix pass, selection, bin
  unsigned long long within[2][SURF_MAX_TOL];  // direction, tolerance: edge voxels whose squared distance to the other edge set is <= tau^2
};

struct SurfTol {  // the tolerances of a call, by value in the kernel arguments
  int n;
  float t2[SURF_MAX_TOL];  // (float)(tau * tau), the product in fp64
};

struct SurfLayout {
  int64_t partial, edges, field, total;
};
SurfLayout surf_layout(int64_t nvox) {
  SurfLayout l;
  l.partial = align256(sizeof(SurfRec));
  l.edges = l.partial + align256(SURF_RB * 2 * sizeof(double));
  l.field = l.edges + align256(nvox);
  l.total = l.field + align256(nvox * (int64_t)sizeof(float2));
  return l;
}

__device__ __forceinline__ unsigned surf_mask(const float* __restrict__ logits, const float* __restrict__ label, int64_t v) {
  const float2 l = *reinterpret_cast<const float2*>(logits + 2 * v);
  return (vsseg_pred_fg(l) ? 1u : 0u) | (vsseg_label_fg(label[v]) ? 2u : 0u);
}

__global__ __launch_bounds__(256) void surf_init_kernel(SurfRec* rec) {
  unsigned* w = reinterpret_cast<unsigned*>(rec);
  for (int i = threadIdx.x; i < (int)(sizeof(SurfRec) / 4); i += 256) w[i] = 0;
  __syncthreads();
  box_reset(rec->bmin, rec->bmax, 3);
}

__global__ __launch_bounds__(256) void surf_edge_kernel(const float* __restrict__ logits, const float* __restrict__ label, int X, int Y, int Z, uint8_t* __restrict__ edges,
                                                       SurfRec* __restrict__ rec) {
  // ring of four staged planes (plane x in win[x & 3]): iteration x writes plane x + 1 over plane x - 3, whose last readers passed iteration x - 1's barrier
  __shared__ uint8_t win[4][EW_Y][EW_Z];
  __shared__ CountBox<3, 2> red[4];
  const int z0 = blockIdx.x * ET_Z, y0 = blockIdx.y * ET_Y, x0 = blockIdx.z * ET_X;
  const int x1 = min(x0 + ET_X, X);
  const int tz = threadIdx.x & 63, ty = threadIdx.x >> 6;  // rows ty, ty + 4, ty + 8, ty + 12 of column tz
  auto stage = [&](int x) {
    uint8_t(*w)[EW_Z] = win[x & 3];
    for (int i = threadIdx.x; i < EW_Y * EW_Z; i += 256) {
      const int r = i / EW_Z, c = i - r * EW_Z;
      const int y = y0 - 1 + r, z = z0 - 1 + c;
      unsigned m = 0;
      if (x >= 0 && x < X && y >= 0 && y < Y && z >= 0 && z < Z) m = surf_mask(logits, label, ((int64_t)x * Y + y) * Z + z);
      w[r][c] = (uint8_t)m;
    }
  };
  stage(x0 - 1);
  stage(x0);
  CountBox<3, 2> box;  // |E(P)|, |E(G)| and the box of both
  box.clear();
  const int z = z0 + tz, c = tz + 1;
  for (int x = x0; x < x1; ++x) {
    stage(x + 1);
    __syncthreads();
    const uint8_t(*wp)[EW_Z] = win[(x - 1) & 3];
    const uint8_t(*wc)[EW_Z] = win[x & 3];
    const uint8_t(*wn)[EW_Z] = win[(x + 1) & 3];
#pragma unroll
    for (int k = 0; k < ET_Y / 4; ++k) {
      const int r = ty + 4 * k + 1, y = y0 + r - 1;
      if (y >= Y || z >= Z) continue;
      const unsigned inner = wp[r][c] & wn[r][c] & wc[r - 1][c] & wc[r + 1][c] & wc[r][c - 1] & wc[r][c + 1];
      const unsigned e = wc[r][c] & ~inner & 3u;
      edges[((int64_t)x * Y + y) * Z + z] = (uint8_t)e;
      if (e) {
        box.n[0] += e & 1u;
        box.n[1] += e >> 1;
        box.grow({x, y, z}, {x, y, z});
      }
    }
  }
  box.wave_reduce();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = box;
  __syncthreads();
  if (threadIdx.x == 0) joined(red).merge(rec->cnt, rec->bmin, rec->bmax);  // one set of atomics per workgroup that saw an edge voxel
}

// One per-axis pass of the squared distance transform inside the box, both fields at once (.x: to E(G), .y: to E(P)).  AX = 2 (along z) is the
// first pass and reads the edge bytes (0 on a feature voxel, +inf elsewhere); AX = 1 (y) and AX = 0 (x) rewrite the box field in place (each line
// belongs to one workgroup, staged before it is written).  A workgroup stages PT = 1 << pt_log2 neighbouring lines [n][PT] in LDS; thread
// (line p, group ag) computes the outputs ag, ag + G, ag + 2G, ... (G = 256 / PT), EDT_J of them per sweep over the line.
template <int AX>
__global__ __launch_bounds__(256) void surf_edt_kernel(const SurfRec* __restrict__ rec, const uint8_t* __restrict__ edges, int Y, int Z, float2* __restrict__ field, float s, int pt_log2) {
  extern __shared__ float2 line[];
  const int bx = rec->bmax[0] - rec->bmin[0] + 1, by = rec->bmax[1] - rec->bmin[1] + 1, bz = rec->bmax[2] - rec->bmin[2] + 1;
  if (bx <= 0) return;  // no edge voxel: bmax = -1 on every axis
  const int PT = 1 << pt_log2;
  int n, np, nq;
  int64_t sa, sp, sq;
  if (AX == 2) n = bz, np = by, nq = bx, sa = 1, sp = bz, sq = (int64_t)by * bz;
  else if (AX == 1) n = by, np = bz, nq = bx, sa = bz, sp = 1, sq = (int64_t)by * bz;
  else n = bx, np = bz, nq = by, sa = (int64_t)by * bz, sp = 1, sq = bz;
  const int q = blockIdx.y, p0 = blockIdx.x * PT;
  if (q >= nq || p0 >= np) return;
  const int npt = min(PT, np - p0);
  const float INF = __builtin_inff();
  const int64_t base = (int64_t)q * sq + (int64_t)p0 * sp;
  for (int i = threadIdx.x; i < n * PT; i += 256) {
    int a, p;
    if (AX == 2) p = i / n, a = i - p * n;  // consecutive threads along a line: contiguous edge bytes
    else a = i >> pt_log2, p = i & (PT - 1);  // consecutive threads across lines: contiguous field
    float2 g = make_float2(INF, INF);
    if (p < npt) {
      if (AX == 2) {
        const unsigned e = edges[((int64_t)(rec->bmin[0] + q) * Y + (rec->bmin[1] + p0 + p)) * Z + rec->bmin[2] + a];
        g = make_float2((e & 2u) ? 0.f : INF, (e & 1u) ? 0.f : INF);
      } else {
        g = field[base + (int64_t)p * sp + (int64_t)a * sa];
      }
    }
    line[a * PT + p] = g;
  }
  __syncthreads();
  const int G = 256 >> pt_log2, p = threadIdx.x & (PT - 1), ag = threadIdx.x >> pt_log2;
  for (int a0 = ag; a0 < n; a0 += G * EDT_J) {
    float fa[EDT_J], b0[EDT_J], b1[EDT_J];
#pragma unroll
    for (int j = 0; j < EDT_J; ++j) fa[j] = (float)(a0 + j * G), b0[j] = INF, b1[j] = INF;
    for (int a2 = 0; a2 < n; ++a2) {
      const float2 g = line[a2 * PT + p];
      const float f2 = (float)a2;
#pragma unroll
      for (int j = 0; j < EDT_J; ++j) {
        const float d = s * (fa[j] - f2);  // integer difference (exact), then the spacing
        b0[j] = fminf(b0[j], fmaf(d, d, g.x));
        b1[j] = fminf(b1[j], fmaf(d, d, g.y));
      }
    }
    if (p < npt) {
#pragma unroll
      for (int j = 0; j < EDT_J; ++j) {
        const int a = a0 + j * G;
        if (a < n) field[base + (int64_t)p * sp + (int64_t)a * sa] = make_float2(b0[j], b1[j]);
      }
    }
  }
}

// Histogram pass `pass` (0: bits 31..24, ..., 3: bits 7..0) of the radix select over the distances at the edge voxels: d(P->G) = sqrt(field.x) at
// E(P), d(G->P) = sqrt(field.y) at E(G).  A value counts for selection s when its higher bits equal the prefix found so far.  One wave per box row
// (x, y), lanes along z; the row -> wave assignment depends on the box only, so pass 0's per-workgroup partial sums are reproducible.
// TOL (pass 0 of vsseg_surface_metrics only): also count, per direction and tolerance, the values whose SQUARED distance, the field value itself, is
// <= tol.t2 (a tie counts, +inf never does).  Edge voxels are a few thousand per volume, so the counts go through LDS atomics.
template <bool TOL>
__global__ __launch_bounds__(256) void surf_hist_kernel(SurfRec* __restrict__ rec, const uint8_t* __restrict__ edges, const float2* __restrict__ field, int Y, int Z, int pass,
                                                       double* __restrict__ partial, SurfTol tol) {
  __shared__ unsigned h[4][256];
  __shared__ double red[4][2];
  __shared__ unsigned within[2][SURF_MAX_TOL];
  for (int i = threadIdx.x; i < 4 * 256; i += 256) (&h[0][0])[i] = 0;
  if (TOL && threadIdx.x < 2 * SURF_MAX_TOL) (&within[0][0])[threadIdx.x] = 0;
  __syncthreads();
  const int bx = rec->bmax[0] - rec->bmin[0] + 1, by = rec->bmax[1] - rec->bmin[1] + 1, bz = rec->bmax[2] - rec->bmin[2] + 1;
  const int shift = 24 - 8 * pass;
  const unsigned hmask = (unsigned)(0xFFFFFFFF00000000ull >> (8 * pass));  // the bits already selected (none in pass 0)
  unsigned pre[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) pre[s] = rec->prefix[s] & hmask;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t rows = bx > 0 ? (int64_t)bx * by : 0;
  double sum[2] = {0.0, 0.0};
  bool any = false;
  for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < rows; r += (int64_t)gridDim.x * 4) {
    const int i = (int)(r / by), j = (int)(r - (int64_t)i * by);
    const uint8_t* er = edges + ((int64_t)(rec->bmin[0] + i) * Y + (rec->bmin[1] + j)) * Z + rec->bmin[2];
    const float2* fr = field + r * bz;
    for (int k = lane; k < bz; k += 64) {
      const unsigned e = er[k];
      if (!e) continue;
      any = true;
      const float2 f = fr[k];
#pragma unroll
      for (int d = 0; d < 2; ++d) {
        if (!((e >> d) & 1u)) continue;
        const float f2 = d ? f.y : f.x;
        const float v = sqrtf(f2);
        if (pass == 0) sum[d] += v;
        if (TOL && f2 < __builtin_inff())
          for (int t = 0; t < tol.n; ++t)
            if (f2 <= tol.t2[t]) atomicAdd(&within[d][t], 1u);
        const unsigned u = __float_as_uint(v);
#pragma unroll
        for (int t = 0; t < 2; ++t)
          if ((u & hmask) == pre[2 * d + t]) atomicAdd(&h[2 * d + t][(u >> shift) & 255u], 1u);
      }
    }
  }
  if (pass == 0) {
    const double s0 = wave_sum_d(sum[0]), s1 = wave_sum_d(sum[1]);
    if (lane == 0) red[wave][0] = s0, red[wave][1] = s1;
  }
  if (__syncthreads_or(any)) {
    for (int i = threadIdx.x; i < 4 * 256; i += 256) {
      const unsigned c = (&h[0][0])[i];
      if (c) atomicAdd(&rec->hist[pass][0][0] + i, c);
    }
    if (TOL && threadIdx.x < 2 * SURF_MAX_TOL) {  // (after the barrier above: every LDS count is final)
      const unsigned c = (&within[0][0])[threadIdx.x];
      if (c) atomicAdd(&rec->within[0][0] + threadIdx.x, (unsigned long long)c);
    }
  }
  if (pass == 0 && threadIdx.x < 2) partial[2 * blockIdx.x + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// After histogram pass `pass`: each selection takes the bin that holds its rank.  Pass 0 first turns the counts into the ranks of numpy.percentile's
// linear method: position (n - 1) * q, lower = floor, upper = min(lower + 1, n - 1).
__global__ __launch_bounds__(256) void surf_select_kernel(SurfRec* __restrict__ rec, int pass, double q) {
  __shared__ unsigned long long sc[2][256];
  __shared__ unsigned long long rank[4];
  __shared__ unsigned prefix[4];
  const int t = threadIdx.x;
  if (t < 4) {
    if (pass == 0) {
      const unsigned long long n = rec->cnt[t >> 1];
      unsigned long long k = 0;
      if (n) {
        const double pos = (double)(n - 1) * q, lo = floor(pos);
        k = (unsigned long long)lo;
        if (t & 1) k = k + 1 < n ? k + 1 : n - 1;
        if (!(t & 1)) rec->gamma[t >> 1] = pos - lo;
      }
      rank[t] = k;
      prefix[t] = 0;
    } else {
      rank[t] = rec->rank[t];
      prefix[t] = rec->prefix[t];
    }
  }
  for (int s = 0; s < 4; ++s) {
    int cur = 0;
    sc[0][t] = rec->hist[pass][s][t];
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {  // inclusive scan
      sc[cur ^ 1][t] = sc[cur][t] + (t >= o ? sc[cur][t - o] : 0ull);
      cur ^= 1;
      __syncthreads();
    }
    const unsigned long long incl = sc[cur][t], excl = t ? sc[cur][t - 1] : 0ull, k = rank[s];
    __syncthreads();
    if (excl <= k && k < incl) {  // one bin at most; none when the direction has no value
      prefix[s] |= (unsigned)t << (24 - 8 * pass);
      rank[s] = k - excl;
    }
    __syncthreads();
  }
  if (t < 4) {
    rec->rank[t] = rank[t];
    rec->prefix[t] = prefix[t];
  }
}

__device__ __forceinline__ double surf_lerp(double a, double b, double t) {  // numpy's _lerp
  const double d = b - a;
  return t >= 0.5 ? b - d * (1.0 - t) : a + d * t;
}

// ntol < 0: out = [hd, assd] (vsseg_surface_distances).  ntol >= 0: out = [hd, assd, masd] and [nsd, precision, recall] per tolerance.
__global__ __launch_bounds__(256) void surf_finalize_kernel(const SurfRec* __restrict__ rec, const double* __restrict__ partial, float* __restrict__ out, int ntol) {
  __shared__ double red[2][256];
  const int t = threadIdx.x;
  double a = 0.0, b = 0.0;
  for (int i = t; i < SURF_RB; i += 256) a += partial[2 * i], b += partial[2 * i + 1];
  red[0][t] = a, red[1][t] = b;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) red[0][t] += red[0][t + o], red[1][t] += red[1][t + o];
    __syncthreads();
  }
  if (t == 0) {
    const unsigned long long n0 = rec->cnt[0], n1 = rec->cnt[1];
    float hd, assd;
    if (!n0 && !n1) {
      hd = assd = __builtin_nanf("");
    } else if (!n0 || !n1) {
      hd = assd = __builtin_inff();
    } else {
      const double p0 = surf_lerp(__uint_as_float(rec->prefix[0]), __uint_as_float(rec->prefix[1]), rec->gamma[0]);
      const double p1 = surf_lerp(__uint_as_float(rec->prefix[2]), __uint_as_float(rec->prefix[3]), rec->gamma[1]);
      hd = (float)fmax(p0, p1);
      assd = (float)((red[0][0] + red[1][0]) / (double)(n0 + n1));
    }
    out[0] = hd;
    out[1] = assd;
    if (ntol >= 0) {
      const float NaN = __builtin_nanf("");
      const bool both = n0 && n1;
      // mean of the two directed means; one edge set empty: +inf like hd and assd, both empty: NaN
      out[2] = both ? (float)((red[0][0] / (double)n0 + red[1][0] / (double)n1) * 0.5) : hd;
      for (int k = 0; k < ntol; ++k) {
        // one empty edge set: no voxel of the other is within any tolerance of it (the field there is +inf), so the counts are 0 already
        const unsigned long long wp = both ? rec->within[0][k] : 0ull, wg = both ? rec->within[1][k] : 0ull;
        out[3 + 3 * k] = (n0 + n1) ? (float)((double)(wp + wg) / (double)(n0 + n1)) : NaN;
        out[4 + 3 * k] = n0 ? (float)((double)wp / (double)n0) : NaN;
        out[5 + 3 * k] = n1 ? (float)((double)wg / (double)n1) : NaN;
      }
    }
  }
}

int surf_pt_log2(int extent) {  // lines per distance-transform workgroup: at most 16, and [extent][lines] float2 within 64 KiB
  int l = 4;
  while (l > 0 && (int64_t)extent * (8 << l) > 65536) --l;
  return l;
}

}  // namespace

extern "C" int64_t vsseg_surface_scratch_bytes(const int32_t dims[3]) {
  VSSEG_CHECK(dims_ok(dims, SURF_MAX_EXTENT), "vsseg_surface_scratch_bytes: dims must be 1 .. %d on every axis", SURF_MAX_EXTENT);
  return surf_layout((int64_t)dims[0] * dims[1] * dims[2]).total;
}

namespace {

// The launch sequence of both entry points.  tol == nullptr: vsseg_surface_distances (two outputs, no counting); otherwise vsseg_surface_metrics.
int surf_launch(const char* who, const float* logits, int32_t pitch, const float* label, const int32_t dims[3], const float spacing[3], double percentile, const SurfTol* tol,
                void* scratch, int64_t scratch_bytes, float* out, void* stream) {
  VOLUME_CHECK_ARGS(who, logits && label && scratch && out && spacing, "", pitch, dims, SURF_MAX_EXTENT, true, "", spacing,
                    aligned_to(logits, 8) && aligned_to(label, 4) && aligned_to(out, 4) && aligned_to(scratch, 256), "logits 8 B, label / out 4 B, scratch 256 B", scratch_bytes,
                    surf_layout((int64_t)dims[0] * dims[1] * dims[2]).total, "vsseg_surface_scratch_bytes");
  VSSEG_CHECK(percentile >= 0.0 && percentile <= 100.0, "%s: percentile %g outside [0, 100]", who, percentile);
  const int X = dims[0], Y = dims[1], Z = dims[2];
  const SurfLayout l = surf_layout((int64_t)X * Y * Z);
  hipStream_t s = as_stream(stream);
  char* base = static_cast<char*>(scratch);
  SurfRec* rec = reinterpret_cast<SurfRec*>(base);
  double* partial = reinterpret_cast<double*>(base + l.partial);
  uint8_t* edges = reinterpret_cast<uint8_t*>(base + l.edges);
  float2* field = reinterpret_cast<float2*>(base + l.field);
  const SurfTol none = {};
  hipLaunchKernelGGL(surf_init_kernel, dim3(1), dim3(256), 0, s, rec);
  hipLaunchKernelGGL(surf_edge_kernel, dim3((Z + ET_Z - 1) / ET_Z, (Y + ET_Y - 1) / ET_Y, (X + ET_X - 1) / ET_X), dim3(256), 0, s, logits, label, X, Y, Z, edges, rec);
  const int pz = surf_pt_log2(Z), py = surf_pt_log2(Y), px = surf_pt_log2(X);
  hipLaunchKernelGGL(surf_edt_kernel<2>, dim3((Y + (1 << pz) - 1) >> pz, X), dim3(256), (size_t)Z * (8 << pz), s, rec, edges, Y, Z, field, spacing[2], pz);
  hipLaunchKernelGGL(surf_edt_kernel<1>, dim3((Z + (1 << py) - 1) >> py, X), dim3(256), (size_t)Y * (8 << py), s, rec, edges, Y, Z, field, spacing[1], py);
  hipLaunchKernelGGL(surf_edt_kernel<0>, dim3((Z + (1 << px) - 1) >> px, Y), dim3(256), (size_t)X * (8 << px), s, rec, edges, Y, Z, field, spacing[0], px);
  for (int pass = 0; pass < 4; ++pass) {
    if (pass == 0 && tol && tol->n > 0)
      hipLaunchKernelGGL(surf_hist_kernel<true>, dim3(SURF_RB), dim3(256), 0, s, rec, edges, (const float2*)field, Y, Z, pass, partial, *tol);
    else
      hipLaunchKernelGGL(surf_hist_kernel<false>, dim3(SURF_RB), dim3(256), 0, s, rec, edges, (const float2*)field, Y, Z, pass, partial, none);
    hipLaunchKernelGGL(surf_select_kernel, dim3(1), dim3(256), 0, s, rec, pass, percentile / 100.0);
  }
  hipLaunchKernelGGL(surf_finalize_kernel, dim3(1), dim3(256), 0, s, (const SurfRec*)rec, (const double*)partial, out, tol ? tol->n : -1);
  VSSEG_LAUNCH_CHECK(who);
  return VSSEG_OK;
}

}  // namespace

extern "C" int vsseg_surface_distances(const float* logits, int32_t pitch, const float* label, const int32_t dims[3], const float spacing[3], double percentile, void* scratch,
                                       int64_t scratch_bytes, float* out, void* stream) {
  return surf_launch("vsseg_surface_distances", logits, pitch, label, dims, spacing, percentile, nullptr, scratch, scratch_bytes, out, stream);
}

extern "C" int vsseg_surface_metrics(const float* logits, int32_t pitch, const float* label, const int32_t dims[3], const float spacing[3], double percentile,
                                     const float* tolerances_mm, int32_t ntol, void* scratch, int64_t scratch_bytes, float* out, void* stream) {
  VSSEG_CHECK(ntol >= 0 && ntol <= SURF_MAX_TOL, "vsseg_surface_metrics: ntol = %d outside 0 .. %d", ntol, SURF_MAX_TOL);
  VSSEG_CHECK(ntol == 0 || tolerances_mm, "vsseg_surface_metrics: tolerances_mm is a null pointer with ntol = %d", ntol);
  SurfTol tol = {};
  tol.n = ntol;
  for (int t = 0; t < ntol; ++t) {
    const float tau = tolerances_mm[t];
    VSSEG_CHECK(tau >= 0.f && tau < __builtin_inff(), "vsseg_surface_metrics: tolerances_mm[%d] = %g is not a finite value >= 0", t, (double)tau);
    tol.t2[t] = (float)((double)tau * (double)tau);
  }
  return surf_launch("vsseg_surface_metrics", logits, pitch, label, dims, spacing, percentile, &tol, scratch, scratch_bytes, out, stream);
}
