// Sampling: the last operation of every decode step, one 1024-thread workgroup per row of logits with
// 16-byte loads (8 x bf16 per lane, 8 independent loads in flight per lane).
//
//   lta_argmax_rows  greedy: row-wise argmax (`logits[:, -1].argmax(-1)`).  PyTorch's generic reduction
//                    takes ~40 us for one 128k-wide bf16 row on MI355X; this needs a fraction of that.
//                    Ties resolve to the smallest index and NaN wins, as torch.argmax does.
//   lta_sample_rows  temperature / top-k / top-p sampling in one launch (definition: ops/sampling.py).
//                    The row is re-read from L2 per pass: row max, radix select of the top-k threshold,
//                    the same descent over softmax mass for the top-p threshold, then a Gumbel-max draw
//                    from the project's Philox stream over the kept set.
#include "common.h"

namespace lta {
namespace {

constexpr int kThreads = 1024;

__device__ __forceinline__ bool better(float v, int64_t i, float bv, int64_t bi) {
  const bool vn = v != v, bn = bv != bv;
  if (vn || bn) return vn && (!bn || i < bi);
  return v > bv || (v == bv && i < bi);
}

// f(element, index) for every element of a row: 16-byte vectors, G of them loaded per lane before
// they are used (8 x 16 B in flight), then the scalar tail of V % NV elements.  f is instantiated
// G * NV times: a long body takes a smaller G.
template <int G, typename T, typename F>
__device__ __forceinline__ void for_each_in_row(const T* __restrict__ row, int64_t V, F&& f) {
  constexpr int NV = Vec16<T>::N;
  const int64_t nvec = V / NV;
  for (int64_t c0 = threadIdx.x; c0 < nvec; c0 += (int64_t)G * kThreads) {
    Vec16<T> p[G];
#pragma unroll
    for (int u = 0; u < G; ++u)
      if (c0 + u * kThreads < nvec) p[u] = load16(row + (c0 + u * kThreads) * NV);
#pragma unroll
    for (int u = 0; u < G; ++u) {
      const int64_t c = c0 + u * kThreads;
      if (c < nvec) {
#pragma unroll
        for (int e = 0; e < NV; ++e) f(p[u].v[e], c * NV + e);
      }
    }
  }
  for (int64_t j = nvec * NV + threadIdx.x; j < V; j += kThreads) f(row[j], j);
}

// The block's best (value, index) under `better`, returned to every thread.
__device__ __forceinline__ void block_best(float& bv, int64_t& bi, float* sv, int64_t* si) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float ov = __shfl_xor(bv, off, 64);
    const int64_t oi = __shfl_xor(bi, off, 64);
    if (better(ov, oi, bv, bi)) {
      bv = ov;
      bi = oi;
    }
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();  // sv / si may still be read from an earlier call
  if (lane == 0) {
    sv[w] = bv;
    si[w] = bi;
  }
  __syncthreads();
  bv = sv[0];
  bi = si[0];
  for (int u = 1; u < kThreads / 64; ++u)
    if (better(sv[u], si[u], bv, bi)) {
      bv = sv[u];
      bi = si[u];
    }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void argmax_rows_kernel(const T* __restrict__ x, int64_t* __restrict__ out,
                                                               int64_t V, int64_t ld) {
  __shared__ float sv[kThreads / 64];
  __shared__ int64_t si[kThreads / 64];
  float bv = -INFINITY;
  int64_t bi = V;  // sentinel larger than every index
  for_each_in_row<8>(x + blockIdx.x * ld, V, [&](T raw, int64_t i) {
    const float v = to_f32(raw);
    if (better(v, i, bv, bi)) {
      bv = v;
      bi = i;
    }
  });
  block_best(bv, bi, sv, si);
  if (threadIdx.x == 0) out[blockIdx.x] = bi < V ? bi : 0;
}

// ------------------------------------------------------------------------------------------------
// lta_sample_rows
// ------------------------------------------------------------------------------------------------
// Order-preserving unsigned key of a stored value that is not NaN: a < b as floats <=> key(a) < key(b),
// and -0.0 has the key of +0.0.  16-bit types keep 16-bit keys (two 8-bit radix passes, fp32 four).
__device__ __forceinline__ uint32_t ordered_key(uint32_t b, uint32_t sign) {
  if (b == sign) b = 0;  // -0.0
  return (b & sign) ? (~b & (sign | (sign - 1))) : (b | sign);
}

template <typename T> struct Key;
template <> struct Key<__hip_bfloat16> {
  static constexpr int kBits = 16;
  static __device__ __forceinline__ uint32_t of(__hip_bfloat16 v) { return ordered_key(__builtin_bit_cast(unsigned short, v), 0x8000u); }
};
template <> struct Key<__half> {
  static constexpr int kBits = 16;
  static __device__ __forceinline__ uint32_t of(__half v) { return ordered_key(__builtin_bit_cast(unsigned short, v), 0x8000u); }
};
template <> struct Key<float> {
  static constexpr int kBits = 32;
  static __device__ __forceinline__ uint32_t of(float v) { return ordered_key(__float_as_uint(v), 0x80000000u); }
};

// Philox4x32-10, the convention of core/rng.py (PHILOX_HIP): counter (blk_lo, blk_hi, off_lo, off_hi), key (seed, 0)
__device__ __forceinline__ void philox4(unsigned seed, unsigned long long off, unsigned long long blk, unsigned* w) {
  unsigned c0 = (unsigned)blk, c1 = (unsigned)(blk >> 32), c2 = (unsigned)off, c3 = (unsigned)(off >> 32);
  unsigned k0 = seed, k1 = 0u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0;
    const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
    c1 = (unsigned)p1;
    c3 = (unsigned)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  w[0] = c0;
  w[1] = c1;
  w[2] = c2;
  w[3] = c3;
}

constexpr int kBins = 256;   // 8 key bits per radix pass
constexpr int kCopies = 16;  // copies of every bin, one per lane % 16: 64 lanes on one bin are a 4-way, not a 64-way, LDS conflict
typedef unsigned long long u64;

struct RadixLds {
  u64 bins[kBins * kCopies];  // 32 KiB
  u64 tot[kBins / 64];        // weight of each wave of 64 bins
  u64 sel[2];                 // digit chosen in this pass, weight of the keys above it
};

// Radix select, 8 key bits per pass from the top: the largest key k that occurs among the row's elements
// with key >= kmin for which
//   sum of weight(x) over { key(x) >= k }  >=  target,        target = target_of(that sum for k = kmin).
// With weight 1 and target top_k this is the top_k-th largest value, with the softmax mass the top-p
// threshold.  The weights are integers and meet in integer LDS atomics, so the result does not depend on the
// order in which lanes and waves arrive.
template <typename T, typename W, typename TG>
__device__ __forceinline__ uint32_t radix_threshold(const T* __restrict__ row, int64_t V, uint32_t kmin, W&& weight,
                                                    TG&& target_of, RadixLds& s) {
  constexpr int KB = Key<T>::kBits;
  const int tid = threadIdx.x;
  uint32_t prefix = 0;
  u64 above = 0, target = 0;
  for (int p = 0; p < KB / 8; ++p) {
    for (int i = tid; i < kBins * kCopies; i += kThreads) s.bins[i] = 0;
    __syncthreads();
    const int shift = KB - 8 * (p + 1);
    for_each_in_row<8>(row, V, [&](T raw, int64_t) {
      const uint32_t k = Key<T>::of(raw);
      if (k >= kmin && (p == 0 || (k >> (shift + 8)) == prefix))
        atomicAdd(&s.bins[((k >> shift) & (kBins - 1)) * kCopies + (tid & (kCopies - 1))], weight(to_f32(raw)));
    });
    __syncthreads();
    // suffix sums over the 256 bins (one per thread of the first 4 waves): in the wave by shuffles, then across waves
    u64 t = 0;
    if (tid < kBins) {
#pragma unroll
      for (int j = 0; j < kCopies; ++j) t += s.bins[tid * kCopies + ((j + tid) & (kCopies - 1))];  // rotated: no bank conflict
    }
    const int lane = tid & 63, wv = tid >> 6;
    u64 ge = t;  // weight of this wave's bins >= mine
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const u64 o = __shfl_down(ge, off, 64);
      if (lane + off < 64) ge += o;
    }
    if (lane == 0 && wv < kBins / 64) s.tot[wv] = ge;
    __syncthreads();
    if (p == 0) {
      u64 all = 0;
      for (int u = 0; u < kBins / 64; ++u) all += s.tot[u];
      target = target_of(all);
    }
    if (tid < kBins) {
      u64 before = above + ge - t;
      for (int u = wv + 1; u < kBins / 64; ++u) before += s.tot[u];
      if (before < target && target <= before + t) {  // true for exactly one bin, and that bin is occupied
        s.sel[0] = tid;
        s.sel[1] = before;
      }
    }
    __syncthreads();
    prefix = (prefix << 8) | (uint32_t)s.sel[0];
    above = s.sel[1];
  }
  return prefix;
}

constexpr float kMassScale = 1099511627776.0f;  // 2^40: masses in (0, 1] as fixed point, a row of 2^18 sums below 2^58

__device__ __forceinline__ float gumbel_score(float z, unsigned word) {
  const float u = (float)(2u * (word >> 9) + 1u) * 0x1p-24f;  // exact, strictly inside (0, 1)
  return z - logf(-logf(u));                                  // accurate logf: winners have u next to 1
}

template <typename T>
__global__ __launch_bounds__(kThreads) void sample_rows_kernel(const T* __restrict__ x, int64_t* __restrict__ out,
                                                               int64_t V, int64_t ld, float temperature, int64_t top_k,
                                                               float top_p, unsigned seed, u64 offset) {
  __shared__ float sv[kThreads / 64];
  __shared__ int64_t si[kThreads / 64];
  __shared__ RadixLds radix;
  const T* row = x + blockIdx.x * ld;

  // 1. row maximum; the special rows end here as argmax does: first NaN, else first +inf, else (all -inf) 0
  float xmax = -INFINITY;
  int64_t imax = V;
  for_each_in_row<8>(row, V, [&](T raw, int64_t i) {
    const float v = to_f32(raw);
    if (better(v, i, xmax, imax)) {
      xmax = v;
      imax = i;
    }
  });
  block_best(xmax, imax, sv, si);
  if (xmax != xmax || xmax == INFINITY || xmax == -INFINITY) {  // uniform over the block
    if (threadIdx.x == 0) out[blockIdx.x] = imax < V ? imax : 0;
    return;
  }
  const float zmax = xmax / temperature;

  // 2. / 3. the kept set is { key >= thr }
  uint32_t thr = 0;
  if (top_k >= 1 && top_k < V)
    thr = radix_threshold(row, V, 0u, [](float) { return (u64)1; }, [&](u64) { return (u64)top_k; }, radix);
  if (top_p < 1.0f)
    thr = radix_threshold(
        row, V, thr, [&](float v) { return (u64)(expf(v / temperature - zmax) * kMassScale); },
        [&](u64 total) {
          const u64 t = (u64)ceil((double)top_p * (double)total);
          return t < 1 ? (u64)1 : t > total ? total : t;
        },
        radix);

  // 4. Gumbel-max over the kept set.  Element i of row r is counter e = r * V4 + i of the call's Philox
  // range; V4 % 4 == 0, so a Philox block never spans two rows and word e % 4 is word i % 4.
  // `bound` is a score that some kept element attains, at first the row maximum's: an element that cannot
  // reach it cannot win and skips, before its Philox block if no draw would do (g < 16.64), else before its
  // two accurate logs: -log(-log u) <= -log(1 - u), and 1 - u = (2^24 - n) 2^-24 exactly, one fast log2.
  const u64 rowbase = (u64)blockIdx.x * (u64)((V + 3) / 4 * 4);
  unsigned w[4];
  philox4(seed, offset, (rowbase + (u64)imax) >> 2, w);
  const unsigned qmax = (unsigned)imax & 3u;
  float bound = gumbel_score(zmax, qmax == 0u ? w[0] : qmax == 1u ? w[1] : qmax == 2u ? w[2] : w[3]);
  u64 blk = (rowbase + (u64)imax) >> 2;
  const float inv_t = 1.0f / temperature;
  float bs = -INFINITY;
  int64_t bi = V;
  for_each_in_row<2>(row, V, [&](T raw, int64_t i) {
    const float v = to_f32(raw);
    if (Key<T>::of(raw) < thr || v == -INFINITY) return;
    const float za = v * inv_t;                        // within 2^-22 |z| of z: good enough to skip by
    const float slack = 1e-3f + fabsf(za) * 0x1p-20f;  // far above the rounding of either side of the comparisons
    if (za + (16.64f + slack) < bound) return;
    const u64 e = rowbase + (u64)i;
    if ((e >> 2) != blk) {
      blk = e >> 2;
      philox4(seed, offset, blk, w);
    }
    const unsigned q = (unsigned)e & 3u;
    const unsigned word = q == 0u ? w[0] : q == 1u ? w[1] : q == 2u ? w[2] : w[3];
    const float d = (float)(0x1000000u - (2u * (word >> 9) + 1u));  // (1 - u) 2^24, an integer in [1, 2^24)
    if (za + (24.0f - __log2f(d)) * 0.69314718f + slack < bound) return;
    const float sc = gumbel_score(v / temperature, word);
    if (better(sc, i, bs, bi)) {
      bs = sc;
      bi = i;
    }
    bound = fmaxf(bound, sc);
  });
  block_best(bs, bi, sv, si);
  if (threadIdx.x == 0) out[blockIdx.x] = bi < V ? bi : imax;
}

template <typename T>
int launch_sample(const void* x, void* out, int R, int64_t V, int64_t ld, float temperature, int64_t top_k, float top_p,
                  unsigned seed, u64 offset, hipStream_t s) {
  hipLaunchKernelGGL(sample_rows_kernel<T>, dim3(R), dim3(kThreads), 0, s, (const T*)x, (int64_t*)out, V, ld,
                     temperature, top_k, top_p, seed, offset);
  return (int)hipGetLastError();
}

}  // namespace
}  // namespace lta

// x: R rows of V logits (row stride ld elements; rows 16-byte aligned, ld % 8 == 0) -> out[R] int64.
LTA_EXPORT int lta_argmax_rows(int dtype, const void* x, void* out, int R, int64_t V, int64_t ld, void* stream) {
  using namespace lta;
  if (R < 1 || V < 1) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == kBF16)
    hipLaunchKernelGGL(argmax_rows_kernel<__hip_bfloat16>, dim3(R), dim3(kThreads), 0, s, (const __hip_bfloat16*)x,
                       (int64_t*)out, V, ld);
  else if (dtype == kF16)
    hipLaunchKernelGGL(argmax_rows_kernel<__half>, dim3(R), dim3(kThreads), 0, s, (const __half*)x, (int64_t*)out, V,
                       ld);
  else if (dtype == kF32)
    hipLaunchKernelGGL(argmax_rows_kernel<float>, dim3(R), dim3(kThreads), 0, s, (const float*)x, (int64_t*)out, V, ld);
  else
    return (int)hipErrorInvalidValue;
  return (int)hipGetLastError();
}

// One token per row, drawn with temperature > 0 from the logits kept by top_k (0: no top-k filter) and
// top_p (1: no nucleus filter); x, out and the preconditions as for lta_argmax_rows.  The call owns the
// Philox counters [offset, offset + R * ceil(V / 4) * 4) of `seed` (its low 32 bits).
LTA_EXPORT int lta_sample_rows(int dtype, const void* x, void* out, int R, int64_t V, int64_t ld, float temperature,
                               int64_t top_k, float top_p, int64_t seed, int64_t offset, void* stream) {
  using namespace lta;
  if (R < 1 || V < 1 || ld < 0 || ld % 8 != 0 || ((uintptr_t)x & 15) != 0) return (int)hipErrorInvalidValue;
  if (!(temperature > 0.f) || !(temperature < INFINITY) || top_k < 0 || !(top_p > 0.f) || !(top_p <= 1.f) || offset < 0)
    return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  const unsigned sd = (unsigned)seed;
  const u64 off = (u64)offset;
  if (dtype == kBF16) return launch_sample<__hip_bfloat16>(x, out, R, V, ld, temperature, top_k, top_p, sd, off, s);
  if (dtype == kF16) return launch_sample<__half>(x, out, R, V, ld, temperature, top_k, top_p, sd, off, s);
  if (dtype == kF32) return launch_sample<float>(x, out, R, V, ld, temperature, top_k, top_p, sd, off, s);
  return (int)hipErrorInvalidValue;
}
