// K6: fused qkv split + RoPE (forward and backward) for CDNA4.
//
// Forward: qkv [B, T, (nh + 2*ng) * hs] (output of the fused QKV projection) ->
//   q [B, nh, T, hs], k [B, ng, T, hs] with LitGPT's rotate-half RoPE on the first `rope_n`
//   elements of every head, v [B, ng, T, hs] (pure layout change).
// Backward: (dq, dk, dv) -> dqkv with the inverse rotation.
// Replaces the reference's torch.compile(Inductor) "torchcompile_cat" RoPE fusion
// (thunder/executors/torch_compile.py:205-234; benchmark LlamaQKVSplitRopeBenchmark).
//
// Each work item moves one 16-byte chunk (8 elements) of a head row and, for rotated chunks,
// also its partner chunk half a rope width away, so every HBM access is a 16-B vector.
#include "common.h"
#include "fp8_cvt.h"

using namespace lta;

namespace {

// k / v rows go to k + b*ks[0] + g*ks[1] + s*ks[2] with s = pos ? pos[t] : t: with `pos` they are
// written straight into a static KV cache at the decode positions (no separate index_copy launch).
struct KVDst {
  int64_t ksb, ksg, kss, vsb, vsg, vss;
};

// Per-row positions (ROWS, a ragged batch): cos / sin are [B*Tn, rope_n] and pos is [B*Tn], all indexed by
// b * Tn + t where the shared-position kernels index by t.  S is the cache's capacity: a token whose position
// is outside [0, S) writes no k / v row (and no scale byte), so a bad position never writes outside the cache;
// its q row is stored as usual.
struct RowsCap {
  int S;
};
struct NoRows {};

template <typename T, typename C, bool ROWS = false>
__global__ __launch_bounds__(256) void qkv_rope_fwd_kernel(const T* __restrict__ qkv, const C* __restrict__ cos_,
                                                           const C* __restrict__ sin_, T* __restrict__ q,
                                                           T* __restrict__ k, T* __restrict__ v,
                                                           const int64_t* __restrict__ pos, KVDst st, int B, int Tn,
                                                           int nh, int ng, int hs, int rope_n,
                                                           std::conditional_t<ROWS, RowsCap, NoRows> rc) {
  constexpr int VW = Vec16<T>::N;
  const int chunks = hs / VW;
  const int heads = nh + 2 * ng;
  const int64_t total = (int64_t)B * Tn * heads * chunks;
  const int half = rope_n / 2;
  for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < total; it += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(it % chunks);
    int64_t rest = it / chunks;
    const int h = (int)(rest % heads);
    rest /= heads;
    const int t = (int)(rest % Tn);
    const int b = (int)(rest / Tn);
    const int d0 = c * VW;
    const T* src = qkv + (((int64_t)b * Tn + t) * heads + h) * hs;
    T* dst;
    bool rotate;
    if (h < nh) {
      dst = q + (((int64_t)b * nh + h) * Tn + t) * hs;
      rotate = true;
    } else if (h < nh + ng) {
      int64_t s;
      if constexpr (ROWS) {
        s = pos[(int64_t)b * Tn + t];
        if (s < 0 || s >= rc.S) continue;
      } else {
        s = pos ? pos[t] : t;
      }
      dst = k + b * st.ksb + (h - nh) * st.ksg + s * st.kss;
      rotate = true;
    } else {
      int64_t s;
      if constexpr (ROWS) {
        s = pos[(int64_t)b * Tn + t];
        if (s < 0 || s >= rc.S) continue;
      } else {
        s = pos ? pos[t] : t;
      }
      dst = v + b * st.vsb + (h - nh - ng) * st.vsg + s * st.vss;
      rotate = false;
    }
    if (!rotate || d0 >= rope_n) {
      store16(dst + d0, load16(src + d0));
      continue;
    }
    if (d0 >= half) continue;  // handled together with its partner chunk
    const Vec16<T> x1 = load16(src + d0);
    const Vec16<T> x2 = load16(src + d0 + half);
    const int64_t cs_row = ROWS ? (int64_t)b * Tn + t : (int64_t)t;
    const C* cr = cos_ + cs_row * rope_n;
    const C* sr = sin_ + cs_row * rope_n;
    Vec16<T> o1, o2;
#pragma unroll
    for (int j = 0; j < VW; ++j) {
      const float a = to_f32(x1.v[j]), bb = to_f32(x2.v[j]);
      const float c1 = to_f32(cr[d0 + j]), s1 = to_f32(sr[d0 + j]);
      const float c2 = to_f32(cr[d0 + half + j]), s2 = to_f32(sr[d0 + half + j]);
      o1.v[j] = from_f32<T>(a * c1 - bb * s1);
      o2.v[j] = from_f32<T>(bb * c2 + a * s2);
    }
    store16(dst + d0, o1);
    store16(dst + d0 + half, o2);
  }
}

template <typename T, typename C>
__global__ __launch_bounds__(256) void qkv_rope_bwd_kernel(const T* __restrict__ dq, const T* __restrict__ dk,
                                                           const T* __restrict__ dv, const C* __restrict__ cos_,
                                                           const C* __restrict__ sin_, T* __restrict__ dqkv, int B,
                                                           int Tn, int nh, int ng, int hs, int rope_n) {
  constexpr int VW = Vec16<T>::N;
  const int chunks = hs / VW;
  const int heads = nh + 2 * ng;
  const int64_t total = (int64_t)B * Tn * heads * chunks;
  const int half = rope_n / 2;
  for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < total; it += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(it % chunks);
    int64_t rest = it / chunks;
    const int h = (int)(rest % heads);
    rest /= heads;
    const int t = (int)(rest % Tn);
    const int b = (int)(rest / Tn);
    const int d0 = c * VW;
    T* dst = dqkv + (((int64_t)b * Tn + t) * heads + h) * hs;
    const T* src;
    bool rotate;
    if (h < nh) {
      src = dq + (((int64_t)b * nh + h) * Tn + t) * hs;
      rotate = true;
    } else if (h < nh + ng) {
      src = dk + (((int64_t)b * ng + (h - nh)) * Tn + t) * hs;
      rotate = true;
    } else {
      src = dv + (((int64_t)b * ng + (h - nh - ng)) * Tn + t) * hs;
      rotate = false;
    }
    if (!rotate || d0 >= rope_n) {
      store16(dst + d0, load16(src + d0));
      continue;
    }
    if (d0 >= half) continue;
    const Vec16<T> g1 = load16(src + d0);
    const Vec16<T> g2 = load16(src + d0 + half);
    const C* cr = cos_ + (int64_t)t * rope_n;
    const C* sr = sin_ + (int64_t)t * rope_n;
    Vec16<T> o1, o2;
#pragma unroll
    for (int j = 0; j < VW; ++j) {
      const float a = to_f32(g1.v[j]), bb = to_f32(g2.v[j]);
      const float c1 = to_f32(cr[d0 + j]), s1 = to_f32(sr[d0 + j]);
      const float c2 = to_f32(cr[d0 + half + j]), s2 = to_f32(sr[d0 + half + j]);
      // y1 = x1*c1 - x2*s1 ; y2 = x2*c2 + x1*s2
      o1.v[j] = from_f32<T>(a * c1 + bb * s2);
      o2.v[j] = from_f32<T>(bb * c2 - a * s1);
    }
    store16(dst + d0, o1);
    store16(dst + d0 + half, o2);
  }
}

// Full-width RoPE (rope_n == hs, the Llama case), one token row per workgroup: each work item owns a
// chunk and its rotation partner half a head away, so no lane idles, and the item -> (head, chunk)
// split is a shift (no 64-bit division); cos / sin rows are read as 16-B vectors.
template <typename C>
__device__ __forceinline__ void load_cs8(const C* p, float (&o)[8]) {
  if constexpr (sizeof(C) == 4) {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
  } else {
    const Vec16<C> v = load16(p);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = to_f32(v.v[j]);
  }
}

// 8 values already rounded to T -> 8 bytes of saturating e4m3 (round to nearest even), one 8-byte store
template <typename T>
__device__ __forceinline__ void store8_e4m3(uint8_t* p, const Vec16<T>& x) {
  uint2 w;
  w.x = cvt4<false>(to_f32(x.v[0]), to_f32(x.v[1]), to_f32(x.v[2]), to_f32(x.v[3]));
  w.y = cvt4<false>(to_f32(x.v[4]), to_f32(x.v[5]), to_f32(x.v[6]), to_f32(x.v[7]));
  *reinterpret_cast<uint2*>(p) = w;
}

// Scaled e4m3 cache (ops/kv8.py): where the scale byte of a k / v head row goes, as KVDst for the rows.
struct ScaleDst {
  uint8_t *k, *v;
  int64_t ksb, ksg, kss, vsb, vsg, vss;
};
struct NoScale {};

// One k / v head row of a scaled e4m3 cache.  The row's 2 << pair_shift chunks sit in 1 << pair_shift
// consecutive lanes of one wave, a group aligned to its size and either wholly active or wholly inactive
// (all its lanes share h, and the item loop's bound is a multiple of the group), so the xor shuffles below
// read active lanes only.  amax of the values already rounded to T -> e = the smallest exponent in
// [-15, 7] with amax * 2^-e <= 448 (integer formula of ops/kv8.py; fmaxf drops a NaN, see there) ->
// bytes of x * 2^-e (exact product, then the saturating conversion) and the byte e + 127.
template <typename T>
__device__ __forceinline__ void store_row_e4m3_scaled(uint8_t* row, uint8_t* scale, int d0, int half, int pair_shift,
                                                      const Vec16<T>& a, const Vec16<T>& b) {
  float m = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) m = fmaxf(m, fmaxf(fabsf(to_f32(a.v[j])), fabsf(to_f32(b.v[j]))));
  for (int off = 1; off < (1 << pair_shift); off <<= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
  const uint32_t bits = __float_as_uint(m);  // m >= 0: no sign bit
  int e = (int)(bits >> 23) - 135 + ((bits & 0x7FFFFFu) > 0x600000u ? 1 : 0);
  e = min(max(e, -15), 7);
  const float inv = __uint_as_float((uint32_t)(127 - e) << 23);  // 2^-e
  uint2 w0, w1;
  w0.x = cvt4<false>(to_f32(a.v[0]) * inv, to_f32(a.v[1]) * inv, to_f32(a.v[2]) * inv, to_f32(a.v[3]) * inv);
  w0.y = cvt4<false>(to_f32(a.v[4]) * inv, to_f32(a.v[5]) * inv, to_f32(a.v[6]) * inv, to_f32(a.v[7]) * inv);
  w1.x = cvt4<false>(to_f32(b.v[0]) * inv, to_f32(b.v[1]) * inv, to_f32(b.v[2]) * inv, to_f32(b.v[3]) * inv);
  w1.y = cvt4<false>(to_f32(b.v[4]) * inv, to_f32(b.v[5]) * inv, to_f32(b.v[6]) * inv, to_f32(b.v[7]) * inv);
  *reinterpret_cast<uint2*>(row + d0) = w0;
  *reinterpret_cast<uint2*>(row + d0 + half) = w1;
  if (d0 == 0) *scale = (uint8_t)(e + 127);  // the group's first lane
}

// KT: the element type of the forward's k / v destination, T or uint8_t (an unscaled e4m3 cache: the
// row rounded to T as for a T cache, then converted, so the launch equals RoPE + clamp + cast + copy).
// KS: the uint8_t cache is the scaled one, one power-of-two scale byte per head row through `sd`.
// ROWS (forward only): per-row positions, see RowsCap.  All items of a workgroup share the token, so a token
// whose position is out of range skips its k / v heads as whole shuffle groups.
template <typename T, typename C, bool BWD, typename KT = T, bool KS = false, bool ROWS = false>
__global__ __launch_bounds__(256) void qkv_rope_row_kernel(const T* __restrict__ in0, const T* __restrict__ in1,
                                                           const T* __restrict__ in2, const C* __restrict__ cos_,
                                                           const C* __restrict__ sin_, T* __restrict__ out0,
                                                           KT* __restrict__ out1, KT* __restrict__ out2,
                                                           const int64_t* __restrict__ pos, KVDst st, int Tn, int nh,
                                                           int ng, int hs, int pair_shift,
                                                           std::conditional_t<KS, ScaleDst, NoScale> sd,
                                                           std::conditional_t<ROWS, RowsCap, NoRows> rc) {
  static_assert(!ROWS || !BWD, "per-row positions belong to the forward");
  // fwd: in0 = qkv, out0/1/2 = q/k/v (k/v through st); bwd: in0/1/2 = dq/dk/dv, out0 = dqkv
  constexpr int VW = 8;
  constexpr bool kE4M3 = !BWD && sizeof(KT) == 1;
  const int row = blockIdx.x;  // b * Tn + t
  const int t = row % Tn, b = row / Tn;
  const int heads = nh + 2 * ng, half = hs / 2;
  const int items = heads << pair_shift;
  const C* cr = cos_ + (int64_t)(ROWS ? row : t) * hs;
  const C* sr = sin_ + (int64_t)(ROWS ? row : t) * hs;
  for (int it = threadIdx.x; it < items; it += blockDim.x) {
    const int h = it >> pair_shift, d0 = (it & ((1 << pair_shift) - 1)) * VW;
    const T* src;
    T* dst;
    [[maybe_unused]] uint8_t* kv8 = nullptr;  // e4m3 cache: the row of a k / v head (dst unused for it)
    [[maybe_unused]] uint8_t* sc8 = nullptr;  // scaled e4m3 cache: that row's scale byte
    if constexpr (!BWD) {
      src = in0 + ((int64_t)row * heads + h) * hs;
      if (h < nh) {
        dst = out0 + (((int64_t)b * nh + h) * Tn + t) * hs;
      } else {
        int64_t s;
        if constexpr (ROWS) {
          s = pos[row];
          if (s < 0 || s >= rc.S) continue;
        } else {
          s = pos ? pos[t] : t;
        }
        if constexpr (kE4M3) {
          dst = nullptr;
          kv8 = h < nh + ng ? out1 + b * st.ksb + (h - nh) * st.ksg + s * st.kss
                            : out2 + b * st.vsb + (h - nh - ng) * st.vsg + s * st.vss;
          if constexpr (KS)
            sc8 = h < nh + ng ? sd.k + b * sd.ksb + (h - nh) * sd.ksg + s * sd.kss
                              : sd.v + b * sd.vsb + (h - nh - ng) * sd.vsg + s * sd.vss;
        } else {
          dst = h < nh + ng ? out1 + b * st.ksb + (h - nh) * st.ksg + s * st.kss
                            : out2 + b * st.vsb + (h - nh - ng) * st.vsg + s * st.vss;
        }
      }
    } else {
      dst = out0 + ((int64_t)row * heads + h) * hs;
      src = h < nh ? in0 + (((int64_t)b * nh + h) * Tn + t) * hs
                   : (h < nh + ng ? in1 + (((int64_t)b * ng + (h - nh)) * Tn + t) * hs
                                  : in2 + (((int64_t)b * ng + (h - nh - ng)) * Tn + t) * hs);
    }
    const Vec16<T> x1 = load16(src + d0), x2 = load16(src + d0 + half);
    if (h >= nh + ng) {  // v: layout change only
      if constexpr (KS) {
        store_row_e4m3_scaled(kv8, sc8, d0, half, pair_shift, x1, x2);
      } else if constexpr (kE4M3) {
        store8_e4m3(kv8 + d0, x1);
        store8_e4m3(kv8 + d0 + half, x2);
      } else {
        store16(dst + d0, x1);
        store16(dst + d0 + half, x2);
      }
      continue;
    }
    float c1[8], s1[8], c2[8], s2[8];
    load_cs8(cr + d0, c1);
    load_cs8(sr + d0, s1);
    load_cs8(cr + d0 + half, c2);
    load_cs8(sr + d0 + half, s2);
    Vec16<T> o1, o2;
#pragma unroll
    for (int j = 0; j < VW; ++j) {
      const float a = to_f32(x1.v[j]), bb = to_f32(x2.v[j]);
      if constexpr (!BWD) {
        o1.v[j] = from_f32<T>(a * c1[j] - bb * s1[j]);
        o2.v[j] = from_f32<T>(bb * c2[j] + a * s2[j]);
      } else {  // transpose of the rotation
        o1.v[j] = from_f32<T>(a * c1[j] + bb * s2[j]);
        o2.v[j] = from_f32<T>(bb * c2[j] - a * s1[j]);
      }
    }
    if constexpr (kE4M3) {
      if (kv8 != nullptr) {
        if constexpr (KS) {
          store_row_e4m3_scaled(kv8, sc8, d0, half, pair_shift, o1, o2);
        } else {
          store8_e4m3(kv8 + d0, o1);
          store8_e4m3(kv8 + d0 + half, o2);
        }
        continue;
      }
    }
    store16(dst + d0, o1);
    store16(dst + d0 + half, o2);
  }
}

// shift with (1 << shift) == hs / 16 (chunk pairs per head), or -1 when the row kernel does not apply
int row_pair_shift(int dtype, int hs, int rope_n) {
  if (dtype == kF32 || rope_n != hs || hs % 16) return -1;
  const int pairs = hs / 16;
  if (pairs & (pairs - 1)) return -1;
  int sh = 0;
  while ((1 << sh) < pairs) ++sh;
  return sh;
}

int grid_for(int64_t total) {
  int64_t g = (total + 255) / 256;
  if (g > 256 * 16) g = 256 * 16;
  return (int)(g < 1 ? 1 : g);
}

}  // namespace

#define LTA_DISPATCH_TC(dtype, cdtype, ...)                       \
  do {                                                           \
    if (dtype == kBF16 && cdtype == kF32) {                      \
      using T = __hip_bfloat16; using C = float; __VA_ARGS__;     \
    } else if (dtype == kBF16 && cdtype == kBF16) {              \
      using T = __hip_bfloat16; using C = __hip_bfloat16; __VA_ARGS__; \
    } else if (dtype == kF16 && cdtype == kF32) {                \
      using T = __half; using C = float; __VA_ARGS__;             \
    } else if (dtype == kF16 && cdtype == kF16) {                \
      using T = __half; using C = __half; __VA_ARGS__;            \
    } else if (dtype == kF32 && cdtype == kF32) {                \
      using T = float; using C = float; __VA_ARGS__;              \
    } else {                                                     \
      return -1;                                                 \
    }                                                            \
  } while (0)

// the k / v destination of the cache-writing entries out of strides[0..5] (k b,g,s | v b,g,s, in elements): 16-byte
// stores need every one a multiple of 8
static bool kv_dst(const int64_t* strides, KVDst& st) {
  if ((strides[0] | strides[1] | strides[2] | strides[3] | strides[4] | strides[5]) % 8) return false;
  st = KVDst{strides[0], strides[1], strides[2], strides[3], strides[4], strides[5]};
  return true;
}

// ROWS: per-row positions, `rc` the caches' capacity (see RowsCap); cos / sin and pos are then indexed by b * Tn + t.
template <bool ROWS>
static int qkv_rope_fwd_launch(int dtype, int cdtype, const void* qkv, const void* cos_, const void* sin_, void* q,
                               void* k, void* v, const int64_t* pos, KVDst st, int B, int Tn, int nh, int ng, int hs,
                               int rope_n, hipStream_t stream, std::conditional_t<ROWS, RowsCap, NoRows> rc) {
  if (hs % 8 || rope_n % 16 || rope_n > hs) return -2;
  if constexpr (ROWS)
    if (pos == nullptr || rc.S < 0) return -2;
  const int sh = row_pair_shift(dtype, hs, rope_n);
  if (sh >= 0) {
    LTA_DISPATCH_TC(dtype, cdtype,
                    hipLaunchKernelGGL((qkv_rope_row_kernel<T, C, false, T, false, ROWS>), dim3(B * Tn), dim3(256), 0,
                                       stream, (const T*)qkv, (const T*)nullptr, (const T*)nullptr, (const C*)cos_,
                                       (const C*)sin_, (T*)q, (T*)k, (T*)v, pos, st, Tn, nh, ng, hs, sh, NoScale{}, rc));
    return (int)hipGetLastError();
  }
  const int64_t total = (int64_t)B * Tn * (nh + 2 * ng) * (hs / (dtype == kF32 ? 4 : 8));
  LTA_DISPATCH_TC(dtype, cdtype,
                  hipLaunchKernelGGL((qkv_rope_fwd_kernel<T, C, ROWS>), dim3(grid_for(total)), dim3(256), 0, stream,
                                     (const T*)qkv, (const C*)cos_, (const C*)sin_, (T*)q, (T*)k, (T*)v, pos, st, B, Tn,
                                     nh, ng, hs, rope_n, rc));
  return (int)hipGetLastError();
}

LTA_EXPORT int lta_qkv_rope_fwd(int dtype, int cdtype, const void* qkv, const void* cos_, const void* sin_, void* q,
                                void* k, void* v, int B, int Tn, int nh, int ng, int hs, int rope_n,
                                hipStream_t stream) {
  const int64_t sg = (int64_t)Tn * hs, sb = ng * sg;
  return qkv_rope_fwd_launch<false>(dtype, cdtype, qkv, cos_, sin_, q, k, v, nullptr, KVDst{sb, sg, hs, sb, sg, hs}, B,
                                    Tn, nh, ng, hs, rope_n, stream, NoRows{});
}

// k/v written in place into caches kc/vc [B, ng, S, hs] (strides in elements, head dim contiguous and
// 16-byte aligned) at rows pos[0..Tn) (int64, one per query position).
LTA_EXPORT int lta_qkv_rope_cache_fwd(int dtype, int cdtype, const void* qkv, const void* cos_, const void* sin_,
                                      void* q, void* kc, void* vc, const void* pos, const int64_t* strides, int B,
                                      int Tn, int nh, int ng, int hs, int rope_n, hipStream_t stream) {
  KVDst st;
  if (!kv_dst(strides, st)) return -2;
  return qkv_rope_fwd_launch<false>(dtype, cdtype, qkv, cos_, sin_, q, kc, vc, (const int64_t*)pos, st, B, Tn, nh, ng,
                                    hs, rope_n, stream, NoRows{});
}

// As lta_qkv_rope_cache_fwd with uint8 caches holding unscaled OCP e4m3: k (rotated) and v are rounded
// to the activation dtype, saturated to +-448 and converted (round to nearest even), 8 bytes per store.
// Row-kernel shapes only (rope_n == hs, hs / 16 a power of two, 16-bit activations): -2 otherwise.
// KS: the scaled cache of ops/kv8.py: every k / v head row is stored as the bytes of x * 2^-e plus one scale
// byte e + 127 in ksc / vsc [B, ng, S, 1] (uint8), whose strides follow the caches': k b,g,s | v b,g,s |
// k scale b,g,s | v scale b,g,s.  A head row must fit one wave's lanes (hs <= 1024).
// ROWS: as for qkv_rope_fwd_launch.
template <bool KS, bool ROWS>
static int qkv_rope_e4m3_launch(int dtype, int cdtype, const void* qkv, const void* cos_, const void* sin_, void* q,
                                void* kc, void* vc, void* ksc, void* vsc, const void* pos, const int64_t* strides,
                                int B, int Tn, int nh, int ng, int hs, int rope_n, hipStream_t stream,
                                std::conditional_t<ROWS, RowsCap, NoRows> rc) {
  KVDst st;
  if (!kv_dst(strides, st) || ((uintptr_t)kc | (uintptr_t)vc) % 8) return -2;
  const int sh = row_pair_shift(dtype, hs, rope_n);
  if (sh < 0 || dtype == kF32) return -2;
  if constexpr (ROWS)
    if (pos == nullptr || rc.S < 0) return -2;
  std::conditional_t<KS, ScaleDst, NoScale> sd{};
  if constexpr (KS) {
    if (sh > 6 || (ROWS && (ksc == nullptr || vsc == nullptr))) return -2;
    sd = ScaleDst{(uint8_t*)ksc, (uint8_t*)vsc, strides[6], strides[7], strides[8], strides[9], strides[10], strides[11]};
  }
  LTA_DISPATCH_TC(dtype, cdtype,
                  if constexpr (sizeof(T) == 2)  // fp32 activations were refused above: no such kernel is built
                    hipLaunchKernelGGL((qkv_rope_row_kernel<T, C, false, uint8_t, KS, ROWS>), dim3(B * Tn), dim3(256), 0,
                                       stream, (const T*)qkv, (const T*)nullptr, (const T*)nullptr, (const C*)cos_,
                                       (const C*)sin_, (T*)q, (uint8_t*)kc, (uint8_t*)vc, (const int64_t*)pos, st, Tn,
                                       nh, ng, hs, sh, sd, rc));
  return (int)hipGetLastError();
}

LTA_EXPORT int lta_qkv_rope_cache_fwd_kv8(int dtype, int cdtype, const void* qkv, const void* cos_, const void* sin_,
                                          void* q, void* kc, void* vc, const void* pos, const int64_t* strides, int B,
                                          int Tn, int nh, int ng, int hs, int rope_n, hipStream_t stream) {
  return qkv_rope_e4m3_launch<false, false>(dtype, cdtype, qkv, cos_, sin_, q, kc, vc, nullptr, nullptr, pos, strides, B,
                                            Tn, nh, ng, hs, rope_n, stream, NoRows{});
}

LTA_EXPORT int lta_qkv_rope_cache_fwd_kv8s(int dtype, int cdtype, const void* qkv, const void* cos_, const void* sin_,
                                           void* q, void* kc, void* vc, void* ksc, void* vsc, const void* pos,
                                           const int64_t* strides, int B, int Tn, int nh, int ng, int hs, int rope_n,
                                           hipStream_t stream) {
  return qkv_rope_e4m3_launch<true, false>(dtype, cdtype, qkv, cos_, sin_, q, kc, vc, ksc, vsc, pos, strides, B, Tn, nh,
                                           ng, hs, rope_n, stream, NoRows{});
}

// The per-row entries (a ragged batch): cos / sin [B*Tn, rope_n], pos int64 [B*Tn], both indexed by b * Tn + t,
// and the caches' capacity S; a token with a position outside [0, S) writes nothing but its q row.  Strides,
// alignment and shape rules as for the shared-position entries.
LTA_EXPORT int lta_qkv_rope_cache_fwd_rows(int dtype, int cdtype, const void* qkv, const void* cos_, const void* sin_,
                                           void* q, void* kc, void* vc, const void* pos, const int64_t* strides, int B,
                                           int Tn, int nh, int ng, int hs, int rope_n, int S, hipStream_t stream) {
  KVDst st;
  if (!kv_dst(strides, st)) return -2;
  return qkv_rope_fwd_launch<true>(dtype, cdtype, qkv, cos_, sin_, q, kc, vc, (const int64_t*)pos, st, B, Tn, nh, ng,
                                   hs, rope_n, stream, RowsCap{S});
}

LTA_EXPORT int lta_qkv_rope_cache_fwd_kv8_rows(int dtype, int cdtype, const void* qkv, const void* cos_,
                                               const void* sin_, void* q, void* kc, void* vc, const void* pos,
                                               const int64_t* strides, int B, int Tn, int nh, int ng, int hs,
                                               int rope_n, int S, hipStream_t stream) {
  return qkv_rope_e4m3_launch<false, true>(dtype, cdtype, qkv, cos_, sin_, q, kc, vc, nullptr, nullptr, pos, strides, B,
                                           Tn, nh, ng, hs, rope_n, stream, RowsCap{S});
}

LTA_EXPORT int lta_qkv_rope_cache_fwd_kv8s_rows(int dtype, int cdtype, const void* qkv, const void* cos_,
                                                const void* sin_, void* q, void* kc, void* vc, void* ksc, void* vsc,
                                                const void* pos, const int64_t* strides, int B, int Tn, int nh, int ng,
                                                int hs, int rope_n, int S, hipStream_t stream) {
  return qkv_rope_e4m3_launch<true, true>(dtype, cdtype, qkv, cos_, sin_, q, kc, vc, ksc, vsc, pos, strides, B, Tn, nh,
                                          ng, hs, rope_n, stream, RowsCap{S});
}

LTA_EXPORT int lta_qkv_rope_bwd(int dtype, int cdtype, const void* dq, const void* dk, const void* dv, const void* cos_,
                                const void* sin_, void* dqkv, int B, int Tn, int nh, int ng, int hs, int rope_n,
                                hipStream_t stream) {
  if (hs % 8 || rope_n % 16 || rope_n > hs) return -2;
  const int sh = row_pair_shift(dtype, hs, rope_n);
  if (sh >= 0) {
    LTA_DISPATCH_TC(dtype, cdtype,
                    hipLaunchKernelGGL((qkv_rope_row_kernel<T, C, true>), dim3(B * Tn), dim3(256), 0, stream,
                                       (const T*)dq, (const T*)dk, (const T*)dv, (const C*)cos_, (const C*)sin_,
                                       (T*)dqkv, (T*)nullptr, (T*)nullptr, (const int64_t*)nullptr, KVDst{0, 0, 0, 0, 0, 0},
                                       Tn, nh, ng, hs, sh, NoScale{}, NoRows{}));
    return (int)hipGetLastError();
  }
  const int64_t total = (int64_t)B * Tn * (nh + 2 * ng) * (hs / (dtype == kF32 ? 4 : 8));
  LTA_DISPATCH_TC(dtype, cdtype,
                  hipLaunchKernelGGL((qkv_rope_bwd_kernel<T, C>), dim3(grid_for(total)), dim3(256), 0, stream,
                                     (const T*)dq, (const T*)dk, (const T*)dv, (const C*)cos_, (const C*)sin_, (T*)dqkv,
                                     B, Tn, nh, ng, hs, rope_n));
  return (int)hipGetLastError();
}
