// Decode attention for small query counts (K3d): softmax(q k^T * scale + mask) v for T <= 16 query
// rows against a long key/value cache (incremental decoding with a static KV cache, HF/LitGPT
// "mask from a cache of masks" style), GQA, bool or no mask, optional top-left causal.
//
// Why not the flash kernel: with T = 1 an MFMA tile would be 97% padding; decode is bound by
// reading K/V once.  Layout of the work (wave64, CDNA4):
//   * one wave owns one query row (b, hq, t); a 256-thread block holds 4 rows with consecutive
//     hq, i.e. heads of the same KV group (GQA) -> the 4 waves stream the same K/V rows (L1/L2 hits);
//   * lane l owns key j0+l of each 64-key block for both products: QK^T reads its K row with
//     16-byte loads against q broadcast from LDS, PV accumulates p * V-row into a per-lane
//     acc[D] (no serial per-key loop); a block whose mask is all-false is skipped before any
//     K/V byte is read;
//   * online softmax with wave max/sum butterflies once per 64 keys;
//   * the per-lane partial outputs are combined once per row by a recursive-halving
//     reduce-scatter of shuffles (D/2 + D/4 + ... + D/64 of them), leaving each lane D/64
//     contiguous output dims;
//   * split-K over the cache (grid.y) when the cache is long: partial (m, l, acc) go to an fp32
//     workspace and a combine kernel merges them (flash-decoding).
#include "common.h"

namespace lta {
namespace {

constexpr int kRowsPerBlock = 4;

// One 16-byte load of an e4m3 cache row (uint8 storage) as 16 fp32 values, unpacked two at a time by the
// hardware conversion (OCP e4m3 on gfx950; exact).
__device__ __forceinline__ void load16_e4m3(const uint8_t* p, float (&f)[16]) {
  const uint4 x = *reinterpret_cast<const uint4*>(p);
  const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false);
    const auto hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);
    f[4 * i + 0] = lo[0];
    f[4 * i + 1] = lo[1];
    f[4 * i + 2] = hi[0];
    f[4 * i + 3] = hi[1];
  }
}

// WSPLIT (few rows, e.g. batch-1 decode: 32 rows would occupy 8 CUs): one row per block, the 4
// waves take interleaved 64-key blocks of the row's range and merge their (m, l, acc) through LDS,
// so a row's serial key loop is 4x shorter without a second launch.
// KV is the cache's element type: T itself, or uint8_t for an unscaled e4m3 cache (same structure and
// the same fp32 arithmetic in the same order; only the row loads differ).  The e4m3 kernels start their
// sums from -0, the additive identity that keeps a stored -0 (byte 0x80) a -0 when it is all a row
// attends to; the 16-bit kernels keep their +0 start, and every other result is the same either way.
template <typename KV>
constexpr float kSumStart = sizeof(KV) == 1 ? -0.f : 0.f;

// acc / l rounded to T.  For the e4m3 kernels the product first settles in a register: hipcc otherwise folds
// the multiply and the fp16 conversion into one v_fma_mixlo_f16 (x * y + 0), and the + 0 turns a -0 into +0.
// The scaled e4m3 kernels (KS) are held bit for bit to the 16-bit kernel over the dequantised cache, so they
// convert as that kernel does: in fp16 the fold is a single rounding of acc * inv, the settled product a
// double one (fp32, then fp16), and the two differ in about one element in 10^5.
template <typename T, typename KV, bool KS = false>
__device__ __forceinline__ T normalised(float acc, float inv) {
  float r = acc * inv;
  if constexpr (sizeof(KV) == 1 && !KS) asm volatile("" : "+v"(r));
  return from_f32<T>(r);
}

// Scaled e4m3 cache (ops/kv8.py): one byte e + 127 per (b, kv head, key) row of K and of V; the row's
// values are its bytes times 2^e.  Strides in bytes over b, h, s.
struct KVScales {
  const uint8_t *k, *v;
  int64_t ksb, ksh, kss, vsb, vsh, vss;
};
struct NoScales {};

// Position mode (POS): no mask; row (b, hq, t) attends keys 0 .. n-1 with n = clamp(pos[b, t] + 1, 0, S), so a
// ragged batch needs no [B, 1, T, S] mask tensor and a bad position never reads outside the cache.  Strides in
// elements over b, t.
struct RowPos {
  const int64_t* pos;
  int64_t sb, st;
};
struct NoPos {};

// Paged mode (PAGED, a position mode): k / v are pools [Hkv, R + 1, D] of pages of 2^lg_page rows and key j of
// sequence b sits at pool row table[b, j >> lg_page] * 2^lg_page + (j & (2^lg_page - 1)) (ops/kv_pages.py; the
// scale bytes at the same row).  Strides of the int64 table in elements over b and the page index.  A key whose
// table entry is outside [0, num_pages) is invalid exactly like a masked key: nothing of it is loaded, so a bad
// entry never reads outside the pool, and a 64-key block without a valid key is skipped before any K / V traffic.
// The row's live range, its split over gridDim.y, the softmax and the combine are the position mode's.
struct PageMap {
  const int64_t* table;
  int64_t sb, sp;
  int lg_page, num_pages;
};
struct PagedPos : RowPos {
  PageMap pg;
};
// Window mode (WIN, a position mode, static or paged): the row attends its last `window` >= 1 keys only, itself
// included: key j iff p - window < j <= p (the Mistral / HF convention, ops/kv_rows.py window_mask), so the live range
// is [lo, n) with lo = clamp(p + 1 - window, 0, n): max(0, n - window) for a position inside the cache, where
// window >= S is the position mode.
struct WinPos : RowPos {
  int window;
};
struct WinPagedPos : PagedPos {
  int window;
};
template <bool POS, bool PAGED, bool WIN = false>
using Selector = std::conditional_t<WIN, std::conditional_t<PAGED, WinPagedPos, WinPos>,
                                    std::conditional_t<PAGED, PagedPos, std::conditional_t<POS, RowPos, NoPos>>>;

// KS (with KV = uint8_t): the cache is the scaled one.  The lane that owns key j loads that key's two scale
// bytes (consecutive bytes across the lanes of a 64-key block) and forms 2^e as byte << 23; the score is
// dot * 2^ek and V is accumulated with p * 2^ev in place of p, while l keeps the unscaled p.  Both products
// are exact, and scaling an operand by a power of two commutes with the rounding of every fmaf, so the
// result equals the 16-bit kernel's over the dequantised cache bit for bit.  The claim excludes fp32
// subnormals and overflow (a partial sum below 2^-126 or above 2^127 after scaling rounds differently), and
// an all-zero result (the sums start from the e4m3 kernels' -0).  A contraction of dot * 2^ek into the following subtraction
// (v_fma) is harmless for the same reason: the product it skips rounding is exact.
//
// POS: the host still picks the grid from the capacity S (under a hipGraph it cannot know the positions), and
// the kernel splits the row's live range 0 .. n-1 over the gridDim.y splits itself: chunk_row =
// round_up(ceil(n / nsplit), 64), split s takes [s * chunk_row, min(n, (s + 1) * chunk_row)).  Every split of
// a row then has work unless n is tiny; an empty one stores m = -inf, l = 0, which the combine kernel skips.
// With n = S and the host's nsplit, chunk_row is the host's chunk, so the result equals the mask kernel's
// under an all-true mask bit for bit.  `mask`, `chunk` and `causal` are unused.  All three position kernels
// round acc / l as the 16-bit kernel does (`normalised` with its scaled-cache form), so both e4m3 ones equal
// the 16-bit one over the dequantised cache bit for bit, with the exclusions above (a zero result's sign included).
//
// WIN: the same split over the row's window, from its first 64-key block on: lo64 = lo & ~63, chunk_row =
// round_up(ceil((n - lo64) / nsplit), 64), split s takes [lo64 + s * chunk_row, min(n, lo64 + (s + 1) * chunk_row)),
// and a key is valid iff lo <= j < j_end.  A row at position 32767 under a window of 4096 then costs what a row at
// 4095 costs.  On a paged cache the test stands before the table lookup: an entry below the window is never loaded
// and may hold anything (PageTable.trim hands such pages back).  With lo = 0 all of this is the position mode's, bit
// for bit; everything after `valid` is untouched.
template <typename T, typename KV, int D, bool WSPLIT, bool KS = false, bool POS = false, bool PAGED = false,
          bool WIN = false>
__global__ __launch_bounds__(256) void decode_attn_kernel(
    const T* __restrict__ q, const KV* __restrict__ k, const KV* __restrict__ v, const uint8_t* __restrict__ mask,
    T* __restrict__ o, float* __restrict__ ws_acc, float* __restrict__ ws_ml, int B, int Hq, int Hkv, int Tq, int S,
    int64_t qsb, int64_t qsh, int64_t qst, int64_t ksb, int64_t ksh, int64_t kss, int64_t vsb, int64_t vsh,
    int64_t vss, int64_t msb, int64_t msh, int64_t mst, int64_t mss, int chunk, int causal, float scale,
    std::conditional_t<KS, KVScales, NoScales> sc, Selector<POS, PAGED, WIN> rp) {
  static_assert(!KS || sizeof(KV) == 1, "scales belong to an e4m3 cache");
  static_assert(!PAGED || POS, "a paged cache is read by positions");
  static_assert(!WIN || POS, "a window hangs on a row's position");
  constexpr int DPL = D / 64;          // output dims per lane after the final reduce-scatter
  constexpr bool kE4M3 = sizeof(KV) == 1;
  constexpr int NV = 16 / sizeof(KV);  // elements per 16-byte load
  __shared__ float q_lds[kRowsPerBlock][D];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int rows = B * Tq * Hq;
  const int row = WSPLIT ? blockIdx.x : blockIdx.x * kRowsPerBlock + w;
  if (!WSPLIT && row >= rows) return;  // whole wave exits together (no block-level sync below)
  const int hq = row % Hq;
  const int t = (row / Hq) % Tq;
  const int b = row / (Hq * Tq);
  const int hk = hq / (Hq / Hkv);
  const int split = blockIdx.y;
  int j_begin = split * chunk;
  int j_end = min(S, j_begin + chunk);
  if (causal) j_end = min(j_end, t + 1);
  [[maybe_unused]] int lo = 0;  // WIN: the row's first live key
  if constexpr (POS) {
    // a wave owns one row: its position is one scalar load (the row index made uniform for the compiler)
    const int urow = __builtin_amdgcn_readfirstlane(row);
    const int64_t p = rp.pos[(urow / (Hq * Tq)) * rp.sb + ((urow / Hq) % Tq) * rp.st];
    const int n = (int)min(max(p + 1, (int64_t)0), (int64_t)S);
    const int nsplit = gridDim.y;
    const int chunk_row = ((n + nsplit - 1) / nsplit + 63) / 64 * 64;
    j_begin = split * chunk_row;
    j_end = min(n, j_begin + chunk_row);
    if constexpr (WIN) {  // wave-uniform, as n is
      lo = (int)min(max(p + 1 - (int64_t)rp.window, (int64_t)0), (int64_t)n);
      const int lo64 = lo & ~63;
      const int chunk_win = ((n - lo64 + nsplit - 1) / nsplit + 63) / 64 * 64;
      j_begin = lo64 + split * chunk_win;
      j_end = min(n, j_begin + chunk_win);
    }
  }

  // scaled q row -> wave-private LDS (read back as broadcasts)
  const T* qrow = q + b * qsb + hq * qsh + t * qst;
  for (int d = lane; d < D; d += 64) q_lds[w][d] = to_f32(qrow[d]) * scale;
  __builtin_amdgcn_wave_barrier();
  const KV* kbase = k + b * ksb + hk * ksh;
  const KV* vbase = v + b * vsb + hk * vsh;
  [[maybe_unused]] const uint8_t* mrow = mask ? mask + b * msb + hq * msh + t * mst : nullptr;
  [[maybe_unused]] const uint8_t* ksrow = nullptr;
  [[maybe_unused]] const uint8_t* vsrow = nullptr;
  if constexpr (KS) {
    ksrow = sc.k + b * sc.ksb + hk * sc.ksh;
    vsrow = sc.v + b * sc.vsb + hk * sc.vsh;
  }

  // every lane owns one key per 64-key block: QK and PV are both lane-parallel; the per-lane
  // partial outputs acc[D] are reduce-scattered across the wave once at the end.
  float m = -INFINITY, l = 0.f;
  float acc[D];
#pragma unroll
  for (int i = 0; i < D; ++i) acc[i] = kSumStart<KV>;

  for (int j0 = j_begin + (WSPLIT ? w * 64 : 0); j0 < j_end; j0 += (WSPLIT ? kRowsPerBlock * 64 : 64)) {
    const int j = j0 + lane;
    bool valid = j < j_end;
    if constexpr (WIN) valid = valid && j >= lo;
    if constexpr (!POS) {
      if (valid && mrow) valid = mrow[(int64_t)j * mss] != 0;
    }
    [[maybe_unused]] int64_t r = j;  // the key's row in its cache
    if constexpr (PAGED) {
      if (valid) {  // one table entry per lane: j < j_end <= S = (table entries per sequence) << lg_page
        const int64_t pid = rp.pg.table[b * rp.pg.sb + (int64_t)(j >> rp.pg.lg_page) * rp.pg.sp];
        valid = pid >= 0 && pid < rp.pg.num_pages;
        r = (pid << rp.pg.lg_page) + (j & ((1 << rp.pg.lg_page) - 1));
      }
    }
    if (!__any(valid)) continue;  // fully masked block: no K/V traffic
    float s = -INFINITY;
    // scale bytes of key j's K row and V row: loaded ahead of the K row, turned into 2^e where first used
    [[maybe_unused]] uint32_t kb = 127, vb = 127;
    if (valid) {
      if constexpr (KS) {
        kb = ksrow[(PAGED ? r : (int64_t)j) * sc.kss];
        vb = vsrow[(PAGED ? r : (int64_t)j) * sc.vss];
      }
      const KV* krow = kbase + (PAGED ? r : (int64_t)j) * kss;
      float dot = 0.f;
#pragma unroll
      for (int d = 0; d < D; d += NV) {
        if constexpr (kE4M3) {
          float x[NV];
          load16_e4m3(krow + d, x);
#pragma unroll
          for (int e = 0; e < NV; ++e) dot = fmaf(q_lds[w][d + e], x[e], dot);
        } else {
          Vec16<T> x = load16(krow + d);
#pragma unroll
          for (int e = 0; e < NV; ++e) dot = fmaf(q_lds[w][d + e], to_f32(x.v[e]), dot);
        }
      }
      s = dot;
      if constexpr (KS) s = dot * __uint_as_float(kb << 23);
    }
    const float m_new = fmaxf(m, wave_max(s));
    const float p = valid ? __expf(s - m_new) : 0.f;
    const float corr = __expf(m - m_new);  // m = -inf on the first block -> 0
    l = l * corr + wave_sum(p);
    m = m_new;
    if (valid) {
      const KV* vrow = vbase + (PAGED ? r : (int64_t)j) * vss;
      const float pv = KS ? p * __uint_as_float(vb << 23) : p;
#pragma unroll
      for (int d = 0; d < D; d += NV) {
        if constexpr (kE4M3) {
          float x[NV];
          load16_e4m3(vrow + d, x);
#pragma unroll
          for (int e = 0; e < NV; ++e) acc[d + e] = fmaf(pv, x[e], acc[d + e] * corr);
        } else {
          Vec16<T> x = load16(vrow + d);
#pragma unroll
          for (int e = 0; e < NV; ++e) acc[d + e] = fmaf(pv, to_f32(x.v[e]), acc[d + e] * corr);
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < D; ++i) acc[i] *= corr;
    }
  }

  // recursive-halving reduce-scatter over the 64 lanes: lane ends with dims [lane*DPL, lane*DPL+DPL)
#pragma unroll
  for (int off = 32, n = D; off >= 1; off >>= 1, n >>= 1) {
    const bool upper = (lane & off) != 0;
    const int half = n >> 1;
#pragma unroll
    for (int i = 0; i < half; ++i) {
      const float give = upper ? acc[i] : acc[half + i];
      const float keep = upper ? acc[half + i] : acc[i];
      acc[i] = keep + __shfl_xor(give, off, 64);
    }
  }

  if constexpr (WSPLIT) {
    __shared__ float c_acc[kRowsPerBlock][D];
    __shared__ float c_ml[kRowsPerBlock][2];
#pragma unroll
    for (int i = 0; i < DPL; ++i) c_acc[w][lane * DPL + i] = acc[i];
    if (lane == 0) {
      c_ml[w][0] = m;
      c_ml[w][1] = l;
    }
    __syncthreads();
    if (w != 0) return;
    float M = -INFINITY;
#pragma unroll
    for (int u = 0; u < kRowsPerBlock; ++u) M = fmaxf(M, c_ml[u][0]);
    float L = 0.f;
#pragma unroll
    for (int i = 0; i < DPL; ++i) acc[i] = kSumStart<KV>;
#pragma unroll
    for (int u = 0; u < kRowsPerBlock; ++u) {
      const float c = c_ml[u][0] == -INFINITY ? 0.f : __expf(c_ml[u][0] - M);
      L = fmaf(c, c_ml[u][1], L);
#pragma unroll
      for (int i = 0; i < DPL; ++i) acc[i] = fmaf(c, c_acc[u][lane * DPL + i], acc[i]);
    }
    m = M;
    l = L;
  }

  if (gridDim.y == 1) {
    const float inv = 1.f / l;  // fully masked row -> 0 * inf = nan, like PyTorch SDPA
    T* orow = o + (((int64_t)b * Hq + hq) * Tq + t) * D + lane * DPL;  // o is [B, Hq, Tq, D]
#pragma unroll
    for (int i = 0; i < DPL; ++i) orow[i] = normalised<T, KV, KS || POS>(acc[i], inv);
  } else {
    float* wa = ws_acc + ((int64_t)split * rows + row) * D + lane * DPL;
#pragma unroll
    for (int i = 0; i < DPL; ++i) wa[i] = acc[i];
    if (lane == 0) {
      ws_ml[((int64_t)split * rows + row) * 2 + 0] = m;
      ws_ml[((int64_t)split * rows + row) * 2 + 1] = l;
    }
  }
}

template <typename T, typename KV, int D, bool KS = false>
__global__ __launch_bounds__(64) void decode_attn_combine_kernel(const float* __restrict__ ws_acc,
                                                                 const float* __restrict__ ws_ml, T* __restrict__ o,
                                                                 int rows, int nsplit, int Hq, int Tq) {
  constexpr int DPL = D / 64;
  const int row = blockIdx.x, lane = threadIdx.x;
  const int hq = row % Hq, t = (row / Hq) % Tq, b = row / (Hq * Tq);
  float M = -INFINITY;
  for (int s = 0; s < nsplit; ++s) M = fmaxf(M, ws_ml[((int64_t)s * rows + row) * 2]);
  float L = 0.f, acc[DPL];
#pragma unroll
  for (int i = 0; i < DPL; ++i) acc[i] = kSumStart<KV>;
  for (int s = 0; s < nsplit; ++s) {
    const float ms = ws_ml[((int64_t)s * rows + row) * 2];
    if (ms == -INFINITY) continue;
    const float c = __expf(ms - M);
    L += c * ws_ml[((int64_t)s * rows + row) * 2 + 1];
    const float* wa = ws_acc + ((int64_t)s * rows + row) * D + lane * DPL;
#pragma unroll
    for (int i = 0; i < DPL; ++i) acc[i] = fmaf(c, wa[i], acc[i]);
  }
  const float inv = 1.f / L;
  T* orow = o + (((int64_t)b * Hq + hq) * Tq + t) * D + lane * DPL;
#pragma unroll
  for (int i = 0; i < DPL; ++i) orow[i] = normalised<T, KV, KS>(acc[i], inv);
}

template <typename T, typename KV, int D, bool KS = false, bool POS = false, bool PAGED = false, bool WIN = false>
int launch(const void* q, const void* k, const void* v, const void* mask, void* o, void* ws_acc, void* ws_ml, int B,
           int Hq, int Hkv, int Tq, int S, const int64_t* st, int chunk, int nsplit, int causal, float scale,
           int wsplit, hipStream_t stream, std::conditional_t<KS, KVScales, NoScales> sc = {},
           Selector<POS, PAGED, WIN> rp = {}) {
  const int rows = B * Tq * Hq;
  if (wsplit) {
    hipLaunchKernelGGL((decode_attn_kernel<T, KV, D, true, KS, POS, PAGED, WIN>), dim3(rows, nsplit), dim3(256), 0, stream, (const T*)q,
                       (const KV*)k, (const KV*)v, (const uint8_t*)mask, (T*)o, (float*)ws_acc, (float*)ws_ml, B, Hq, Hkv,
                       Tq, S, st[0], st[1], st[2], st[3], st[4], st[5], st[6], st[7], st[8], st[9], st[10], st[11],
                       st[12], chunk, causal, scale, sc, rp);
  } else {
    dim3 grid((rows + kRowsPerBlock - 1) / kRowsPerBlock, nsplit);
    hipLaunchKernelGGL((decode_attn_kernel<T, KV, D, false, KS, POS, PAGED, WIN>), grid, dim3(256), 0, stream, (const T*)q, (const KV*)k,
                       (const KV*)v, (const uint8_t*)mask, (T*)o, (float*)ws_acc, (float*)ws_ml, B, Hq, Hkv, Tq, S,
                       st[0], st[1], st[2], st[3], st[4], st[5], st[6], st[7], st[8], st[9], st[10], st[11], st[12],
                       chunk, causal, scale, sc, rp);
  }
  if (nsplit > 1)
    hipLaunchKernelGGL((decode_attn_combine_kernel<T, KV, D, KS || POS>), dim3(rows), dim3(64), 0, stream, (const float*)ws_acc,
                       (const float*)ws_ml, (T*)o, rows, nsplit, Hq, Tq);
  return (int)hipGetLastError();
}

// `launch` for q / o of `dtype` and head dim D; KV = void: the cache holds q's type.  `a`: launch's arguments.
template <typename KV, bool KS = false, bool POS = false, bool PAGED = false, bool WIN = false, typename... A>
int dispatch(int dtype, int D, A... a) {
  using B16 = __hip_bfloat16;
  constexpr bool kSame = std::is_void_v<KV>;
  if (dtype == kBF16 && D == 64) return launch<B16, std::conditional_t<kSame, B16, KV>, 64, KS, POS, PAGED, WIN>(a...);
  if (dtype == kBF16 && D == 128) return launch<B16, std::conditional_t<kSame, B16, KV>, 128, KS, POS, PAGED, WIN>(a...);
  if (dtype == kF16 && D == 64) return launch<__half, std::conditional_t<kSame, __half, KV>, 64, KS, POS, PAGED, WIN>(a...);
  if (dtype == kF16 && D == 128) return launch<__half, std::conditional_t<kSame, __half, KV>, 128, KS, POS, PAGED, WIN>(a...);
  return (int)hipErrorInvalidValue;
}

// what every entry requires of its sizes
bool sizes_ok(int Hq, int Hkv, int chunk, int nsplit) { return Hkv > 0 && Hq % Hkv == 0 && chunk > 0 && nsplit > 0; }

// an e4m3 cache is read with 16-byte loads: k / v strides (strides[3..8], bytes) and bases are multiples of 16
bool e4m3_cache_ok(const void* k, const void* v, const int64_t* strides) {
  for (int i = 3; i < 9; ++i)
    if (strides[i] % 16) return false;
  return (((uintptr_t)k | (uintptr_t)v) % 16) == 0;
}

// The host side of every entry: the checks, then the kernels' records out of `strides`, which holds (elements;
// 0 for broadcast dims; head dim contiguous)
//   q b,h,t | k b,h,s | v b,h,s | the selector's | with KS: k scale b,h,s | v scale b,h,s (bytes),
// where the selector `sel` is the bool mask (strides b,h,t,s; may be null) or, with POS, the int64 positions
// [B, Tq] (strides b,t; see RowPos).  KV = void: the cache holds q's type; uint8_t: e4m3.
// PAGED: k / v (and the scales) are pools, their b strides 0 and S the logical capacity, a multiple of the page;
// `table` int64 [B, S >> lg_page] with its strides b,p last in `strides`; see PageMap.
// WIN: `window` >= 1 keys per row; anything less is refused and launches nothing.
template <typename KV, bool KS, bool POS, bool PAGED = false, bool WIN = false>
int decode_entry(int dtype, const void* q, const void* k, const void* v, const void* k_scale, const void* v_scale,
                 const void* sel, void* o, void* ws_acc, void* ws_ml, int B, int Hq, int Hkv, int Tq, int S, int D,
                 const int64_t* strides, int chunk, int nsplit, int causal, float scale, int wsplit, void* stream,
                 const void* table = nullptr, int lg_page = 0, int num_pages = 0, int window = 0) {
  constexpr int kSel = POS ? 2 : 4;  // strides of the selector; the scales' follow them
  if (!sizes_ok(Hq, Hkv, POS ? 64 : chunk, nsplit)) return (int)hipErrorInvalidValue;  // POS: no chunk to check
  if (nsplit > 1 && (ws_acc == nullptr || ws_ml == nullptr)) return (int)hipErrorInvalidValue;
  if constexpr (std::is_same_v<KV, uint8_t>)
    if (!e4m3_cache_ok(k, v, strides)) return (int)hipErrorInvalidValue;
  int64_t st[13] = {};  // the kernels' q, k, v and mask strides; without a mask its four stay 0
  for (int i = 0; i < (POS ? 9 : 13); ++i) st[i] = strides[i];
  std::conditional_t<KS, KVScales, NoScales> sc{};
  if constexpr (KS) {
    if (k_scale == nullptr || v_scale == nullptr) return (int)hipErrorInvalidValue;
    const int64_t* ss = strides + 9 + kSel;
    sc = KVScales{(const uint8_t*)k_scale, (const uint8_t*)v_scale, ss[0], ss[1], ss[2], ss[3], ss[4], ss[5]};
  }
  Selector<POS, PAGED, WIN> rp{};
  if constexpr (WIN) {
    if (window < 1) return (int)hipErrorInvalidValue;
    rp.window = window;
  }
  if constexpr (POS) {
    if (sel == nullptr || S < 0) return (int)hipErrorInvalidValue;
    rp.pos = (const int64_t*)sel;
    rp.sb = strides[9];
    rp.st = strides[10];
  }
  if constexpr (PAGED) {
    if (table == nullptr || lg_page < 4 || lg_page > 24 || num_pages <= 0 || num_pages > (INT32_MAX >> lg_page) ||
        S % (1 << lg_page))
      return (int)hipErrorInvalidValue;
    const int64_t* ts = strides + 9 + kSel + (KS ? 6 : 0);
    rp.pg = PageMap{(const int64_t*)table, ts[0], ts[1], lg_page, num_pages};
  }
  return dispatch<KV, KS, POS, PAGED, WIN>(dtype, D, q, k, v, POS ? (const void*)nullptr : sel, o, ws_acc, ws_ml, B, Hq, Hkv, Tq, S,
                               (const int64_t*)st, chunk, nsplit, causal, scale, wsplit, (hipStream_t)stream, sc, rp);
}

}  // namespace
}  // namespace lta

// The mask entries; `strides` as decode_entry has them.
LTA_EXPORT int lta_decode_attn(int dtype, const void* q, const void* k, const void* v, const void* mask, void* o,
                               void* ws_acc, void* ws_ml, int B, int Hq, int Hkv, int Tq, int S, int D,
                               const int64_t* strides, int chunk, int nsplit, int causal, float scale, int wsplit,
                               void* stream) {
  return lta::decode_entry<void, false, false>(dtype, q, k, v, nullptr, nullptr, mask, o, ws_acc, ws_ml, B, Hq, Hkv, Tq,
                                               S, D, strides, chunk, nsplit, causal, scale, wsplit, stream);
}

// The same launch over an unscaled OCP e4m3 cache: k / v are uint8 [B, Hkv, S, D] (strides in elements
// = bytes, multiples of 16, rows 16-byte aligned); `dtype` is q's and the output's.
LTA_EXPORT int lta_decode_attn_kv8(int dtype, const void* q, const void* k, const void* v, const void* mask, void* o,
                                   void* ws_acc, void* ws_ml, int B, int Hq, int Hkv, int Tq, int S, int D,
                                   const int64_t* strides, int chunk, int nsplit, int causal, float scale, int wsplit,
                                   void* stream) {
  return lta::decode_entry<uint8_t, false, false>(dtype, q, k, v, nullptr, nullptr, mask, o, ws_acc, ws_ml, B, Hq, Hkv,
                                                  Tq, S, D, strides, chunk, nsplit, causal, scale, wsplit, stream);
}

// The same launch over the scaled e4m3 cache of ops/kv8.py: k / v as for lta_decode_attn_kv8, k_scale / v_scale
// uint8 [B, Hkv, S, 1] holding e + 127 per row.
LTA_EXPORT int lta_decode_attn_kv8s(int dtype, const void* q, const void* k, const void* v, const void* k_scale,
                                    const void* v_scale, const void* mask, void* o, void* ws_acc, void* ws_ml, int B,
                                    int Hq, int Hkv, int Tq, int S, int D, const int64_t* strides, int chunk, int nsplit,
                                    int causal, float scale, int wsplit, void* stream) {
  return lta::decode_entry<uint8_t, true, false>(dtype, q, k, v, k_scale, v_scale, mask, o, ws_acc, ws_ml, B, Hq, Hkv,
                                                 Tq, S, D, strides, chunk, nsplit, causal, scale, wsplit, stream);
}

// The position entries: no mask and no causal flag; `pos` int64 [B, Tq] gives every row its key count (see
// RowPos).  `nsplit` is the host's split count for the capacity S; the kernel derives each row's own chunk from
// it and reads neither `chunk` nor `causal`, which go on as 0.
LTA_EXPORT int lta_decode_attn_pos(int dtype, const void* q, const void* k, const void* v, const void* pos, void* o,
                                   void* ws_acc, void* ws_ml, int B, int Hq, int Hkv, int Tq, int S, int D,
                                   const int64_t* strides, int nsplit, float scale, int wsplit, void* stream) {
  return lta::decode_entry<void, false, true>(dtype, q, k, v, nullptr, nullptr, pos, o, ws_acc, ws_ml, B, Hq, Hkv, Tq, S,
                                              D, strides, 0, nsplit, 0, scale, wsplit, stream);
}

LTA_EXPORT int lta_decode_attn_kv8_pos(int dtype, const void* q, const void* k, const void* v, const void* pos, void* o,
                                       void* ws_acc, void* ws_ml, int B, int Hq, int Hkv, int Tq, int S, int D,
                                       const int64_t* strides, int nsplit, float scale, int wsplit, void* stream) {
  return lta::decode_entry<uint8_t, false, true>(dtype, q, k, v, nullptr, nullptr, pos, o, ws_acc, ws_ml, B, Hq, Hkv, Tq,
                                                 S, D, strides, 0, nsplit, 0, scale, wsplit, stream);
}

LTA_EXPORT int lta_decode_attn_kv8s_pos(int dtype, const void* q, const void* k, const void* v, const void* k_scale,
                                        const void* v_scale, const void* pos, void* o, void* ws_acc, void* ws_ml, int B,
                                        int Hq, int Hkv, int Tq, int S, int D, const int64_t* strides, int nsplit,
                                        float scale, int wsplit, void* stream) {
  return lta::decode_entry<uint8_t, true, true>(dtype, q, k, v, k_scale, v_scale, pos, o, ws_acc, ws_ml, B, Hq, Hkv, Tq,
                                                S, D, strides, 0, nsplit, 0, scale, wsplit, stream);
}

// The paged entries: the position entries over a paged cache (ops/kv_pages.py).  k / v are pools [Hkv, R + 1, D]
// (strides b = 0, h, row), `table` int64 [B, S >> lg_page], S the logical capacity; see PageMap.
LTA_EXPORT int lta_decode_attn_paged(int dtype, const void* q, const void* k, const void* v, const void* pos, void* o,
                                     void* ws_acc, void* ws_ml, int B, int Hq, int Hkv, int Tq, int S, int D,
                                     const int64_t* strides, int nsplit, float scale, int wsplit, const void* table,
                                     int lg_page, int num_pages, void* stream) {
  return lta::decode_entry<void, false, true, true>(dtype, q, k, v, nullptr, nullptr, pos, o, ws_acc, ws_ml, B, Hq, Hkv,
                                                    Tq, S, D, strides, 0, nsplit, 0, scale, wsplit, stream, table,
                                                    lg_page, num_pages);
}

LTA_EXPORT int lta_decode_attn_kv8_paged(int dtype, const void* q, const void* k, const void* v, const void* pos,
                                         void* o, void* ws_acc, void* ws_ml, int B, int Hq, int Hkv, int Tq, int S,
                                         int D, const int64_t* strides, int nsplit, float scale, int wsplit,
                                         const void* table, int lg_page, int num_pages, void* stream) {
  return lta::decode_entry<uint8_t, false, true, true>(dtype, q, k, v, nullptr, nullptr, pos, o, ws_acc, ws_ml, B, Hq,
                                                       Hkv, Tq, S, D, strides, 0, nsplit, 0, scale, wsplit, stream,
                                                       table, lg_page, num_pages);
}

LTA_EXPORT int lta_decode_attn_kv8s_paged(int dtype, const void* q, const void* k, const void* v, const void* k_scale,
                                          const void* v_scale, const void* pos, void* o, void* ws_acc, void* ws_ml,
                                          int B, int Hq, int Hkv, int Tq, int S, int D, const int64_t* strides,
                                          int nsplit, float scale, int wsplit, const void* table, int lg_page,
                                          int num_pages, void* stream) {
  return lta::decode_entry<uint8_t, true, true, true>(dtype, q, k, v, k_scale, v_scale, pos, o, ws_acc, ws_ml, B, Hq,
                                                      Hkv, Tq, S, D, strides, 0, nsplit, 0, scale, wsplit, stream,
                                                      table, lg_page, num_pages);
}

// The window entries: the six position / paged entries with one trailing `window` (keys per row, >= 1; see WinPos).
// window < 1 returns hipErrorInvalidValue and launches nothing.
LTA_EXPORT int lta_decode_attn_pos_win(int dtype, const void* q, const void* k, const void* v, const void* pos, void* o,
                                       void* ws_acc, void* ws_ml, int B, int Hq, int Hkv, int Tq, int S, int D,
                                       const int64_t* strides, int nsplit, float scale, int wsplit, void* stream,
                                       int window) {
  return lta::decode_entry<void, false, true, false, true>(dtype, q, k, v, nullptr, nullptr, pos, o, ws_acc, ws_ml, B, Hq,
                                                           Hkv, Tq, S, D, strides, 0, nsplit, 0, scale, wsplit, stream,
                                                           nullptr, 0, 0, window);
}

LTA_EXPORT int lta_decode_attn_kv8_pos_win(int dtype, const void* q, const void* k, const void* v, const void* pos,
                                           void* o, void* ws_acc, void* ws_ml, int B, int Hq, int Hkv, int Tq, int S,
                                           int D, const int64_t* strides, int nsplit, float scale, int wsplit,
                                           void* stream, int window) {
  return lta::decode_entry<uint8_t, false, true, false, true>(dtype, q, k, v, nullptr, nullptr, pos, o, ws_acc, ws_ml, B,
                                                              Hq, Hkv, Tq, S, D, strides, 0, nsplit, 0, scale, wsplit,
                                                              stream, nullptr, 0, 0, window);
}

LTA_EXPORT int lta_decode_attn_kv8s_pos_win(int dtype, const void* q, const void* k, const void* v, const void* k_scale,
                                            const void* v_scale, const void* pos, void* o, void* ws_acc, void* ws_ml,
                                            int B, int Hq, int Hkv, int Tq, int S, int D, const int64_t* strides,
                                            int nsplit, float scale, int wsplit, void* stream, int window) {
  return lta::decode_entry<uint8_t, true, true, false, true>(dtype, q, k, v, k_scale, v_scale, pos, o, ws_acc, ws_ml, B,
                                                             Hq, Hkv, Tq, S, D, strides, 0, nsplit, 0, scale, wsplit,
                                                             stream, nullptr, 0, 0, window);
}

LTA_EXPORT int lta_decode_attn_paged_win(int dtype, const void* q, const void* k, const void* v, const void* pos,
                                         void* o, void* ws_acc, void* ws_ml, int B, int Hq, int Hkv, int Tq, int S,
                                         int D, const int64_t* strides, int nsplit, float scale, int wsplit,
                                         const void* table, int lg_page, int num_pages, void* stream, int window) {
  return lta::decode_entry<void, false, true, true, true>(dtype, q, k, v, nullptr, nullptr, pos, o, ws_acc, ws_ml, B, Hq,
                                                          Hkv, Tq, S, D, strides, 0, nsplit, 0, scale, wsplit, stream,
                                                          table, lg_page, num_pages, window);
}

LTA_EXPORT int lta_decode_attn_kv8_paged_win(int dtype, const void* q, const void* k, const void* v, const void* pos,
                                             void* o, void* ws_acc, void* ws_ml, int B, int Hq, int Hkv, int Tq, int S,
                                             int D, const int64_t* strides, int nsplit, float scale, int wsplit,
                                             const void* table, int lg_page, int num_pages, void* stream, int window) {
  return lta::decode_entry<uint8_t, false, true, true, true>(dtype, q, k, v, nullptr, nullptr, pos, o, ws_acc, ws_ml, B,
                                                             Hq, Hkv, Tq, S, D, strides, 0, nsplit, 0, scale, wsplit,
                                                             stream, table, lg_page, num_pages, window);
}

LTA_EXPORT int lta_decode_attn_kv8s_paged_win(int dtype, const void* q, const void* k, const void* v,
                                              const void* k_scale, const void* v_scale, const void* pos, void* o,
                                              void* ws_acc, void* ws_ml, int B, int Hq, int Hkv, int Tq, int S, int D,
                                              const int64_t* strides, int nsplit, float scale, int wsplit,
                                              const void* table, int lg_page, int num_pages, void* stream, int window) {
  return lta::decode_entry<uint8_t, true, true, true, true>(dtype, q, k, v, k_scale, v_scale, pos, o, ws_acc, ws_ml, B,
                                                            Hq, Hkv, Tq, S, D, strides, 0, nsplit, 0, scale, wsplit,
                                                            stream, table, lg_page, num_pages, window);
}
