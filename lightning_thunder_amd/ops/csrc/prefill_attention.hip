// Prefill attention by positions (K3p): the flash forward for query rows that sit at positions of a KV cache.
// Row (b, hq, t) attends keys 0 .. n-1 with n = clamp(pos[b, t] + 1, 0, S): what the masked v1 forward
// (attention_fwd.hip, EX = kExMask) computes under the mask `arange(S) <= pos[b, t]`, without the fp32 mask image
// [B, 1, T, S], without the sweep over the key tiles no row of the workgroup can see, and with the cache read as it
// is stored: 16-bit or OCP e4m3 bytes (with or without row scales), static [B, Hkv, S, D] or paged pools
// [Hkv, R + 1, D] behind a block table.  The counterpart of decode_attn_kernel's position and paged modes for more
// than 16 query rows; inference only (no mask pointer, no causal flag, no dropout, no LSE).
//
// The structure is the v1 forward's: 4 waves and 128 query rows per workgroup, grid (B * Hq, query tiles) with the
// last query tile first, 64-key tiles staged global -> registers -> LDS with the next tile's loads issued before the
// current tile's math, swapped S^T = K Q^T, lane-local online softmax, P^T straight into the PV MFMA.  The fp32
// arithmetic and its order are v1's, so the result equals that kernel's under the equivalent mask bit for bit.
//
// What differs:
//  * every lane takes its row's key count n from pos; the tile loop runs to ceil(nmax / 64) with nmax the workgroup's
//    largest n (wave reduce, then LDS), so the host sizes the grid from Tq alone and never reads pos or the table;
//  * a key at or past nmax, and on a paged cache a key whose table entry is outside [0, num_pages), is dead: nothing of
//    it is loaded, zeros are staged and its score is -inf (the staging threads pass a flag per key through LDS);
//  * e4m3 staging: a thread loads 16 bytes (16 elements), unpacks them with v_cvt_pk_f32_fp8, with KS multiplies by
//    the row's 2^e (scale byte << 23), rounds to T (exact: ops/kv8.py) and writes 32 bytes to LDS.  The LDS tile is
//    then the dequantised cache's bit for bit and everything after staging is the 16-bit instantiation's code.
//  * WIN (a sliding window of `window` >= 1 keys per row, itself included: key j iff p - window < j <= p, the Mistral /
//    HF convention): every lane also has its row's first live key lo = clamp(p + 1 - window, 0, n), which is
//    max(0, n - window) for a position inside the cache.  The tile loop starts at
//    floor(lo_min / 64) with lo_min the workgroup's smallest lo over rows with n > 0 (rows with n = 0, those >= Tq of the
//    last query tile among them, take no part); a key below lo_min is dead like one at or past nmax (zeros staged,
//    nothing loaded, on a paged cache no table lookup: PageTable.trim may have taken the page back); the score stage
//    sets -inf for j < lo of its row, and a tile needs no per-key select only if it lies in [lo_high, n_low) with
//    lo_high the wave's largest lo.  A skipped leading tile would have left m = -inf, l = 0 and O = 0, so the result is
//    still the masked v1 forward's bit for bit.
// No split over keys: 17 .. 128 rows at batch 1 fill Hq workgroups, as the masked launch this replaces does.
#include <type_traits>

#include "attention.h"

using namespace lta;
using namespace lta::attn;

namespace {

constexpr int kBM = 128;  // queries per workgroup
constexpr int kBN = 64;   // keys per tile
constexpr int kThreads = 256;

// The argument records of decode_attention.hip, duplicated here so that that file and its instantiations stay exactly
// what they were (they are private to each translation unit).
// Scaled e4m3 cache (ops/kv8.py): one byte e + 127 per (b, kv head, key) row of K and of V.  Strides in bytes.
struct KVScales {
  const uint8_t *k, *v;
  int64_t ksb, ksh, kss, vsb, vsh, vss;
};
struct NoScales {};
// int64 positions [B, Tq]; strides in elements over b, t.
struct RowPos {
  const int64_t* pos;
  int64_t sb, st;
};
// Paged cache: key j of sequence b sits at pool row table[b, j >> lg_page] * 2^lg_page + (j & (2^lg_page - 1)).
struct PageMap {
  const int64_t* table;
  int64_t sb, sp;
  int lg_page, num_pages;
};
struct NoPages {};
// Sliding window (WIN): `window` >= 1 keys per row, carried behind the page map so that the kernels without a window
// keep their argument lists.
struct WinPageMap : PageMap {
  int window;
};
struct WinNoPages {
  int window;
};
template <bool PAGED, bool WIN>
using Pages = std::conditional_t<WIN, std::conditional_t<PAGED, WinPageMap, WinNoPages>,
                                 std::conditional_t<PAGED, PageMap, NoPages>>;

// Element strides (batch, head, token / key row) of Q, K, V and O; head dim contiguous.
struct Strides {
  int64_t qb, qh, qt, kb, kh, kt, vb, vh, vt, ob, oh, ot;
};

template <int D, int ESZ> struct Cfg {
  static constexpr int KSTR = D + 8;                 // K tile row stride (16-bit elements), as v1
  static constexpr int VSTR = D + 32;                // V tile row stride
  static constexpr int EPC = 16 / ESZ;               // cache elements per 16-byte chunk
  static constexpr int CH = D / EPC;                 // chunks per row
  static constexpr int LOADS = kBN * CH / kThreads;  // chunks per thread per tile
  static constexpr int KSTEPS = D / 16;              // MFMA k-steps over D
  static constexpr int DT = D / 32;                  // 32-wide d tiles
};

// 16 e4m3 bytes as fp32 (OCP e4m3 on gfx950; exact), as decode_attention.hip load16_e4m3 unpacks them
__device__ __forceinline__ void unpack16_e4m3(const uint4& x, float (&f)[16]) {
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

template <typename T, typename KV, int D, bool KS, bool PAGED, bool WIN = false>
__global__ __launch_bounds__(kThreads, 2) void prefill_attn_kernel(
    const T* __restrict__ Q, const KV* __restrict__ K, const KV* __restrict__ V, T* __restrict__ O, int Hq, int Hkv,
    int Tq, int S, float scale_log2, Strides sx, RowPos rp, std::conditional_t<KS, KVScales, NoScales> sc,
    Pages<PAGED, WIN> pg) {
  static_assert(!KS || sizeof(KV) == 1, "scales belong to an e4m3 cache");
  constexpr bool kE4M3 = sizeof(KV) == 1;
  using C = Cfg<D, sizeof(KV)>;
  using F = typename Frag<T>::type;
  __shared__ __attribute__((aligned(16))) short smem[kBN * C::KSTR + kBN * C::VSTR];
  __shared__ __attribute__((aligned(16))) uint8_t dead_lds[kBN];  // PAGED: 1 for a key of the tile that is not staged
  __shared__ int wave_n[kThreads / 64];
  __shared__ int wave_first[WIN ? kThreads / 64 : 1];  // WIN: every wave's smallest lo over its rows with n > 0
  short* Ks = smem;
  short* Vs = smem + kBN * C::KSTR;
  const __attribute__((address_space(3))) short* Vs3 = (const __attribute__((address_space(3))) short*)Vs;

  const int n_qt = (Tq + kBM - 1) / kBM;
  const int qt = n_qt - 1 - (int)blockIdx.y;
  const int bh = blockIdx.x;
  const int b = bh / Hq, hq = bh % Hq;
  const int hk = hq / (Hq / Hkv);
  const T* Qb = Q + b * sx.qb + hq * sx.qh;
  const KV* Kb = K + b * sx.kb + hk * sx.kh;
  const KV* Vb = V + b * sx.vb + hk * sx.vh;
  [[maybe_unused]] const uint8_t* ksrow = nullptr;
  [[maybe_unused]] const uint8_t* vsrow = nullptr;
  if constexpr (KS) {
    ksrow = sc.k + b * sc.ksb + hk * sc.ksh;
    vsrow = sc.v + b * sc.vsb + hk * sc.vsh;
  }

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5, g = lane >> 4, l16 = lane & 15;
  const int q0 = qt * kBM + wave * 32;
  const int qi = q0 + r;  // this lane's query

  // this row's key count, the wave's smallest (below it no key of a tile needs the select) and the workgroup's largest
  int n = 0;
  [[maybe_unused]] int lo = 0;  // WIN: this row's first live key
  if (qi < Tq) {
    const int64_t p = rp.pos[b * rp.sb + (int64_t)qi * rp.st];
    n = (int)min(max(p + 1, (int64_t)0), (int64_t)S);
    if constexpr (WIN) lo = (int)min(max(p + 1 - (int64_t)pg.window, (int64_t)0), (int64_t)n);
  }
  int nmx = n, nmn = n;
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) {  // lanes r and r + 32 hold the same row
    nmx = max(nmx, __shfl_xor(nmx, o, 64));
    nmn = min(nmn, __shfl_xor(nmn, o, 64));
  }
  const int n_low = __builtin_amdgcn_readfirstlane(nmn);
  if (lane == 0) wave_n[wave] = nmx;
  // WIN: the wave's largest lo (a tile below it needs the select) and its smallest over the rows that attend anything
  [[maybe_unused]] int lo_high = 0, lo_min = 0;
  if constexpr (WIN) {
    int lmx = lo, lmn = n > 0 ? lo : INT32_MAX;
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) {
      lmx = max(lmx, __shfl_xor(lmx, o, 64));
      lmn = min(lmn, __shfl_xor(lmn, o, 64));
    }
    lo_high = __builtin_amdgcn_readfirstlane(lmx);
    if (lane == 0) wave_first[wave] = lmn;
  }
  __syncthreads();
  const int nmax = __builtin_amdgcn_readfirstlane(max(max(wave_n[0], wave_n[1]), max(wave_n[2], wave_n[3])));
  const int n_tiles = (nmax + kBN - 1) / kBN;  // workgroup-uniform: the loop holds barriers
  int t_first = 0;
  if constexpr (WIN) {
    // INT32_MAX when no row attends: no tile either
    lo_min = __builtin_amdgcn_readfirstlane(min(min(wave_first[0], wave_first[1]), min(wave_first[2], wave_first[3])));
    t_first = lo_min / kBN;
  }

  // Q fragments (B operand of S^T = K Q^T): Q[qi][16s + 8h .. +7]
  F qf[C::KSTEPS];
  {
    const int qrow = min(qi, Tq - 1);
#pragma unroll
    for (int s = 0; s < C::KSTEPS; ++s) qf[s] = load_frag<F>(Qb + (int64_t)qrow * sx.qt + 16 * s + 8 * h);
  }

  f32x16 oacc[C::DT];
#pragma unroll
  for (int dt = 0; dt < C::DT; ++dt)
#pragma unroll
    for (int i = 0; i < 16; ++i) oacc[dt][i] = 0.f;
  float m = -INFINITY, l = 0.f;

  // register staging of one K/V tile: 16 bytes of K and of V per chunk, as the cache stores them
  uint4 kreg[C::LOADS], vreg[C::LOADS];
  [[maybe_unused]] uint32_t kexp[C::LOADS], vexp[C::LOADS];  // KS: the row's scale bytes
  [[maybe_unused]] int prow[C::LOADS];                       // PAGED: the chunk's pool row, -1 for a dead key
  [[maybe_unused]] unsigned live_bits = 0;                   // PAGED: bit c = chunk c of the staged tile is live
  // PAGED: the pool rows of tile t, one tile ahead of its loads (the table entry's latency is not in their way)
  auto tload = [&](int t) {
    if constexpr (PAGED) {
#pragma unroll
      for (int c = 0; c < C::LOADS; ++c) {
        const int key = t * kBN + (c * kThreads + tid) / C::CH;
        int pr = -1;
        bool inside = key < nmax;  // nmax <= S = (table entries per sequence) << lg_page
        if constexpr (WIN) inside = inside && key >= lo_min;  // below every row's window: no table lookup
        if (inside) {
          const int64_t pid = pg.table[b * pg.sb + (int64_t)(key >> pg.lg_page) * pg.sp];
          if (pid >= 0 && pid < pg.num_pages) pr = (int)(pid << pg.lg_page) + (key & ((1 << pg.lg_page) - 1));
        }
        prow[c] = pr;
      }
    }
  };
  auto gload = [&](int t) {
    if constexpr (PAGED) live_bits = 0;
#pragma unroll
    for (int c = 0; c < C::LOADS; ++c) {
      const int id = c * kThreads + tid;
      const int row = id / C::CH, ch = id % C::CH;
      int64_t kr = t * kBN + row;  // the key's row in its cache
      bool live = kr < nmax;
      if constexpr (WIN) live = live && kr >= lo_min;
      if constexpr (PAGED) {
        kr = prow[c];
        live = kr >= 0;
        live_bits |= (unsigned)live << c;
      }
      kreg[c] = make_uint4(0, 0, 0, 0);
      vreg[c] = make_uint4(0, 0, 0, 0);
      if constexpr (KS) kexp[c] = vexp[c] = 127;
      if (live) {  // a dead key is not loaded: zeros are staged
        kreg[c] = *reinterpret_cast<const uint4*>(Kb + kr * sx.kt + ch * C::EPC);
        vreg[c] = *reinterpret_cast<const uint4*>(Vb + kr * sx.vt + ch * C::EPC);
        if constexpr (KS) {
          kexp[c] = ksrow[kr * sc.kss];
          vexp[c] = vsrow[kr * sc.vss];
        }
      }
    }
  };
  auto lstore = [&]() {
#pragma unroll
    for (int c = 0; c < C::LOADS; ++c) {
      const int id = c * kThreads + tid;
      const int row = id / C::CH, ch = id % C::CH;
      if constexpr (kE4M3) {
        float kf[16], vf[16];
        unpack16_e4m3(kreg[c], kf);
        unpack16_e4m3(vreg[c], vf);
        if constexpr (KS) {
          const float ksc = __uint_as_float(kexp[c] << 23), vsc = __uint_as_float(vexp[c] << 23);
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            kf[e] *= ksc;
            vf[e] *= vsc;
          }
        }
        union {
          T v[16];
          uint4 u[2];
        } kp, vp;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          kp.v[e] = from_f32<T>(kf[e]);
          vp.v[e] = from_f32<T>(vf[e]);
        }
        *reinterpret_cast<uint4*>(Ks + row * C::KSTR + ch * 16) = kp.u[0];
        *reinterpret_cast<uint4*>(Ks + row * C::KSTR + ch * 16 + 8) = kp.u[1];
        *reinterpret_cast<uint4*>(Vs + row * C::VSTR + ch * 16) = vp.u[0];
        *reinterpret_cast<uint4*>(Vs + row * C::VSTR + ch * 16 + 8) = vp.u[1];
      } else {
        *reinterpret_cast<uint4*>(Ks + row * C::KSTR + ch * 8) = kreg[c];
        *reinterpret_cast<uint4*>(Vs + row * C::VSTR + ch * 8) = vreg[c];
      }
      if constexpr (PAGED)
        if (ch == 0) dead_lds[row] = ((live_bits >> c) & 1u) ? 0 : 1;
    }
  };

  if (t_first < n_tiles) {
    tload(t_first);
    gload(t_first);
    if (t_first + 1 < n_tiles) tload(t_first + 1);
  }
  for (int t = t_first; t < n_tiles; ++t) {
    __syncthreads();  // previous tile fully consumed
    lstore();
    __syncthreads();
    if (t + 1 < n_tiles) {  // next tile's HBM traffic overlaps this tile's math
      gload(t + 1);
      if (t + 2 < n_tiles) tload(t + 2);
    }

    // ---- S^T = K Q^T : two 32-key sub-tiles -------------------------------------------------
    f32x16 sacc[2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int i = 0; i < 16; ++i) sacc[kt][i] = 0.f;
#pragma unroll
    for (int s = 0; s < C::KSTEPS; ++s) {
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        const F ka = load_frag<F>(Ks + (kt * 32 + r) * C::KSTR + 16 * s + 8 * h);
        sacc[kt] = mfma(ka, qf[s], sacc[kt]);
      }
    }

    // ---- scale, dead keys, online softmax (lane-local row = query qi): v1's arithmetic and order ----------
    const int kbase = t * kBN;
    const bool need_mask = PAGED || kbase + kBN > n_low || (WIN && kbase < lo_high);  // wave-uniform
    [[maybe_unused]] uint32_t dead4[8];  // PAGED: the flags of this lane's keys, 4 consecutive keys per word
    if constexpr (PAGED) {
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int a = 0; a < 4; ++a)
          dead4[kt * 4 + a] = *reinterpret_cast<const uint32_t*>(dead_lds + kt * 32 + 8 * a + 4 * h);
    }
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        float v = sacc[kt][i] * scale_log2;
        if (need_mask) {
          const int key = kbase + kt * 32 + acc_row(i, h);
          bool dead = key >= n;
          if constexpr (WIN) dead = dead || key < lo;
          if constexpr (PAGED) dead = dead || ((dead4[kt * 4 + (i >> 2)] >> (8 * (i & 3))) & 0xffu) != 0;
          v = dead ? -INFINITY : v;
        }
        sacc[kt][i] = v;
        mx = fmaxf(mx, v);
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m, mx);
    const float m_use = (m_new == -INFINITY) ? 0.f : m_new;
    const float alpha = __builtin_amdgcn_exp2f(m - m_use);
    float rs = 0.f;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float p = __builtin_amdgcn_exp2f(sacc[kt][i] - m_use);
        sacc[kt][i] = p;
        rs += p;
      }
    }
    rs += __shfl_xor(rs, 32, 64);
    l = l * alpha + rs;
    m = m_new;
#pragma unroll
    for (int dt = 0; dt < C::DT; ++dt)
#pragma unroll
      for (int i = 0; i < 16; ++i) oacc[dt][i] *= alpha;

    // ---- O^T += V^T P^T ----------------------------------------------------------------------
    F pf[2][2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      pack_frag(pf[kt][0], sacc[kt], 0);
      pack_frag(pf[kt][1], sacc[kt], 1);
    }
#pragma unroll
    for (int dt = 0; dt < C::DT; ++dt) {
      const int col0 = dt * 32 + 16 * (g & 1);
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const F va = tr_frag<F>(Vs3, kt * 32 + 16 * s + 4 * h, col0, C::VSTR, l16);
          oacc[dt] = mfma(va, pf[kt][s], oacc[dt]);
        }
      }
    }
  }

  // ---- epilogue: O = O^T / l; a row without a live key stores zeros ---------------------------------
  if (qi < Tq) {
    const float inv = (l > 0.f) ? 1.f / l : 0.f;
    T* orow = O + b * sx.ob + hq * sx.oh + qi * sx.ot;
#pragma unroll
    for (int dt = 0; dt < C::DT; ++dt) {
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const int d = dt * 32 + 8 * a + 4 * h;
        union {
          T v[4];
          uint2 u;
        } pk;
#pragma unroll
        for (int e = 0; e < 4; ++e) pk.v[e] = from_f32<T>(oacc[dt][4 * a + e] * inv);
        *reinterpret_cast<uint2*>(orow + d) = pk.u;
      }
    }
  }
}

template <typename T, typename KV, int D, bool KS, bool PAGED, bool WIN>
int launch(const void* q, const void* k, const void* v, void* o, int B, int Hq, int Hkv, int Tq, int S, float scale,
           const Strides& sx, const RowPos& rp, std::conditional_t<KS, KVScales, NoScales> sc,
           Pages<PAGED, WIN> pg, hipStream_t stream) {
  const float sl2 = scale * 1.44269504088896340736f;
  dim3 grid(B * Hq, (Tq + kBM - 1) / kBM), block(kThreads);
  hipLaunchKernelGGL((prefill_attn_kernel<T, KV, D, KS, PAGED, WIN>), grid, block, 0, stream, (const T*)q,
                     (const KV*)k, (const KV*)v, (T*)o, Hq, Hkv, Tq, S, sl2, sx, rp, sc, pg);
  return (int)hipGetLastError();
}

// `launch` for q / o of `dtype` and head dim D; KV = void: the cache holds q's type.
template <typename KV, bool KS, bool PAGED, bool WIN, typename... A>
int dispatch(int dtype, int D, A... a) {
  using B16 = __hip_bfloat16;
  constexpr bool kSame = std::is_void_v<KV>;
  if (dtype == kBF16 && D == 64) return launch<B16, std::conditional_t<kSame, B16, KV>, 64, KS, PAGED, WIN>(a...);
  if (dtype == kBF16 && D == 128) return launch<B16, std::conditional_t<kSame, B16, KV>, 128, KS, PAGED, WIN>(a...);
  if (dtype == kF16 && D == 64) return launch<__half, std::conditional_t<kSame, __half, KV>, 64, KS, PAGED, WIN>(a...);
  if (dtype == kF16 && D == 128) return launch<__half, std::conditional_t<kSame, __half, KV>, 128, KS, PAGED, WIN>(a...);
  return (int)hipErrorInvalidValue;
}

// The host side of every entry: the checks, then the kernel's records out of `strides`, which holds (elements; head
// dim contiguous)
//   q b,h,t | k b,h,s | v b,h,s | pos b,t | with KS: k scale b,h,s | v scale b,h,s (bytes) | with PAGED: table b,p
// as decode_attention.hip decode_entry has them, and `o_strides` = O's b,h,t.  KV = void: the cache holds q's type;
// uint8_t: e4m3.  PAGED: k / v (and the scales) are pools, their b strides 0 and S the logical capacity, a multiple
// of the page; `table` int64 [B, S >> lg_page].  WIN: `window` >= 1 keys per row.  A refusal returns
// hipErrorInvalidValue and launches nothing.
template <typename KV, bool KS, bool PAGED, bool WIN = false>
int prefill_entry(int dtype, const void* q, const void* k, const void* v, const void* k_scale, const void* v_scale,
                  const void* pos, void* o, int B, int Hq, int Hkv, int Tq, int S, int D, const int64_t* strides,
                  const int64_t* o_strides, float scale, void* stream, const void* table = nullptr, int lg_page = 0,
                  int num_pages = 0, int window = 0) {
  constexpr bool kE4M3 = std::is_same_v<KV, uint8_t>;
  if (q == nullptr || k == nullptr || v == nullptr || o == nullptr || pos == nullptr || strides == nullptr ||
      o_strides == nullptr)
    return (int)hipErrorInvalidValue;
  if (B <= 0 || Hq <= 0 || Hkv <= 0 || Hq % Hkv != 0 || Tq <= 0 || S <= 0) return (int)hipErrorInvalidValue;
  if ((int64_t)B * Hq > INT32_MAX || (Tq + kBM - 1) / kBM > 65535) return (int)hipErrorInvalidValue;
  // every row is read with 16-byte loads: 8 elements of q and of a 16-bit cache, 16 bytes of an e4m3 cache
  const int64_t unit = kE4M3 ? 16 : 8;
  for (int i = 0; i < 9; ++i)
    if (strides[i] % (i < 3 ? 8 : unit)) return (int)hipErrorInvalidValue;
  for (int i = 0; i < 3; ++i)
    if (o_strides[i] % 4) return (int)hipErrorInvalidValue;  // O is stored 8 bytes at a time
  if ((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) % 16) || ((uintptr_t)o % 8)) return (int)hipErrorInvalidValue;
  const Strides sx{strides[0], strides[1], strides[2], strides[3], strides[4],   strides[5],
                   strides[6], strides[7], strides[8], o_strides[0], o_strides[1], o_strides[2]};
  const RowPos rp{(const int64_t*)pos, strides[9], strides[10]};
  std::conditional_t<KS, KVScales, NoScales> sc{};
  if constexpr (KS) {
    if (k_scale == nullptr || v_scale == nullptr) return (int)hipErrorInvalidValue;
    const int64_t* ss = strides + 11;
    sc = KVScales{(const uint8_t*)k_scale, (const uint8_t*)v_scale, ss[0], ss[1], ss[2], ss[3], ss[4], ss[5]};
  }
  Pages<PAGED, WIN> pg{};
  if constexpr (WIN) {
    if (window < 1) return (int)hipErrorInvalidValue;
    pg.window = window;
  }
  if constexpr (PAGED) {
    if (table == nullptr || lg_page < 4 || lg_page > 24 || num_pages <= 0 || num_pages > (INT32_MAX >> lg_page) ||
        S % (1 << lg_page))
      return (int)hipErrorInvalidValue;
    const int64_t* ts = strides + 11 + (KS ? 6 : 0);
    static_cast<PageMap&>(pg) = PageMap{(const int64_t*)table, ts[0], ts[1], lg_page, num_pages};
  }
  return dispatch<KV, KS, PAGED, WIN>(dtype, D, q, k, v, o, B, Hq, Hkv, Tq, S, scale, sx, rp, sc, pg,
                                      (hipStream_t)stream);
}

}  // namespace

// The position entries: q [B, Hq, Tq, D], k / v [B, Hkv, S, D], `pos` int64 [B, Tq]; `strides` as prefill_entry has
// them, `o_strides` int64[3] = O's (batch, head, token) element strides (e.g. [B, T, H, D] storage).
LTA_EXPORT int lta_prefill_attn_pos(int dtype, const void* q, const void* k, const void* v, const void* pos, void* o,
                                    int B, int Hq, int Hkv, int Tq, int S, int D, const int64_t* strides,
                                    const int64_t* o_strides, float scale, void* stream) {
  return prefill_entry<void, false, false>(dtype, q, k, v, nullptr, nullptr, pos, o, B, Hq, Hkv, Tq, S, D, strides,
                                           o_strides, scale, stream);
}

// The same over an unscaled OCP e4m3 cache: k / v uint8 (strides in bytes, multiples of 16, rows 16-byte aligned).
LTA_EXPORT int lta_prefill_attn_kv8_pos(int dtype, const void* q, const void* k, const void* v, const void* pos,
                                        void* o, int B, int Hq, int Hkv, int Tq, int S, int D, const int64_t* strides,
                                        const int64_t* o_strides, float scale, void* stream) {
  return prefill_entry<uint8_t, false, false>(dtype, q, k, v, nullptr, nullptr, pos, o, B, Hq, Hkv, Tq, S, D, strides,
                                              o_strides, scale, stream);
}

// The same over the scaled e4m3 cache of ops/kv8.py: k_scale / v_scale uint8 [B, Hkv, S, 1] holding e + 127 per row.
LTA_EXPORT int lta_prefill_attn_kv8s_pos(int dtype, const void* q, const void* k, const void* v, const void* k_scale,
                                         const void* v_scale, const void* pos, void* o, int B, int Hq, int Hkv, int Tq,
                                         int S, int D, const int64_t* strides, const int64_t* o_strides, float scale,
                                         void* stream) {
  return prefill_entry<uint8_t, true, false>(dtype, q, k, v, k_scale, v_scale, pos, o, B, Hq, Hkv, Tq, S, D, strides,
                                             o_strides, scale, stream);
}

// The paged entries: the position entries over a paged cache (ops/kv_pages.py).  k / v are pools [Hkv, R + 1, D]
// (strides b = 0, h, row), `table` int64 [B, S >> lg_page], S the logical capacity.
LTA_EXPORT int lta_prefill_attn_paged(int dtype, const void* q, const void* k, const void* v, const void* pos, void* o,
                                      int B, int Hq, int Hkv, int Tq, int S, int D, const int64_t* strides,
                                      const int64_t* o_strides, float scale, const void* table, int lg_page,
                                      int num_pages, void* stream) {
  return prefill_entry<void, false, true>(dtype, q, k, v, nullptr, nullptr, pos, o, B, Hq, Hkv, Tq, S, D, strides,
                                          o_strides, scale, stream, table, lg_page, num_pages);
}

LTA_EXPORT int lta_prefill_attn_kv8_paged(int dtype, const void* q, const void* k, const void* v, const void* pos,
                                          void* o, int B, int Hq, int Hkv, int Tq, int S, int D, const int64_t* strides,
                                          const int64_t* o_strides, float scale, const void* table, int lg_page,
                                          int num_pages, void* stream) {
  return prefill_entry<uint8_t, false, true>(dtype, q, k, v, nullptr, nullptr, pos, o, B, Hq, Hkv, Tq, S, D, strides,
                                             o_strides, scale, stream, table, lg_page, num_pages);
}

LTA_EXPORT int lta_prefill_attn_kv8s_paged(int dtype, const void* q, const void* k, const void* v, const void* k_scale,
                                           const void* v_scale, const void* pos, void* o, int B, int Hq, int Hkv,
                                           int Tq, int S, int D, const int64_t* strides, const int64_t* o_strides,
                                           float scale, const void* table, int lg_page, int num_pages, void* stream) {
  return prefill_entry<uint8_t, true, true>(dtype, q, k, v, k_scale, v_scale, pos, o, B, Hq, Hkv, Tq, S, D, strides,
                                            o_strides, scale, stream, table, lg_page, num_pages);
}

// The window entries: the six entries above with one trailing `window` (keys per row, >= 1; see Window).
// window < 1 returns hipErrorInvalidValue and launches nothing.
LTA_EXPORT int lta_prefill_attn_pos_win(int dtype, const void* q, const void* k, const void* v, const void* pos,
                                        void* o, int B, int Hq, int Hkv, int Tq, int S, int D, const int64_t* strides,
                                        const int64_t* o_strides, float scale, void* stream, int window) {
  return prefill_entry<void, false, false, true>(dtype, q, k, v, nullptr, nullptr, pos, o, B, Hq, Hkv, Tq, S, D, strides,
                                                 o_strides, scale, stream, nullptr, 0, 0, window);
}

LTA_EXPORT int lta_prefill_attn_kv8_pos_win(int dtype, const void* q, const void* k, const void* v, const void* pos,
                                            void* o, int B, int Hq, int Hkv, int Tq, int S, int D,
                                            const int64_t* strides, const int64_t* o_strides, float scale, void* stream,
                                            int window) {
  return prefill_entry<uint8_t, false, false, true>(dtype, q, k, v, nullptr, nullptr, pos, o, B, Hq, Hkv, Tq, S, D,
                                                    strides, o_strides, scale, stream, nullptr, 0, 0, window);
}

LTA_EXPORT int lta_prefill_attn_kv8s_pos_win(int dtype, const void* q, const void* k, const void* v,
                                             const void* k_scale, const void* v_scale, const void* pos, void* o, int B,
                                             int Hq, int Hkv, int Tq, int S, int D, const int64_t* strides,
                                             const int64_t* o_strides, float scale, void* stream, int window) {
  return prefill_entry<uint8_t, true, false, true>(dtype, q, k, v, k_scale, v_scale, pos, o, B, Hq, Hkv, Tq, S, D,
                                                   strides, o_strides, scale, stream, nullptr, 0, 0, window);
}

LTA_EXPORT int lta_prefill_attn_paged_win(int dtype, const void* q, const void* k, const void* v, const void* pos,
                                          void* o, int B, int Hq, int Hkv, int Tq, int S, int D, const int64_t* strides,
                                          const int64_t* o_strides, float scale, const void* table, int lg_page,
                                          int num_pages, void* stream, int window) {
  return prefill_entry<void, false, true, true>(dtype, q, k, v, nullptr, nullptr, pos, o, B, Hq, Hkv, Tq, S, D, strides,
                                                o_strides, scale, stream, table, lg_page, num_pages, window);
}

LTA_EXPORT int lta_prefill_attn_kv8_paged_win(int dtype, const void* q, const void* k, const void* v, const void* pos,
                                              void* o, int B, int Hq, int Hkv, int Tq, int S, int D,
                                              const int64_t* strides, const int64_t* o_strides, float scale,
                                              const void* table, int lg_page, int num_pages, void* stream, int window) {
  return prefill_entry<uint8_t, false, true, true>(dtype, q, k, v, nullptr, nullptr, pos, o, B, Hq, Hkv, Tq, S, D,
                                                   strides, o_strides, scale, stream, table, lg_page, num_pages, window);
}

LTA_EXPORT int lta_prefill_attn_kv8s_paged_win(int dtype, const void* q, const void* k, const void* v,
                                               const void* k_scale, const void* v_scale, const void* pos, void* o,
                                               int B, int Hq, int Hkv, int Tq, int S, int D, const int64_t* strides,
                                               const int64_t* o_strides, float scale, const void* table, int lg_page,
                                               int num_pages, void* stream, int window) {
  return prefill_entry<uint8_t, true, true, true>(dtype, q, k, v, k_scale, v_scale, pos, o, B, Hq, Hkv, Tq, S, D, strides,
                                                  o_strides, scale, stream, table, lg_page, num_pages, window);
}
