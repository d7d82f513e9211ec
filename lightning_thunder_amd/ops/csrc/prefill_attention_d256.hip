// Prefill attention by positions at head dim 256 (K3p-256, Gemma): prefill_attention.hip's semantics in the register
// budget of attention_fwd_d256.hip.  Row (b, hq, t) attends keys lo <= j < n with n = clamp(pos[b, t] + 1, 0, S) and,
// under WIN, lo = clamp(p + 1 - window, 0, n) (else 0); the cache is read as it is stored: 16-bit or OCP e4m3 bytes
// (with or without row scales), static [B, Hkv, S, D] or paged pools [Hkv, R + 1, D] behind a block table.  A row
// without a live key stores zeros; O is stored through its (b, h, t) strides.  Inference only.
//
// The 64-key kernel of prefill_attention.hip is not an instantiation away at D = 256: its Q fragments (64 VGPRs), O
// accumulators (128) and register staging (64) pass 256 registers before the softmax has one, at two waves per SIMD.
// The budget that works at this head dim is the ring kernel's:
//  * one workgroup per CU (__launch_bounds__(256, 1): 256 VGPRs + 256 AGPRs per lane), 4 waves of 32 query rows, grid
//    (B * Hq, query tiles) with the last query tile first; consecutive hq of one KV head are neighbouring workgroups
//    and share K / V through L2;
//  * 32-key tiles; the loop runs floor(lo_min / 32) .. ceil(nmax / 32) with nmax / lo_min the workgroup's largest n and
//    smallest lo (wave reduce, then LDS), so the host sizes the grid from Tq alone and reads neither pos nor the table;
//  * staging is global -> registers -> LDS (the ring kernel's LDS-DMA cannot serve a cache: an e4m3 row has to pass
//    through registers, and a dead key is staged as zeros with nothing loaded).  Per thread and tile: 4 + 4 sixteen-byte
//    chunks of a 16-bit cache (32 VGPRs) or 2 + 2 chunks of 16 e4m3 bytes (16 VGPRs), unpacked with v_cvt_pk_f32_fp8,
//    multiplied by the row's 2^e (scale byte << 23), rounded to T (exact: ops/kv8.py) and written as 2 x 16 bytes, so
//    the LDS tile is the dequantised cache's bit for bit and everything after staging is one code path;
//  * LDS: two stages of K [32][512 B] with 16-byte chunk c at slot c ^ (row & 15) (ds_read_b128 row fragments) and
//    V [32][512 B] with chunk c at slot c ^ ((row & 3) << 2) (ds_read_b64_tr_b16), the ring kernel's two conflict-free
//    swizzles, applied by the staging threads on their writes: 64 KB.  With two stages a tile costs one barrier: at
//    the top of tile t the registers holding tile t + 1 (loaded during tile t - 1's math) go to the other stage, the
//    global loads of tile t + 2 are issued, then tile t's math runs.  The table entries are loaded one tile ahead of
//    the global loads that need them.  On a paged cache a per-key dead flag travels beside its stage;
//  * swapped S^T = K Q^T (16 MFMAs 32x32x16, a lane owns one query), lane-local online softmax in the exp2 domain,
//    P^T packed straight from the S accumulator into O^T += V^T P^T (8 d-tiles x 2 k-steps), O^T in the AGPR file
//    (inline-asm MFMAs; the file is compiled with -amdgpu-mfma-vgpr-form=1 so that S stays in VGPRs);
//  * the ring kernel's deferred rescale: O and l are rescaled only when some row maximum of the wave grows by more
//    than 8 log2 units (exact: P <= 2^8 and l share the offset), so the 128 AGPR read-multiply-writes are a rare event.
//    Because of it the result is not the masked v1 forward's bit for bit; it is held to fp64.
//  * a tile needs no per-key select iff it lies in [lo_high, n_low) of its wave (and the cache is not paged).
// A dead key (at or past nmax, below lo_min, or behind a table entry outside [0, num_pages)) is never loaded: a bad
// position or table entry cannot read outside the cache.  A key below lo_min or at / past nmax has no table lookup.
//
// Deviations from the ring kernel: the LDS reads are plain C++ / builtins (no DMA is in flight whose stage the
// compiler could confuse them with, so it may schedule and count them itself), and the scores are scaled before the
// row maximum is taken (one multiply per score more, but right for any sign of the softmax scale).
#include <type_traits>

#include "attention.h"

using namespace lta;
using namespace lta::attn;

namespace lta {
// called by prefill_attention.hip's dispatch at D = 256; `a` points at its launch arguments in order
int prefill_attn_d256_launch(int dtype, bool e4m3, bool ks, bool paged, bool win, const void* const* a);
}  // namespace lta

namespace {

constexpr int kThreads = 256;
constexpr int kBM = 128;          // queries per workgroup
constexpr int kKT = 32;           // keys per tile
constexpr int kD = 256;           // head dim
constexpr int kRow = kD * 2;      // bytes of an LDS row
constexpr int kImg = kKT * kRow;  // one K or V tile
constexpr int kStage = 2 * kImg;

// The argument records of prefill_attention.hip, duplicated here member for member: that file hands them over by
// address (they are private to each translation unit).
struct KVScales {
  const uint8_t *k, *v;
  int64_t ksb, ksh, kss, vsb, vsh, vss;
};
struct NoScales {};
struct RowPos {
  const int64_t* pos;
  int64_t sb, st;
};
struct PageMap {
  const int64_t* table;
  int64_t sb, sp;
  int lg_page, num_pages;
};
struct NoPages {};
struct WinPageMap : PageMap {
  int window;
};
struct WinNoPages {
  int window;
};
template <bool PAGED, bool WIN>
using Pages = std::conditional_t<WIN, std::conditional_t<PAGED, WinPageMap, WinNoPages>,
                                 std::conditional_t<PAGED, PageMap, NoPages>>;
template <bool KS> using Scales = std::conditional_t<KS, KVScales, NoScales>;
struct Strides {
  int64_t qb, qh, qt, kb, kh, kt, vb, vh, vt, ob, oh, ot;
};

typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
typedef __attribute__((address_space(3))) char lds_char;

// the O^T accumulators live in AGPRs for the whole kernel
__device__ __forceinline__ void mfma_o(f32x16& acc, const bf16x8& a, const bf16x8& b) {
  asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+a"(acc) : "v"(a), "v"(b));
}
__device__ __forceinline__ void mfma_o(f32x16& acc, const f16x8& a, const f16x8& b) {
  asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+a"(acc) : "v"(a), "v"(b));
}
// acc *= a element by element (a C++ multiply pulls the whole tile into VGPRs)
__device__ __forceinline__ void scale_acc(f32x16& acc, float a) {
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    float e = acc[i], tmp;
    asm volatile("v_accvgpr_read_b32 %1, %0\n\tv_mul_f32 %1, %1, %2\n\tv_accvgpr_write_b32 %0, %1"
                 : "+a"(e), "=&v"(tmp)
                 : "v"(a));
    acc[i] = e;
  }
}

// 16 e4m3 bytes as fp32 (OCP e4m3 on gfx950; exact), as prefill_attention.hip unpacks them
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

// V^T fragment (A operand of O^T += V^T P^T): two transposed 4 x 16 reads, 8 rows apart
template <typename F>
__device__ __forceinline__ F vfrag(const lds_char* p) {
  union {
    struct {
      s16x4 a, b;
    } s;
    F f;
  } u;
  u.s.a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)p);
  u.s.b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p + 8 * kRow));
  return u.f;
}

template <typename T, typename KV, bool KS, bool PAGED, bool WIN>
__global__ __launch_bounds__(kThreads, 1) void prefill_attn_d256_kernel(
    const T* __restrict__ Q, const KV* __restrict__ K, const KV* __restrict__ V, T* __restrict__ O, int Hq, int Hkv,
    int Tq, int S, float scale_log2, Strides sx, RowPos rp, Scales<KS> sc, Pages<PAGED, WIN> pg) {
  static_assert(!KS || sizeof(KV) == 1, "scales belong to an e4m3 cache");
  constexpr bool kE4M3 = sizeof(KV) == 1;
  constexpr int EPC = 16 / sizeof(KV);          // cache elements per 16-byte chunk
  constexpr int CH = kD / EPC;                  // chunks per cache row: 32 / 16
  constexpr int LOADS = kKT * CH / kThreads;    // chunks of K (and of V) per thread per tile: 4 / 2
  constexpr int RPL = kThreads / CH;            // rows per load round: 8 / 16
  constexpr float THR = 8.f;
  using F = typename Frag<T>::type;
  __shared__ __attribute__((aligned(1024))) char smem[2 * kStage];
  __shared__ __attribute__((aligned(16))) uint8_t dead_lds[2][kKT];  // PAGED: 1 for a key of the stage that is dead
  __shared__ int wave_n[kThreads / 64];
  __shared__ int wave_first[kThreads / 64];  // WIN: every wave's smallest lo over its rows with n > 0

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
  const int r = lane & 31, h = lane >> 5, g = lane >> 4, l16 = lane & 15, vq = l16 >> 2, vp = l16 & 3;
  const int qi = qt * kBM + wave * 32 + r;  // this lane's query

  // this row's key range, the wave's [lo_high, n_low) and the workgroup's [lo_min, nmax)
  int n = 0;
  [[maybe_unused]] int lo = 0;
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
  const int n_tiles = (nmax + kKT - 1) / kKT;  // workgroup-uniform: the loop holds barriers
  int t_first = 0;
  if constexpr (WIN) {
    // INT32_MAX when no row attends: no tile either
    lo_min = __builtin_amdgcn_readfirstlane(min(min(wave_first[0], wave_first[1]), min(wave_first[2], wave_first[3])));
    t_first = lo_min / kKT;
  }

  // Q fragments (B operand of S^T = K Q^T): Q[qi][16 s + 8 h .. + 7]
  F qf[16];
  {
    const int qrow = min(qi, Tq - 1);
#pragma unroll
    for (int s = 0; s < 16; ++s) qf[s] = load_frag<F>(Qb + (int64_t)qrow * sx.qt + 16 * s + 8 * h);
  }
  f32x16 oacc[8];
#pragma unroll
  for (int dt = 0; dt < 8; ++dt)
#pragma unroll
    for (int i = 0; i < 16; ++i) oacc[dt][i] = 0.f;

  // per-lane LDS offsets.  K chunk (2 s + h) of row r sits at slot (2 s + h) ^ (r & 15) = 2 (s' ^ xh) + hb with
  // s = 8 a + s', xh = (r & 15) >> 1, hb = h ^ (r & 1): k-step s reads koff[s'] + 256 a.  V^T of d-tile dt, rows
  // 4 h + vq (+ 8, 16, 24): chunk 4 dt + 2 (g & 1) + (vp >> 1) at slot 4 (dt ^ vq) + ..., since row & 3 = vq.
  uint32_t koff[8], voff[8];
  {
    const int xh = (r & 15) >> 1, hb = h ^ (r & 1);
#pragma unroll
    for (int s = 0; s < 8; ++s) koff[s] = r * kRow + 32 * (s ^ xh) + 16 * hb;
#pragma unroll
    for (int dt = 0; dt < 8; ++dt)
      voff[dt] = (4 * h + vq) * kRow + ((4 * (dt ^ vq) + 2 * (g & 1) + (vp >> 1)) << 4) + 8 * (vp & 1);
  }

  // register staging of one K / V tile: thread tid holds chunk (tid % CH) of rows c * RPL + tid / CH
  const int srow = tid / CH, sch = tid % CH;
  uint4 kreg[LOADS], vreg[LOADS];
  [[maybe_unused]] uint32_t kexp[LOADS], vexp[LOADS];  // KS: the row's scale bytes
  [[maybe_unused]] int prow[LOADS];                    // PAGED: the chunk's pool row, -1 for a dead key
  [[maybe_unused]] unsigned live_bits = 0;             // PAGED: bit c = chunk c of the staged tile is live
  // PAGED: the pool rows of tile t, one tile ahead of its loads
  auto tload = [&](int t) {
    if constexpr (PAGED) {
#pragma unroll
      for (int c = 0; c < LOADS; ++c) {
        const int key = t * kKT + c * RPL + srow;
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
    for (int c = 0; c < LOADS; ++c) {
      int64_t kr = t * kKT + c * RPL + srow;  // the key's row in its cache
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
        kreg[c] = *reinterpret_cast<const uint4*>(Kb + kr * sx.kt + sch * EPC);
        vreg[c] = *reinterpret_cast<const uint4*>(Vb + kr * sx.vt + sch * EPC);
        if constexpr (KS) {
          kexp[c] = ksrow[kr * sc.kss];
          vexp[c] = vsrow[kr * sc.vss];
        }
      }
    }
  };
  // the staged registers into stage st, through the two swizzles
  auto lstore = [&](int st) {
    char* kimg = smem + st * kStage;
    char* vimg = kimg + kImg;
#pragma unroll
    for (int c = 0; c < LOADS; ++c) {
      const int row = c * RPL + srow;
      char* krow = kimg + row * kRow;
      char* vrow = vimg + row * kRow;
      const int kx = row & 15, vx = (row & 3) << 2;
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
        } kp, vp2;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          kp.v[e] = from_f32<T>(kf[e]);
          vp2.v[e] = from_f32<T>(vf[e]);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          *reinterpret_cast<uint4*>(krow + (((2 * sch + j) ^ kx) << 4)) = kp.u[j];
          *reinterpret_cast<uint4*>(vrow + (((2 * sch + j) ^ vx) << 4)) = vp2.u[j];
        }
      } else {
        *reinterpret_cast<uint4*>(krow + ((sch ^ kx) << 4)) = kreg[c];
        *reinterpret_cast<uint4*>(vrow + ((sch ^ vx) << 4)) = vreg[c];
      }
      if constexpr (PAGED)
        if (sch == 0) dead_lds[st][row] = ((live_bits >> c) & 1u) ? 0 : 1;
    }
  };

  float m_use = -INFINITY, l = 0.f;  // l: this lane's half of the row (keys 8 a + 4 h + 0..3)
  const float ninf = -INFINITY;

  if (t_first < n_tiles) {
    tload(t_first);
    gload(t_first);
    if (t_first + 1 < n_tiles) tload(t_first + 1);
    lstore(0);
    if (t_first + 1 < n_tiles) {
      gload(t_first + 1);
      if (t_first + 2 < n_tiles) tload(t_first + 2);
    }
  }
  for (int t = t_first; t < n_tiles; ++t) {
    const int st = (t - t_first) & 1;
    __syncthreads();  // tile t is in stage st for every wave; stage st ^ 1 (tile t - 1) is fully consumed
    if (t + 1 < n_tiles) {
      lstore(st ^ 1);  // tile t + 1, loaded during tile t - 1's math
      if (t + 2 < n_tiles) {  // tile t + 2's HBM traffic overlaps this tile's math
        gload(t + 2);
        if (t + 3 < n_tiles) tload(t + 3);
      }
    }
    const lds_char* kimg = (const lds_char*)smem + st * kStage;
    const lds_char* vimg = kimg + kImg;

    // ---- S^T = K Q^T : 16 k-steps over d -----------------------------------------------------
    f32x16 sacc;
#pragma unroll
    for (int i = 0; i < 16; ++i) sacc[i] = 0.f;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int s = 0; s < 8; ++s) 
        sacc = mfma(*reinterpret_cast<const __attribute__((address_space(3))) F*>(kimg + koff[s] + 256 * a),
                    qf[8 * a + s], sacc);

    // ---- scale, dead keys, deferred online softmax (lane-local row + the lane ^ 32 partner) ---------
    const int kbase = t * kKT;
    const bool need_mask = PAGED || kbase + kKT > n_low || (WIN && kbase < lo_high);  // wave-uniform
    [[maybe_unused]] uint32_t dead4[4];  // PAGED: the flags of this lane's keys, 4 consecutive keys per word
    if constexpr (PAGED) {
#pragma unroll
      for (int a = 0; a < 4; ++a) dead4[a] = *reinterpret_cast<const uint32_t*>(&dead_lds[st][8 * a + 4 * h]);
    }
    float mx = ninf;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      float v = sacc[i] * scale_log2;
      if (need_mask) {
        const int key = kbase + acc_row(i, h);
        bool dead = key >= n;
        if constexpr (WIN) dead = dead || key < lo;
        if constexpr (PAGED) dead = dead || ((dead4[i >> 2] >> (8 * (i & 3))) & 0xffu) != 0;
        v = dead ? ninf : v;
      }
      sacc[i] = v;
      mx = fmaxf(mx, v);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    if (__builtin_amdgcn_ballot_w64(mx > m_use + THR || (m_use == ninf && mx != ninf)) != 0) {
      const float m_new = fmaxf(m_use, mx);
      const float alpha = m_use == ninf ? 0.f : __builtin_amdgcn_exp2f(m_use - m_new);
      l *= alpha;
#pragma unroll
      for (int dt = 0; dt < 8; ++dt) scale_acc(oacc[dt], alpha);
      m_use = m_new;
    }
    const float msafe = m_use == ninf ? 0.f : m_use;
    float rs = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float pv = __builtin_amdgcn_exp2f(sacc[i] - msafe);
      sacc[i] = pv;
      rs += pv;
    }
    l += rs;
    F pf0, pf1;
    pack_frag(pf0, sacc, 0);
    pack_frag(pf1, sacc, 1);

    // ---- O^T += V^T P^T : 8 d-tiles x 2 key steps -------------------------------------------------
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) {
      const F v0 = vfrag<F>(vimg + voff[dt]);
      const F v1 = vfrag<F>(vimg + voff[dt] + 16 * kRow);
      mfma_o(oacc[dt], v0, pf0);
      mfma_o(oacc[dt], v1, pf1);
    }
  }

  // ---- epilogue: O = O^T / l; a row without a live key stores zeros ---------------------------------
  l += __shfl_xor(l, 32, 64);
  if (qi < Tq) {
    const float inv = (l > 0.f) ? 1.f / l : 0.f;
    T* orow = O + b * sx.ob + hq * sx.oh + (int64_t)qi * sx.ot;
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) {
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        union {
          T v[4];
          uint2 u;
        } pk;
#pragma unroll
        for (int e = 0; e < 4; ++e) pk.v[e] = from_f32<T>(oacc[dt][4 * a + e] * inv);
        *reinterpret_cast<uint2*>(orow + dt * 32 + 8 * a + 4 * h) = pk.u;
      }
    }
  }
}

// `a`: q, k, v, o, B, Hq, Hkv, Tq, S, scale, Strides, RowPos, scales record, pages record, stream
template <typename T, typename KV, bool KS, bool PAGED, bool WIN>
int launch(const void* const* a) {
  const auto ptr = [&](int i) { return *(void* const*)a[i]; };
  const auto num = [&](int i) { return *(const int*)a[i]; };
  const int B = num(4), Hq = num(5), Hkv = num(6), Tq = num(7), S = num(8);
  const float sl2 = *(const float*)a[9] * 1.44269504088896340736f;
  dim3 grid(B * Hq, (Tq + kBM - 1) / kBM), block(kThreads);
  hipLaunchKernelGGL((prefill_attn_d256_kernel<T, KV, KS, PAGED, WIN>), grid, block, 0, *(const hipStream_t*)a[14],
                     (const T*)ptr(0), (const KV*)ptr(1), (const KV*)ptr(2), (T*)ptr(3), Hq, Hkv, Tq, S, sl2,
                     *(const Strides*)a[10], *(const RowPos*)a[11], *(const Scales<KS>*)a[12],
                     *(const Pages<PAGED, WIN>*)a[13]);
  return (int)hipGetLastError();
}

template <typename T, typename KV, bool KS>
int by_selector(bool paged, bool win, const void* const* a) {
  if (paged) return win ? launch<T, KV, KS, true, true>(a) : launch<T, KV, KS, true, false>(a);
  return win ? launch<T, KV, KS, false, true>(a) : launch<T, KV, KS, false, false>(a);
}

template <typename T>
int by_format(bool e4m3, bool ks, bool paged, bool win, const void* const* a) {
  if (!e4m3) return ks ? (int)hipErrorInvalidValue : by_selector<T, T, false>(paged, win, a);
  return ks ? by_selector<T, uint8_t, true>(paged, win, a) : by_selector<T, uint8_t, false>(paged, win, a);
}

}  // namespace

int lta::prefill_attn_d256_launch(int dtype, bool e4m3, bool ks, bool paged, bool win, const void* const* a) {
  if (dtype == kBF16) return by_format<__hip_bfloat16>(e4m3, ks, paged, win, a);
  if (dtype == kF16) return by_format<__half>(e4m3, ks, paged, win, a);
  return (int)hipErrorInvalidValue;
}
