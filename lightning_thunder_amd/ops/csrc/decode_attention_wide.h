// Decode attention at head dim 256 (K3w): the wide-row kernel of csrc/decode_attention.hip, which includes this file
// after its own kernel's records (Selector, KVScales, kSumStart, normalised, load16_e4m3) and launches it for D = 256.
//
// Why not decode_attn_kernel at D = 256: that kernel gives a lane one key and a private acc[D], 256 accumulator
// registers before one load is in flight, and each of its load instructions walks 64 different 512-byte rows.
// Here a key row is spread over lanes instead (wave64, CDNA4, VALU only: at T = 1 an MFMA tile is padding):
//   * NV = 16 / sizeof(KV) elements per 16-byte load, LPK = D / NV lanes per key row (32 for a 16-bit cache, 16 for
//     e4m3), KPI = 64 / LPK key rows per load instruction (2 / 4).  Lane (g, r) = (lane / LPK, lane % LPK) owns head
//     dims [r * NV, (r + 1) * NV): its NV scaled q values and its acc[NV] live in registers, and load instruction i
//     of a 64-key block reads that slice of key i * KPI + g, so one instruction reads KPI whole rows (1 KiB where
//     the rows are adjacent).  A block is LPK K loads and LPK V loads, issued kBatch at a time ahead of their use;
//   * after the K loads of a batch a lane holds kBatch partial dots; a recursive-halving reduce-scatter over the LPK
//     lanes of its group leaves lane (g, r) with the whole score of key r * KPI + g: it is that key's owner.
//     The owner decides `valid` exactly as decode_attn_kernel does, loads the key's scale bytes under KS, and
//     publishes the key's cache row (or -1: dead) and later p (under KS p * 2^ev) in wave-private LDS, where the
//     lanes of group g read their LPK entries back as contiguous 16-byte broadcasts.  No block-level barrier;
//   * nothing of a dead key is loaded: its K slice stands in as zeros under a score of -inf, its V slice as -0 under
//     p = 0, the one addend that leaves every accumulator as it is, a -0 included (kSumStart).  A block without a
//     valid key is skipped before any K / V traffic;
//   * acc is scaled by corr once per block, then takes one fmaf per loaded V element; at the end of the row the KPI
//     groups are summed with log2(KPI) xor-shuffles of NV values and group 0 stores the row, 16 bytes at a time.
// The row-to-wave mapping, WSPLIT and its LDS merge, the POS / WIN live-range split over gridDim.y, the workspace
// [split][row][D] with decode_attn_combine_kernel, kSumStart, `normalised` and the causal flag are that kernel's,
// rule for rule, so the host's launch shape and every entry's checks are shared.  A paged and a static cache, and
// a window that covers the row and none, run the same arithmetic in the same order: only addresses differ.
#pragma once

namespace lta {
namespace {

template <typename T, typename KV, int D, bool WSPLIT, bool KS = false, bool POS = false, bool PAGED = false,
          bool WIN = false>
__global__ __launch_bounds__(256) void decode_attn_wide_kernel(
    const T* __restrict__ q, const KV* __restrict__ k, const KV* __restrict__ v, const uint8_t* __restrict__ mask,
    T* __restrict__ o, float* __restrict__ ws_acc, float* __restrict__ ws_ml, int B, int Hq, int Hkv, int Tq, int S,
    int64_t qsb, int64_t qsh, int64_t qst, int64_t ksb, int64_t ksh, int64_t kss, int64_t vsb, int64_t vsh,
    int64_t vss, int64_t msb, int64_t msh, int64_t mst, int64_t mss, int chunk, int causal, float scale,
    std::conditional_t<KS, KVScales, NoScales> sc, Selector<POS, PAGED, WIN> rp) {
  static_assert(!KS || sizeof(KV) == 1, "scales belong to an e4m3 cache");
  static_assert(!PAGED || POS, "a paged cache is read by positions");
  static_assert(!WIN || POS, "a window hangs on a row's position");
  static_assert(sizeof(T) == 2, "q and the output are 16-bit");
  constexpr bool kE4M3 = sizeof(KV) == 1;
  constexpr int NV = 16 / sizeof(KV);  // elements per 16-byte load = head dims per lane
  constexpr int LPK = D / NV;          // lanes per key row = load instructions per block and operand
  constexpr int KPI = 64 / LPK;        // key rows per load instruction = lane groups
  constexpr int kBatch = 8;            // loads issued ahead of their first use
  static_assert(LPK * KPI == 64 && LPK % kBatch == 0 && NV % 8 == 0, "the lane layout");
  // a dead key's V slice: -0 in every element of either cache format
  constexpr uint32_t kMinusZeros = kE4M3 ? 0x80808080u : 0x80008000u;
  __shared__ __attribute__((aligned(16))) int row_lds[kRowsPerBlock][64];
  __shared__ __attribute__((aligned(16))) float p_lds[kRowsPerBlock][64];
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

  const int g = lane / LPK, r = lane % LPK;
  const int own = r * KPI + g;  // the key of a block whose score the reduce-scatter leaves with this lane

  // this lane's slice of the scaled q row, in registers
  float qf[NV];
  {
    const T* qrow = q + b * qsb + hq * qsh + t * qst + r * NV;
#pragma unroll
    for (int c = 0; c < NV; c += 8) {
      const Vec16<T> x = load16(qrow + c);
#pragma unroll
      for (int e = 0; e < 8; ++e) qf[c + e] = to_f32(x.v[e]) * scale;
    }
  }
  const KV* kbase = k + b * ksb + hk * ksh + r * NV;
  const KV* vbase = v + b * vsb + hk * vsh + r * NV;
  [[maybe_unused]] const uint8_t* mrow = mask ? mask + b * msb + hq * msh + t * mst : nullptr;
  [[maybe_unused]] const uint8_t* ksrow = nullptr;
  [[maybe_unused]] const uint8_t* vsrow = nullptr;
  if constexpr (KS) {
    ksrow = sc.k + b * sc.ksb + hk * sc.ksh;
    vsrow = sc.v + b * sc.vsb + hk * sc.vsh;
  }
  // the group's LPK published entries, read back four at a time (16-byte LDS broadcasts)
  const int* my_rows = &row_lds[w][g * LPK];
  const float* my_p = &p_lds[w][g * LPK];

  // one 16-byte slice as NV fp32 values
  auto unpack = [](const uint4& raw, float (&x)[NV]) {
    if constexpr (kE4M3) {
      const uint32_t wd[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const auto lo2 = __builtin_amdgcn_cvt_pk_f32_fp8((int)wd[i], false);
        const auto hi2 = __builtin_amdgcn_cvt_pk_f32_fp8((int)wd[i], true);
        x[4 * i + 0] = lo2[0];
        x[4 * i + 1] = lo2[1];
        x[4 * i + 2] = hi2[0];
        x[4 * i + 3] = hi2[1];
      }
    } else {
      Vec16<T> y;
      y.raw = raw;
#pragma unroll
      for (int e = 0; e < NV; ++e) x[e] = to_f32(y.v[e]);
    }
  };

  float m = -INFINITY, l = 0.f;
  float acc[NV];
#pragma unroll
  for (int e = 0; e < NV; ++e) acc[e] = kSumStart<KV>;

  for (int j0 = j_begin + (WSPLIT ? w * 64 : 0); j0 < j_end; j0 += (WSPLIT ? kRowsPerBlock * 64 : 64)) {
    // ---- the owner's part: is key j alive, and where is its row
    const int j = j0 + own;
    bool valid = j < j_end;
    if constexpr (WIN) valid = valid && j >= lo;
    if constexpr (!POS) {
      if (valid && mrow) valid = mrow[(int64_t)j * mss] != 0;
    }
    int kr = j;  // the key's row in its cache (a pool row fits an int: num_pages << lg_page <= INT32_MAX)
    if constexpr (PAGED) {
      if (valid) {  // one table entry per lane: j < j_end <= S = (table entries per sequence) << lg_page
        const int64_t pid = rp.pg.table[b * rp.pg.sb + (int64_t)(j >> rp.pg.lg_page) * rp.pg.sp];
        valid = pid >= 0 && pid < rp.pg.num_pages;
        kr = (int)((pid << rp.pg.lg_page) + (j & ((1 << rp.pg.lg_page) - 1)));
      }
    }
    if (!__any(valid)) continue;  // fully masked block: no K/V traffic
    [[maybe_unused]] uint32_t kb = 127, vb = 127;
    if constexpr (KS) {
      if (valid) {
        kb = ksrow[(int64_t)kr * sc.kss];
        vb = vsrow[(int64_t)kr * sc.vss];
      }
    }
    row_lds[w][lane] = valid ? kr : -1;
    __builtin_amdgcn_wave_barrier();

    // ---- QK^T, kBatch keys at a time: kBatch loads in flight, kBatch partial dots, then the recursive-halving
    // reduce-scatter over the group's LPK lanes, its kBatch-lane steps first: lane (g, r) ends with the score of
    // key r * KPI + g.  A loop, not unrolled: the loads of one batch are all that is in flight
    float dot = 0.f;
#pragma unroll 1
    for (int i0 = 0; i0 < LPK; i0 += kBatch) {
      int rr[kBatch];
#pragma unroll
      for (int u = 0; u < kBatch; u += 4)
        __builtin_memcpy(&rr[u], __builtin_assume_aligned(my_rows + i0 + u, 16), 16);
      uint4 raw[kBatch];
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        raw[u] = make_uint4(0, 0, 0, 0);
        if (rr[u] >= 0) raw[u] = *reinterpret_cast<const uint4*>(kbase + (int64_t)rr[u] * kss);
      }
      float part[kBatch];
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        float x[NV];
        unpack(raw[u], x);
        part[u] = 0.f;
#pragma unroll
        for (int e = 0; e < NV; ++e) part[u] = fmaf(qf[e], x[e], part[u]);
      }
#pragma unroll
      for (int off = kBatch / 2, n = kBatch; off >= 1; off >>= 1, n >>= 1) {
        const bool upper = (lane & off) != 0;
        const int half = n >> 1;
#pragma unroll
        for (int i = 0; i < half; ++i) {
          const float give = upper ? part[i] : part[half + i];
          const float keep = upper ? part[half + i] : part[i];
          part[i] = keep + __shfl_xor(give, off, 64);
        }
      }
      // part[0]: key i0 + r % kBatch over this lane's kBatch-lane set; the sets of the group hold the other dims,
      // and the lane whose set index is the batch's keeps the sum (the halving steps over the batches)
#pragma unroll
      for (int off = kBatch; off < LPK; off <<= 1) part[0] += __shfl_xor(part[0], off, 64);
      if (r / kBatch == i0 / kBatch) dot = part[0];
    }
    float s = -INFINITY;
    if (valid) {
      s = dot;
      if constexpr (KS) s = dot * __uint_as_float(kb << 23);
    }

    // ---- online softmax, one wave max and one wave sum per block
    const float m_new = fmaxf(m, wave_max(s));
    const float p = valid ? __expf(s - m_new) : 0.f;
    const float corr = __expf(m - m_new);  // m = -inf on the first block -> 0
    l = l * corr + wave_sum(p);
    m = m_new;
    p_lds[w][lane] = KS ? p * __uint_as_float(vb << 23) : p;
    __builtin_amdgcn_wave_barrier();

    // ---- PV: acc scaled once, then one fmaf per loaded V element
#pragma unroll
    for (int e = 0; e < NV; ++e) acc[e] *= corr;
#pragma unroll 1
    for (int i0 = 0; i0 < LPK; i0 += kBatch) {
      int rr[kBatch];
      float pp[kBatch];
#pragma unroll
      for (int u = 0; u < kBatch; u += 4) {
        __builtin_memcpy(&rr[u], __builtin_assume_aligned(my_rows + i0 + u, 16), 16);
        __builtin_memcpy(&pp[u], __builtin_assume_aligned(my_p + i0 + u, 16), 16);
      }
      uint4 raw[kBatch];
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        raw[u] = make_uint4(kMinusZeros, kMinusZeros, kMinusZeros, kMinusZeros);
        if (rr[u] >= 0) raw[u] = *reinterpret_cast<const uint4*>(vbase + (int64_t)rr[u] * vss);
      }
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        float x[NV];
        unpack(raw[u], x);
#pragma unroll
        for (int e = 0; e < NV; ++e) acc[e] = fmaf(pp[u], x[e], acc[e]);
      }
    }
    __builtin_amdgcn_wave_barrier();  // the next block's owners write where this one's loads were read
  }

  // the KPI groups hold partial rows over disjoint keys: sum them, every lane ends with dims [r * NV, (r + 1) * NV)
#pragma unroll
  for (int off = LPK; off < 64; off <<= 1) {
#pragma unroll
    for (int e = 0; e < NV; ++e) acc[e] += __shfl_xor(acc[e], off, 64);
  }

  if constexpr (WSPLIT) {
    __shared__ __attribute__((aligned(16))) float c_acc[kRowsPerBlock][D];
    __shared__ float c_ml[kRowsPerBlock][2];
    if (g == 0) {
#pragma unroll
      for (int e = 0; e < NV; ++e) c_acc[w][r * NV + e] = acc[e];
    }
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
    for (int e = 0; e < NV; ++e) acc[e] = kSumStart<KV>;
#pragma unroll
    for (int u = 0; u < kRowsPerBlock; ++u) {
      const float c = c_ml[u][0] == -INFINITY ? 0.f : __expf(c_ml[u][0] - M);
      L = fmaf(c, c_ml[u][1], L);
#pragma unroll
      for (int e = 0; e < NV; ++e) acc[e] = fmaf(c, c_acc[u][r * NV + e], acc[e]);
    }
    m = M;
    l = L;
  }

  if (g != 0) return;  // group 0 stores the row
  if (gridDim.y == 1) {
    const float inv = 1.f / l;  // fully masked row -> 0 * inf = nan, like PyTorch SDPA
    T* orow = o + (((int64_t)b * Hq + hq) * Tq + t) * D + r * NV;  // o is [B, Hq, Tq, D]
#pragma unroll
    for (int c = 0; c < NV; c += 8) {
      Vec16<T> y;
#pragma unroll
      for (int e = 0; e < 8; ++e) y.v[e] = normalised<T, KV, KS || POS>(acc[c + e], inv);
      store16(orow + c, y);
    }
  } else {
    float4* wa = reinterpret_cast<float4*>(ws_acc + ((int64_t)split * rows + row) * D + r * NV);
#pragma unroll
    for (int c = 0; c < NV; c += 4) wa[c / 4] = make_float4(acc[c], acc[c + 1], acc[c + 2], acc[c + 3]);
    if (lane == 0) {
      ws_ml[((int64_t)split * rows + row) * 2 + 0] = m;
      ws_ml[((int64_t)split * rows + row) * 2 + 1] = l;
    }
  }
}

}  // namespace
}  // namespace lta
