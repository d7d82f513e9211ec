// Weight-only e4m3 GEMV for decode (W8A16): y[M, N] = act(x'[M, K] . (q[N, K] / scale)^T + bias) + residual
// for M <= 8 bf16 activation rows, q uint8 holding OCP e4m3fn, scale one fp32 device scalar
// (q = e4m3(w * scale), transforms/fp8_inference.py quantize_weight_e4m3) read in the kernel: no host
// read, so a decode step captures into a hipGraph.  x' = x or rmsnorm(x, g, eps).
//
// Why not the fp8 MFMA: with at most 8 bf16 rows an fp8 MFMA would need fp8 activations (a per-token
// quantisation pass and its error) and 8 of 16 / 32 tile rows would be padding; the problem is a weight
// stream (csrc/gemv.hip, csrc/mxfp4.hip say the same of theirs).
//
// Layout.  One 16-byte load carries 16 weights, so a wave step covers 64 x 16 = 1024 K-elements of a
// row, and lane l pairs its piece with two 16-byte loads per activation row.
//   * A wave owns KR consecutive weight rows.  The workgroup's 4 waves are kw along K times 4 / kw
//     along N, kw chosen per launch from K (4 from K > 2048, 2 from K > 1024, else 1): with K = 2048
//     (every input projection of a 1B model) four waves along K would leave two of them without a
//     single piece, so they take the next KR rows instead.  K below one wave step runs kw = 1: lanes
//     with 16 l >= K issue nothing and add zeros to the reduction.
//   * Bytes in flight.  gemv.hip keeps up to 32 sixteen-byte weight loads per lane in flight as 8 rows
//     x 4 K-steps.  Here a workgroup step already spans 4096 K-elements, the whole row of most
//     projections, so the K depth to request ahead does not exist: the same bytes are taken as twice
//     the rows, KR = 16 with M <= 2 when the launch streams >= 8192 rows, KR = 8 otherwise, x 2 K-steps
//     per request group when K has them and M x KR <= 16; KR = 4 with M <= 2 when 8 rows per wave would
//     make fewer workgroups than the 256 compute units (a 2048 x 2048 projection: 128 against 256).
//     M = 3, 4 run KR = 8 and M = 5..8 KR = 4: the 2 M KR accumulator registers and the 8 M x words
//     set the budget there.  Rows past N are clamped to N - 1 on the read side and never written;
//     activation rows past M repeat row M - 1 and are never written either.
//   * Unpack: v_cvt_pk_f32_fp8, two fp32 per instruction, once per loaded weight word; the pair is
//     used by all M rows.  x pairs (bf16 -> fp32: one shift, one and) are unpacked once per K-quarter
//     of the piece and shared by the KR rows.  The products are v_pk_fma_f32 on (even k, odd k)
//     accumulator pairs, folded before the reduction.
//   * VALU per 16 weight bytes and lane: 8 conversions + 8 M packed FMAs + 16 M / KR x unpacks.
//     M = 1, KR = 16: 17 instructions -> 64 lanes/clk/CU serve ~60 B/clk/CU, an order above the
//     ~8 B/clk/CU that HBM delivers per CU: M = 1 is bound by the weight stream (loads in flight).
//     M = 8, KR = 4: 8 + 64 + 32 = 104 -> ~10 B/clk/CU, the same order as the HBM share; with scalar
//     FMAs (168) it would sit below it.  M = 8 is bound by VALU issue and by the x pieces, which are
//     eight times the weight bytes per wave step (8 rows x 32 B against 4 rows x 16 B) and come from
//     L2, not by HBM.
//   * The scale is applied once: fp32 sums of x . q, times 1 / scale in the epilogue.
//   * The M x KR partial dots are combined as in gemv.hip: a recursive-halving reduce-scatter of
//     shuffles within the wave, then across the kw K-splitting waves through LDS; the threads that
//     own outputs apply bias, activation (ops/gemm.py ACT codes 0, 1, 3, 4) and residual.
// NORM: the row's rstd is computed per wave from the L2-resident x rows after the wave's weight loads
//   are issued (no block barrier in front of them); normalised values are rounded to bf16 exactly as
//   the stand-alone RMSNorm kernel stores them.
// GATED: the wave streams KR / 2 rows of q and the same rows of q2, each with its own scale, and
//   writes act(bf16(x' W^T)) * bf16(x' Wg^T); no bias or residual.
// GROUP: up to three (q, scale, N, y, ldy) segments share x'; block ranges map to segments.
#include "common.h"

namespace lta {
namespace {

typedef float f2 __attribute__((ext_vector_type(2)));
typedef __hip_bfloat16 bf16;

constexpr int kWaves = 4;
constexpr int kStep = 64 * 16;  // K elements per wave step (16 weights per lane)

struct E4Operands {
  const uint8_t* q[3];
  const float* scale[3];
  bf16* y[3];
  int n[3];
  int ldy[3];
  int blocks[2];        // workgroups of segments 0 and 1 (segment 2 takes the rest)
  const uint8_t* q2;    // GATED: the second weight of the pair (same shape as q[0]) and its scale
  const float* scale2;
  const bf16* g;        // NORM: the norm weight (may be null)
  const bf16* bias;     // [N] (may be null)
  const bf16* res;      // residual [M, N], row stride ldr (may be null)
  int ldr;
  int act;
  float eps;
};

__device__ __forceinline__ float e4_act(float v, int act) {
  switch (act) {
    case 1: {
      const float u = 0.7978845608028654f * (v + 0.044715f * v * v * v);
      return 0.5f * v * (1.f + tanhf(u));
    }
    case 3:
      return v / (1.f + __expf(-v));
    case 4:
      return fmaxf(v, 0.f);
    default:
      return v;
  }
}

template <int V>
struct Log2 {
  static constexpr int value = 1 + Log2<V / 2>::value;
};
template <>
struct Log2<1> {
  static constexpr int value = 0;
};

// two bf16 of one 32-bit word (low half = even element) as fp32
__device__ __forceinline__ f2 bf16_pair(uint32_t w) {
  f2 r;
  r.x = __uint_as_float(w << 16);
  r.y = __uint_as_float(w & 0xFFFF0000u);
  return r;
}

__device__ __forceinline__ float round_bf16(float v) { return to_f32(__float2bfloat16(v)); }

// Waves per SIMD the register allocation is held to, from the live set the loop needs: 2 MM KR accumulators,
// 4 U KR weight words, 8 U MM x words, ~48 for the unpacked quarter, addresses and the norm.  Without the
// bound the scheduler hoists every conversion of a piece above the FMAs and spills.
constexpr int waves_per_simd(int MM, int KR, int U) {
  const int regs = 2 * MM * KR + 4 * U * KR + 8 * U * MM + 48;
  return regs <= 100 ? 4 : regs <= 150 ? 3 : 2;
}

template <int MM, int KR, int U, bool NORM, bool GATED>
__global__ __launch_bounds__(kWaves * 64, waves_per_simd(MM, KR, U)) void gemv_e4m3_kernel(
    const bf16* __restrict__ x, int M, int K, int ldx, int kw, E4Operands f) {
  constexpr int V = MM * KR;  // partial sums per lane (power of two, <= 64)
  constexpr int LOGV = Log2<V>::value;
  constexpr int COLS = GATED ? KR / 2 : KR;  // output columns per wave
  static_assert(V <= 64 && (V & (V - 1)) == 0, "V must be a power of two <= 64");
  __shared__ float part[kWaves][V];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // scalar: row addresses stay in SGPRs
  const int kwave = wv & (kw - 1), groups = kWaves / kw;  // this wave's K slot; waves along N

  int blk = blockIdx.x, sg = 0;
  if (blk >= f.blocks[0]) {
    blk -= f.blocks[0];
    sg = 1;
    if (blk >= f.blocks[1]) {
      blk -= f.blocks[1];
      sg = 2;
    }
  }
  const uint8_t* w = sg == 0 ? f.q[0] : sg == 1 ? f.q[1] : f.q[2];
  const float* scale = sg == 0 ? f.scale[0] : sg == 1 ? f.scale[1] : f.scale[2];
  bf16* y = sg == 0 ? f.y[0] : sg == 1 ? f.y[1] : f.y[2];
  const int N = sg == 0 ? f.n[0] : sg == 1 ? f.n[1] : f.n[2];
  const int ldy = sg == 0 ? f.ldy[0] : sg == 1 ? f.ldy[1] : f.ldy[2];
  const int n0 = (blk * groups + wv / kw) * COLS;

  f2 acc[V];
#pragma unroll
  for (int i = 0; i < V; ++i) acc[i] = f2{0.f, 0.f};

  if (n0 < N) {  // wave-uniform; a wave past N only joins the barrier below
    const uint8_t* wrow[KR];
#pragma unroll
    for (int r = 0; r < KR; ++r) {
      const uint8_t* base = (GATED && r >= COLS) ? f.q2 : w;
      wrow[r] = base + (int64_t)min(n0 + (GATED ? r % COLS : r), N - 1) * K;  // clamp: read valid rows only
    }
    const int kstride = kw * kStep;
    const int kbase = kwave * kStep + lane * 16;
    const int steps = (K + kstride - 1) / kstride;
    float rstd[MM];
#pragma unroll
    for (int m = 0; m < MM; ++m) rstd[m] = 1.f;

#pragma unroll 1
    for (int s0 = 0; s0 < steps; s0 += U) {
      // x pieces first, then every weight row piece of the group (vmcnt retires in order: waiting for x
      // never waits for the weights): U * KR sixteen-byte weight loads per lane in flight
      uint4 xv[U][MM][2];
      uint4 wr[U][KR];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int k = kbase + (s0 + u) * kstride;
        if (k < K) {
#pragma unroll
          for (int m = 0; m < MM; ++m) {
            // rows past M repeat row M - 1 (no branch in the FMA loop); their sums are never written
            const uint4* p = reinterpret_cast<const uint4*>(x + (int64_t)min(m, M - 1) * ldx + k);
            xv[u][m][0] = p[0];
            xv[u][m][1] = p[1];
          }
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int k = kbase + (s0 + u) * kstride;
        if (k < K) {
#pragma unroll
          for (int r = 0; r < KR; ++r) wr[u][r] = *reinterpret_cast<const uint4*>(wrow[r] + k);
        }
      }
      if (NORM && s0 == 0) {
        // whole rows per wave, behind the weight requests: no barrier, the weights keep flying
#pragma unroll
        for (int m = 0; m < MM; ++m) {
          if (m >= M) break;  // uniform; the repeated rows past M keep rstd = 1 and are never written
          float ss = 0.f;
          for (int kk = lane * 8; kk < K; kk += 64 * 8) {
            const Vec16<bf16> v = load16(x + (int64_t)m * ldx + kk);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const float t = to_f32(v.v[e]);
              ss = fmaf(t, t, ss);
            }
          }
          rstd[m] = rsqrtf(wave_sum(ss) / (float)K + f.eps);
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int k = kbase + (s0 + u) * kstride;
        if (k < K) {
          uint4 gv[2];
          if constexpr (NORM) {
            if (f.g != nullptr) {
              gv[0] = *reinterpret_cast<const uint4*>(f.g + k);
              gv[1] = *reinterpret_cast<const uint4*>(f.g + k + 8);
            }
          }
#pragma unroll
          for (int qd = 0; qd < 4; ++qd) {  // K-quarters of the piece: 4 weights, one word per row
            f2 xf[MM][2];
#pragma unroll
            for (int m = 0; m < MM; ++m) {
              const uint4 xr = xv[u][m][qd >> 1];
              xf[m][0] = bf16_pair((qd & 1) ? xr.z : xr.x);
              xf[m][1] = bf16_pair((qd & 1) ? xr.w : xr.y);
              if constexpr (NORM) {
                f2 g0{1.f, 1.f}, g1{1.f, 1.f};
                if (f.g != nullptr) {
                  const uint4 gr = gv[qd >> 1];
                  g0 = bf16_pair((qd & 1) ? gr.z : gr.x);
                  g1 = bf16_pair((qd & 1) ? gr.w : gr.y);
                }
                xf[m][0].x = round_bf16(xf[m][0].x * rstd[m] * g0.x);
                xf[m][0].y = round_bf16(xf[m][0].y * rstd[m] * g0.y);
                xf[m][1].x = round_bf16(xf[m][1].x * rstd[m] * g1.x);
                xf[m][1].y = round_bf16(xf[m][1].y * rstd[m] * g1.y);
              }
            }
#pragma unroll
            for (int r = 0; r < KR; ++r) {
              const uint32_t word = qd == 0 ? wr[u][r].x : qd == 1 ? wr[u][r].y : qd == 2 ? wr[u][r].z : wr[u][r].w;
              const f2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)word, false);
              const f2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)word, true);
#pragma unroll
              for (int m = 0; m < MM; ++m) {
                acc[m * KR + r] = __builtin_elementwise_fma(xf[m][0], lo, acc[m * KR + r]);
                acc[m * KR + r] = __builtin_elementwise_fma(xf[m][1], hi, acc[m * KR + r]);
              }
            }
            // keep the quarters apart: the scheduler otherwise hoists every conversion of the piece above
            // the FMAs and the allocator spills
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      }
    }
  }

  // fold the (even k, odd k) pairs, then gemv.hip's reduce-scatter: after LOGV halvings the lane holds
  // element (lane >> (6 - LOGV)) summed over the lanes that share those top bits; a butterfly over the
  // remaining low bits completes the sum
  float s1[V];
#pragma unroll
  for (int i = 0; i < V; ++i) s1[i] = acc[i].x + acc[i].y;
#pragma unroll
  for (int step = 0; step < LOGV; ++step) {
    const int off = 32 >> step;
    const int half = V >> (step + 1);
    const bool upper = (lane & off) != 0;
#pragma unroll
    for (int i = 0; i < half; ++i) {
      const float give = upper ? s1[i] : s1[half + i];
      const float keep = upper ? s1[half + i] : s1[i];
      s1[i] = keep + __shfl_xor(give, off, 64);
    }
  }
  float s = s1[0];
#pragma unroll
  for (int off = 32 >> LOGV; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
  if ((lane & ((64 >> LOGV) - 1)) == 0) part[wv][lane >> (6 - LOGV)] = s;
  __syncthreads();

  // thread t < groups * V owns partial sum e = t % V of the wave group t / V
  const int t = threadIdx.x;
  if (t >= groups * V) return;
  const int grp = t / V, e = t % V;
  const int m = e / KR, r = e % KR;
  const int n = (blk * groups + grp) * COLS + r;
  if (r >= COLS || m >= M || n >= N) return;
  float a = 0.f;
  for (int j = 0; j < kw; ++j) a += part[grp * kw + j][e];
  a *= 1.f / *scale;
  if constexpr (GATED) {
    float b = 0.f;
    for (int j = 0; j < kw; ++j) b += part[grp * kw + j][e + COLS];
    b *= 1.f / *f.scale2;
    y[(int64_t)m * ldy + n] = __float2bfloat16(e4_act(round_bf16(a), f.act) * round_bf16(b));
  } else {
    if (f.bias != nullptr) a += to_f32(f.bias[n]);
    a = e4_act(a, f.act);
    if (f.res != nullptr) a += to_f32(f.res[(int64_t)m * f.ldr + n]);
    y[(int64_t)m * ldy + n] = __float2bfloat16(a);
  }
}

template <int MM, int KR, int U, bool NORM, bool GATED>
void launch_u(const bf16* x, int M, int K, int ldx, int kw, E4Operands f, int nseg, hipStream_t stream) {
  const int cols_per_wg = (GATED ? KR / 2 : KR) * (kWaves / kw);
  int total = 0;
  for (int i = 0; i < nseg; ++i) {
    const int b = (f.n[i] + cols_per_wg - 1) / cols_per_wg;
    if (i < 2) f.blocks[i] = b;
    total += b;
  }
  for (int i = nseg; i < 2; ++i) f.blocks[i] = 1 << 30;
  hipLaunchKernelGGL((gemv_e4m3_kernel<MM, KR, U, NORM, GATED>), dim3(total), dim3(kWaves * 64), 0, stream, x, M, K,
                     ldx, kw, f);
}

// two K-steps per request group where K has them, KR >= 8 and MM * KR <= 16 leaves the registers (waves_per_simd)
template <int MM, int KR, bool NORM, bool GATED>
void launch_kr(const bf16* x, int M, int K, int ldx, int kw, E4Operands f, int nseg, hipStream_t stream) {
  constexpr bool deep = MM * KR <= 16 && KR >= 8;  // the 4-row tiling is for short streams
  const int steps = (K + kw * kStep - 1) / (kw * kStep);
  if (deep && steps >= 2) launch_u<MM, KR, (deep ? 2 : 1), NORM, GATED>(x, M, K, ldx, kw, f, nseg, stream);
  else launch_u<MM, KR, 1, NORM, GATED>(x, M, K, ldx, kw, f, nseg, stream);
}

template <bool NORM, bool GATED>
void launch(const void* xp, int M, int K, int ldx, const E4Operands& f, int nseg, hipStream_t stream) {
  const bf16* x = (const bf16*)xp;
  const int kw = K > 2 * kStep ? 4 : K > kStep ? 2 : 1;
  int64_t rows = 0;
  for (int i = 0; i < nseg; ++i) rows += f.n[i];
  const bool wide = rows * (GATED ? 2 : 1) >= 8192;
  // 8 rows per wave would leave fewer workgroups than the device has compute units (256): 4 rows double them
  const bool narrow = rows * (GATED ? 2 : 1) * kw < 8 * kWaves * 256;
  if (M == 1) {
    if (wide) launch_kr<1, 16, NORM, GATED>(x, M, K, ldx, kw, f, nseg, stream);
    else if (narrow) launch_kr<1, 4, NORM, GATED>(x, M, K, ldx, kw, f, nseg, stream);
    else launch_kr<1, 8, NORM, GATED>(x, M, K, ldx, kw, f, nseg, stream);
  } else if (M == 2) {
    if (wide) launch_kr<2, 16, NORM, GATED>(x, M, K, ldx, kw, f, nseg, stream);
    else if (narrow) launch_kr<2, 4, NORM, GATED>(x, M, K, ldx, kw, f, nseg, stream);
    else launch_kr<2, 8, NORM, GATED>(x, M, K, ldx, kw, f, nseg, stream);
  } else if (M <= 4) {
    launch_kr<4, 8, NORM, GATED>(x, M, K, ldx, kw, f, nseg, stream);
  } else {
    launch_kr<8, 4, NORM, GATED>(x, M, K, ldx, kw, f, nseg, stream);
  }
}

bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

// x and the norm weight are read with 16-byte vector loads, the weight rows (K bytes apart) too
bool e4_operands_ok(const void* x, const void* g, int M, int K, int ldx) {
  return M >= 1 && M <= 8 && K >= 16 && K % 16 == 0 && ldx % 8 == 0 && x != nullptr && aligned16(x) && aligned16(g);
}

}  // namespace
}  // namespace lta

// y [M, N] = act(x' . (q / scale)^T + bias) + res, or act(x' . (q / scale)^T) * (x' . (q2 / scale2)^T) with a
// gate weight (no bias / residual then); x' = x or rmsnorm(x, g, eps) (norm != 0, g may be null).
// x [M, K] bf16 (row stride ldx), q [N, K] e4m3 bytes (contiguous), scale fp32 [1] on the device.
LTA_EXPORT int lta_gemv_e4m3_fused(const void* x, const void* q, const void* scale, const void* q2,
                                   const void* scale2, const void* g, int norm, float eps, const void* bias,
                                   const void* res, void* y, int M, int N, int K, int ldx, int ldy, int ldr, int act,
                                   hipStream_t stream) {
  using namespace lta;
  if (!e4_operands_ok(x, norm ? g : nullptr, M, K, ldx) || N < 1 || q == nullptr || scale == nullptr || y == nullptr)
    return -2;
  if (!aligned16(q) || !aligned16(q2)) return -2;
  if ((q2 != nullptr) != (scale2 != nullptr) || (q2 != nullptr && (bias != nullptr || res != nullptr))) return -2;
  if (act != 0 && act != 1 && act != 3 && act != 4) return -2;
  E4Operands f{};
  f.q[0] = (const uint8_t*)q;
  f.scale[0] = (const float*)scale;
  f.y[0] = (bf16*)y;
  f.n[0] = N;
  f.ldy[0] = ldy;
  f.q2 = (const uint8_t*)q2;
  f.scale2 = (const float*)scale2;
  f.g = norm ? (const bf16*)g : nullptr;
  f.bias = (const bf16*)bias;
  f.res = (const bf16*)res;
  f.ldr = ldr;
  f.act = act;
  f.eps = eps;
  if (norm && q2) launch<true, true>(x, M, K, ldx, f, 1, stream);
  else if (norm) launch<true, false>(x, M, K, ldx, f, 1, stream);
  else if (q2) launch<false, true>(x, M, K, ldx, f, 1, stream);
  else launch<false, false>(x, M, K, ldx, f, 1, stream);
  return (int)hipGetLastError();
}

// Grouped decode projections: y_i [M, N_i] = x' . (q_i / scale_i)^T for i < nseg (<= 3) in one launch, x' as
// above; y_i has row stride ldy_i (adjacent column ranges of one buffer when packed).
LTA_EXPORT int lta_gemv_e4m3_group(const void* x, const void* g, int norm, float eps, int nseg,
                                   const void* const* qs, const void* const* scales, void* const* ys, const int* ns,
                                   const int* ldys, int M, int K, int ldx, hipStream_t stream) {
  using namespace lta;
  if (!e4_operands_ok(x, norm ? g : nullptr, M, K, ldx) || nseg < 1 || nseg > 3) return -2;
  E4Operands f{};
  for (int i = 0; i < nseg; ++i) {
    if (ns[i] < 1 || qs[i] == nullptr || scales[i] == nullptr || ys[i] == nullptr || !aligned16(qs[i])) return -2;
    f.q[i] = (const uint8_t*)qs[i];
    f.scale[i] = (const float*)scales[i];
    f.y[i] = (bf16*)ys[i];
    f.n[i] = ns[i];
    f.ldy[i] = ldys[i];
  }
  f.g = norm ? (const bf16*)g : nullptr;
  f.eps = eps;
  if (norm) launch<true, false>(x, M, K, ldx, f, nseg, stream);
  else launch<false, false>(x, M, K, ldx, f, nseg, stream);
  return (int)hipGetLastError();
}
