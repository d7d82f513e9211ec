// MXFP4 weight-only GEMV for decode: y[M, N] = x[M, K] . dequant(W)[N, K]^T with W packed e2m1
// [N, K/2] (low nibble = even k) and E8M0 scales S [N, K/32]; x / y bf16, M <= 8 rows.
//
// Decode is weight-streaming bound: the weight is read once per token, so 4-bit storage streams a
// quarter of the bf16 bytes.  Each lane owns whole 32-element blocks (16 weight bytes + 1 scale):
// one 16-B load, the gfx950 scaled conversion v_cvt_scalef32_pk_f32_fp4 (two scaled fp32 values
// per instruction, the E8M0 scale folded in) and fp32 FMAs against the block's x values, which
// every wave re-reads from L2/L1 (x is a few KB).  A wave computes NPW output columns so each x
// load feeds NPW weight rows (x bytes per weight byte = 4 / NPW); lanes of a wave walk consecutive blocks of the rows (1 KiB per
// wave-instruction, coalesced), and a butterfly reduces the 64 partial sums.
//
// The fused forms carry what csrc/gemv.hip carries for bf16 weights: an RMSNorm prologue, the gated
// (SwiGLU) pair in one launch, bias / activation / residual in the epilogue, and up to three
// projections of one x in one launch.  The plain form (lta_gemv_mxfp4) compiles to the same code
// as before they existed.
#include "common.h"

using namespace lta;

namespace {

typedef float f2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int WAVES = 4;   // waves per workgroup
constexpr int MAXM = 8;

__device__ __forceinline__ float e8m0_to_f32(uint32_t be) {
  return be == 0 ? __uint_as_float(0x00400000u) : __uint_as_float(be << 23);  // 2^(be - 127)
}

// The fused forms (FUSED) take their operands from one table: up to three (q, s, N, y, ldy)
// segments that share x (attention q / k / v in one launch; a block range per segment), the gate
// weight, the norm weight and the epilogue operands.
struct Mx4Fused {
  const uint8_t* q[3];
  const uint8_t* s[3];
  __hip_bfloat16* y[3];
  int n[3];
  int ldy[3];
  int blocks[2];      // workgroups of segments 0 and 1 (segment 2 takes the rest)
  const uint8_t* q2;  // GATED: the second weight of the pair (same shape as q[0]) and its scales
  const uint8_t* s2;
  const __hip_bfloat16* g;    // NORM: the norm weight (may be null)
  const __hip_bfloat16* res;  // residual [M, N], row stride ldr (may be null)
  int ldr;
  int act;  // ops/gemm.py ACT: 0 none, 1 gelu (tanh), 3 silu, 4 relu
  float eps;
};

__device__ __forceinline__ float mx4_act(float v, int act) {
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

// NORM: x is replaced by bf16(x * rstd * g), rounded as the stand-alone RMSNorm stores it.  The
//   row sums of squares are taken once per workgroup (each wave a quarter of every row, combined
//   through LDS behind one barrier ahead of the FMA loop); -DLTA_MX4_NORM_PER_WAVE builds the
//   measured alternative (every wave sums whole rows, no barrier; profiles/mxfp4_decode_fusion.txt).
// GATED: a wave computes NPW / 2 columns of w and the same columns of w2 and stores
//   bf16(act(bf16(x w^T)) * bf16(x w2^T)), as the unfused linear -> swiglu chain rounds them.
// FUSED epilogue: v + bias, activation, + residual in fp32, one rounding.
template <int M, int NPW, bool NORM = false, bool GATED = false, bool FUSED = false>
__global__ __launch_bounds__(WAVES * 64) void gemv_mxfp4_kernel(const __hip_bfloat16* __restrict__ x,
                                                                 const uint8_t* __restrict__ w_,
                                                                 const uint8_t* __restrict__ s_,
                                                                 const __hip_bfloat16* __restrict__ bias,
                                                                 __hip_bfloat16* __restrict__ y_, int N_, int K, int ldx,
                                                                 int ldy_, Mx4Fused f = Mx4Fused{}) {
  static_assert(FUSED || (!NORM && !GATED), "norm / gate need the operand table");
  constexpr int COLS = GATED ? NPW / 2 : NPW;  // output columns per wave
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint8_t* w = w_;
  const uint8_t* s = s_;
  __hip_bfloat16* y = y_;
  int N = N_, ldy = ldy_, blk = blockIdx.x;
  if constexpr (FUSED) {
    int sg = 0;
    if (blk >= f.blocks[0]) {
      blk -= f.blocks[0];
      sg = 1;
      if (blk >= f.blocks[1]) {
        blk -= f.blocks[1];
        sg = 2;
      }
    }
    w = sg == 0 ? f.q[0] : sg == 1 ? f.q[1] : f.q[2];
    s = sg == 0 ? f.s[0] : sg == 1 ? f.s[1] : f.s[2];
    y = sg == 0 ? f.y[0] : sg == 1 ? f.y[1] : f.y[2];
    N = sg == 0 ? f.n[0] : sg == 1 ? f.n[1] : f.n[2];
    ldy = sg == 0 ? f.ldy[0] : sg == 1 ? f.ldy[1] : f.ldy[2];
  }
  const int n0 = (blk * WAVES + wave) * COLS;
  float rstd[M];
  if constexpr (NORM) {
#ifdef LTA_MX4_NORM_PER_WAVE
    if (n0 >= N) return;
#pragma unroll
    for (int m = 0; m < M; ++m) {
      float ss = 0.f;
      for (int k = lane * 8; k < K; k += 64 * 8) {
        const Vec16<__hip_bfloat16> xv = load16(x + (int64_t)m * ldx + k);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float v = to_f32(xv.v[e]);
          ss = fmaf(v, v, ss);
        }
      }
      rstd[m] = rsqrtf(wave_sum(ss) / (float)K + f.eps);
    }
#else
    __shared__ float ss_part[WAVES][M];
#pragma unroll
    for (int m = 0; m < M; ++m) {
      float ss = 0.f;
      for (int k = (int)threadIdx.x * 8; k < K; k += WAVES * 64 * 8) {
        const Vec16<__hip_bfloat16> xv = load16(x + (int64_t)m * ldx + k);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float v = to_f32(xv.v[e]);
          ss = fmaf(v, v, ss);
        }
      }
      ss = wave_sum(ss);
      if (lane == 0) ss_part[wave][m] = ss;
    }
    __syncthreads();  // every wave of the workgroup arrives: the out-of-range exit comes after
#pragma unroll
    for (int m = 0; m < M; ++m)
      rstd[m] = rsqrtf((ss_part[0][m] + ss_part[1][m] + ss_part[2][m] + ss_part[3][m]) / (float)K + f.eps);
    if (n0 >= N) return;
#endif
  } else {
    if (n0 >= N) return;  // whole waves only; no barrier below
  }
  const int nb = K / 32;
  float acc[M][NPW];
#pragma unroll
  for (int m = 0; m < M; ++m)
#pragma unroll
    for (int j = 0; j < NPW; ++j) acc[m][j] = 0.f;

  // two trips in flight; one with NORM, whose fp32 normalized activations take the registers
  constexpr int UNR = NORM ? 1 : 2;
#pragma unroll UNR
  for (int b = lane; b < nb; b += 64) {
    u32x4 wq[NPW];
    uint32_t se[NPW];
#pragma unroll
    for (int j = 0; j < NPW; ++j) {  // all loads of the iteration in flight together
      const int n = min(n0 + (GATED ? j % COLS : j), N - 1);
      const uint8_t* wb = (GATED && j >= COLS) ? f.q2 : w;
      const uint8_t* sb = (GATED && j >= COLS) ? f.s2 : s;
      wq[j] = *reinterpret_cast<const u32x4*>(wb + (int64_t)n * (K / 2) + b * 16);
      se[j] = sb[(int64_t)n * nb + b];
    }
    Vec16<__hip_bfloat16> gv[4];
    if constexpr (NORM) {
      if (f.g != nullptr) {
#pragma unroll
        for (int c = 0; c < 4; ++c) gv[c] = load16(f.g + b * 32 + c * 8);
      }
    }
#pragma unroll
    for (int m = 0; m < M; ++m) {
      // the block's 32 activations of row m (bf16 pairs), then every column's scaled conversion
      const __hip_bfloat16* xr = x + (int64_t)m * ldx + b * 32;
      float xf[32];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const Vec16<__hip_bfloat16> xv = load16(xr + c * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) xf[c * 8 + e] = to_f32(xv.v[e]);
      }
      if constexpr (NORM) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float xn = xf[c * 8 + e] * rstd[m];
            xf[c * 8 + e] = to_f32(__float2bfloat16(f.g != nullptr ? xn * to_f32(gv[c].v[e]) : xn));
          }
      }
#pragma unroll
      for (int j = 0; j < NPW; ++j) {
        const float sc = e8m0_to_f32(se[j]);
        const uint32_t d[4] = {wq[j].x, wq[j].y, wq[j].z, wq[j].w};
        float a = acc[m][j];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
#define LTA_CVT(BS)                                                       \
  {                                                                       \
    const f2 v = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(d[q], sc, BS);   \
    a = fmaf(xf[q * 8 + BS * 2], v.x, a);                                 \
    a = fmaf(xf[q * 8 + BS * 2 + 1], v.y, a);                             \
  }
          LTA_CVT(0) LTA_CVT(1) LTA_CVT(2) LTA_CVT(3)
#undef LTA_CVT
        }
        acc[m][j] = a;
      }
    }
  }
  if constexpr (FUSED) {
    // the butterfly leaves every sum in every lane: lane m * COLS + j keeps output (m, j), so the
    // epilogue's bias / residual loads and stores run once, in parallel, not once per output
    float mine = 0.f, gate = 0.f;
#pragma unroll
    for (int m = 0; m < M; ++m) {
#pragma unroll
      for (int j = 0; j < COLS; ++j) {
        const float a = wave_sum(acc[m][j]);
        if (lane == m * COLS + j) mine = a;
        if constexpr (GATED) {
          const float b = wave_sum(acc[m][j + COLS]);
          if (lane == m * COLS + j) gate = b;
        }
      }
    }
    const int m = lane / COLS, n = n0 + lane % COLS;
    if (lane < M * COLS && n < N) {
      float o;
      if constexpr (GATED) {
        o = mx4_act(to_f32(__float2bfloat16(mine)), f.act) * to_f32(__float2bfloat16(gate));
      } else {
        o = mx4_act(mine + (bias != nullptr ? to_f32(bias[n]) : 0.f), f.act);
        if (f.res != nullptr) o += to_f32(f.res[(int64_t)m * f.ldr + n]);
      }
      y[(int64_t)m * ldy + n] = __float2bfloat16(o);
    }
  } else {
#pragma unroll
    for (int m = 0; m < M; ++m) {
#pragma unroll
      for (int j = 0; j < NPW; ++j) {
        const float v = wave_sum(acc[m][j]);
        if (lane == 0 && n0 + j < N) {
          const float bv = bias != nullptr ? to_f32(bias[n0 + j]) : 0.f;
          y[(int64_t)m * ldy + n0 + j] = __float2bfloat16(v + bv);
        }
      }
    }
  }
}

// One launch over the table's segments.  Wide waves (8 columns) from 8192 streamed weight rows up,
// as the plain entry point; NORM with more than 4 rows keeps 4 columns (the fp32 normalized
// activations of 5+ rows beside 8 columns' accumulators do not fit the register file).
template <bool NORM, bool GATED>
void launch_fused(const void* x, const void* bias, int M, int K, int ldx, Mx4Fused f, int nseg, hipStream_t stream) {
  int64_t rows = 0;
  for (int i = 0; i < nseg; ++i) rows += f.n[i];
  const bool wide = rows * (GATED ? 2 : 1) >= 8192 && !(NORM && M > 4);
  const int cols_per_wg = WAVES * (wide ? 8 : 4) / (GATED ? 2 : 1);
  int total = 0;
  for (int i = 0; i < nseg; ++i) {
    const int b = (f.n[i] + cols_per_wg - 1) / cols_per_wg;
    if (i < 2) f.blocks[i] = b;
    total += b;
  }
  for (int i = nseg; i < 2; ++i) f.blocks[i] = 1 << 30;
  dim3 grid(total), block(WAVES * 64);
#define LTA_F4(MM)                                                                                                \
  case MM:                                                                                                        \
    if (wide)                                                                                                     \
      hipLaunchKernelGGL((gemv_mxfp4_kernel<MM, (NORM && MM > 4) ? 4 : 8, NORM, GATED, true>), grid, block, 0, stream, \
                         (const __hip_bfloat16*)x, (const uint8_t*)nullptr, (const uint8_t*)nullptr,               \
                         (const __hip_bfloat16*)bias, (__hip_bfloat16*)nullptr, 0, K, ldx, 0, f);                  \
    else                                                                                                          \
      hipLaunchKernelGGL((gemv_mxfp4_kernel<MM, 4, NORM, GATED, true>), grid, block, 0, stream,                    \
                         (const __hip_bfloat16*)x, (const uint8_t*)nullptr, (const uint8_t*)nullptr,               \
                         (const __hip_bfloat16*)bias, (__hip_bfloat16*)nullptr, 0, K, ldx, 0, f);                  \
    break;
  switch (M) {
    LTA_F4(1) LTA_F4(2) LTA_F4(3) LTA_F4(4) LTA_F4(5) LTA_F4(6) LTA_F4(7) LTA_F4(8)
  }
#undef LTA_F4
}

bool mx4_operands_ok(const void* x, const void* g, int M, int K, int ldx) {
  if (M < 1 || M > MAXM || K < 32 || K % 32 || ldx % 8) return false;
  // x and the norm weight are read with 16-B vector loads
  return reinterpret_cast<uintptr_t>(x) % 16 == 0 && reinterpret_cast<uintptr_t>(g) % 16 == 0;
}

}  // namespace

// x [M, K] bf16 (row stride ldx), w [N, K/2] packed e2m1, s [N, K/32] E8M0 -> y [M, N] bf16 (ldy).
LTA_EXPORT int lta_gemv_mxfp4(const void* x, const void* w, const void* s, const void* bias, void* y, int M, int N,
                              int K, int ldx, int ldy, hipStream_t stream) {
  if (M < 1 || M > MAXM || K % 32 || ldx % 8) return -2;
  if (reinterpret_cast<uintptr_t>(x) % 16) return -2;  // x is read with 16-B vector loads
  // columns per wave: 8 amortise each activation load over more weight rows (the kernel is
  // bound by L1 traffic otherwise); 4 keep enough workgroups in flight for narrow outputs
  const bool wide = N >= 8192;
  const int cols_per_wg = WAVES * (wide ? 8 : 4);
  dim3 grid((N + cols_per_wg - 1) / cols_per_wg), block(WAVES * 64);
#define LTA_G4(MM)                                                                                             \
  case MM:                                                                                                     \
    if (wide)                                                                                                  \
      hipLaunchKernelGGL((gemv_mxfp4_kernel<MM, 8>), grid, block, 0, stream, (const __hip_bfloat16*)x,          \
                         (const uint8_t*)w, (const uint8_t*)s, (const __hip_bfloat16*)bias, (__hip_bfloat16*)y, N, K, \
                         ldx, ldy);                                                                            \
    else                                                                                                       \
      hipLaunchKernelGGL((gemv_mxfp4_kernel<MM, 4>), grid, block, 0, stream, (const __hip_bfloat16*)x,          \
                         (const uint8_t*)w, (const uint8_t*)s, (const __hip_bfloat16*)bias, (__hip_bfloat16*)y, N, K, \
                         ldx, ldy);                                                                            \
    break;
  switch (M) {
    LTA_G4(1) LTA_G4(2) LTA_G4(3) LTA_G4(4) LTA_G4(5) LTA_G4(6) LTA_G4(7) LTA_G4(8)
  }
#undef LTA_G4
  return (int)hipGetLastError();
}

// y [M, N] = act(x' . dequant(q, s)^T + bias) + res, or act(x' . dequant(q, s)^T) * (x' . dequant(q2, s2)^T)
// with a gate weight (no bias / residual then); x' = x or rmsnorm(x, g, eps) (norm != 0, g may be null).
LTA_EXPORT int lta_gemv_mxfp4_fused(const void* x, const void* q, const void* s, const void* q2, const void* s2,
                                    const void* g, int norm, float eps, const void* bias, const void* res, void* y,
                                    int M, int N, int K, int ldx, int ldy, int ldr, int act, hipStream_t stream) {
  if (!mx4_operands_ok(x, norm ? g : nullptr, M, K, ldx) || N < 1) return -2;
  if ((q2 != nullptr) != (s2 != nullptr) || (q2 != nullptr && (bias != nullptr || res != nullptr))) return -2;
  if (act != 0 && act != 1 && act != 3 && act != 4) return -2;
  Mx4Fused f{};
  f.q[0] = (const uint8_t*)q;
  f.s[0] = (const uint8_t*)s;
  f.y[0] = (__hip_bfloat16*)y;
  f.n[0] = N;
  f.ldy[0] = ldy;
  f.q2 = (const uint8_t*)q2;
  f.s2 = (const uint8_t*)s2;
  f.g = norm ? (const __hip_bfloat16*)g : nullptr;
  f.res = (const __hip_bfloat16*)res;
  f.ldr = ldr;
  f.act = act;
  f.eps = eps;
  if (norm && q2) launch_fused<true, true>(x, bias, M, K, ldx, f, 1, stream);
  else if (norm) launch_fused<true, false>(x, bias, M, K, ldx, f, 1, stream);
  else if (q2) launch_fused<false, true>(x, bias, M, K, ldx, f, 1, stream);
  else launch_fused<false, false>(x, bias, M, K, ldx, f, 1, stream);
  return (int)hipGetLastError();
}

// Grouped decode projections: y_i [M, N_i] = x' . dequant(q_i, s_i)^T for i < nseg (<= 3) in one
// launch, x' as above; y_i has row stride ldy_i (adjacent column ranges of one buffer when packed).
LTA_EXPORT int lta_gemv_mxfp4_group(const void* x, const void* g, int norm, float eps, int nseg,
                                    const void* const* qs, const void* const* ss, void* const* ys, const int* ns,
                                    const int* ldys, int M, int K, int ldx, hipStream_t stream) {
  if (!mx4_operands_ok(x, norm ? g : nullptr, M, K, ldx) || nseg < 1 || nseg > 3) return -2;
  Mx4Fused f{};
  for (int i = 0; i < nseg; ++i) {
    if (ns[i] < 1) return -2;
    f.q[i] = (const uint8_t*)qs[i];
    f.s[i] = (const uint8_t*)ss[i];
    f.y[i] = (__hip_bfloat16*)ys[i];
    f.n[i] = ns[i];
    f.ldy[i] = ldys[i];
  }
  f.g = norm ? (const __hip_bfloat16*)g : nullptr;
  f.eps = eps;
  if (norm) launch_fused<true, false>(x, nullptr, M, K, ldx, f, nseg, stream);
  else launch_fused<false, false>(x, nullptr, M, K, ldx, f, nseg, stream);
  return (int)hipGetLastError();
}
