// linear_rhs.hip — the output GEMM of the GAT layer's value projection
// (mix_features: ax = (A_mean (x W)) Wout, reference src/function_GAT_attention.py:38)
// fused with the RHS epilogue f = a*(ax - x) [+ b*x0] (:60-68) and the Runge-Kutta
// stage combination of the fixed-grid solvers: ax never makes a round trip
// through memory and no separate epilogue pass runs.
//
// Fast path (K % 16 == 0, K <= 128, C % 4 == 0, 16-byte aligned rows):
// linear_rhs_split_kernel, the split-bf16 product of linear_split_kernel
// (linear.hip: three exact bf16 pieces per f32 operand, six
// v_mfma_f32_32x32x16_bf16 products per step, smallest first — f32-GEMM accuracy).
// The product is formed transposed, D = Wt z^T, so a lane ends with 16-byte runs of
// ITS row's outputs; the epilogue reads the same runs of x, x0 and the stage
// operands (x and x0 of an accumulator tile's four runs together) and stores the same
// runs (epi_prefetch / epi_finish of common.hpp: the arithmetic K1 and
// gnpde_stage_apply_* share, so the fused stage equals f followed by the stage pass
// bit for bit).  blockIdx.y walks 64-column slices of the output (two accumulator
// tiles per wavefront); persistent wavefronts walk 32-row
// tiles, the next tile's z rows refilled behind the matrix work as in linear.hip.
//
// Every other shape: linear_rhs_plain_kernel, one exact-f32 fma chain per output
// element and the same epilogue helpers (correctness only).
// No atomics, fixed summation orders: repeated launches give the same bits.
#include <algorithm>

#include "linear_split.hpp"
#include "rhs_host.hpp"

namespace gnpde {

// Accumulator tiles (32 output columns each) per wavefront: 64-column slices over
// blockIdx.y, as the projection; z is re-read once per slice.  Measured and dropped: a
// wavefront keeping 128 columns (four tiles: 32 more accumulator registers, twice the W
// fragments in LDS, so K <= 64 only at two workgroups per CU) — G-arxiv, K = 64, C = 128:
// 0.0874 / 0.0857 ms against 0.0879 / 0.0874 ms, inside the sample-to-sample difference
// (DESIGN.md §6.15).
constexpr int kLrhsTiles = 2;

// STG: 0 stores f, 2 the fixed-grid stage epilogue (up to two outputs and kStagePre
// operands, streamed after the product: common.hpp).  Measured and dropped: reading
// every stage operand row of a (half) accumulator tile before combining any run
// (wide_combine taking pre-read rows by slot): 170-226 VGPRs, the fused rk4 stage on
// G-arxiv at 0.219-0.239 ms, unchanged from 0.213-0.244 ms.
// BIAS: ax = z Wt^T + bias[C] ahead of the epilogue (gnpde_linear_rhs_bias_f32: the transformer
// layer's Wout, an nn.Linear with a bias); the BIAS = false instantiation never reads `bias`.
template <int KS, int STG, bool BIAS>
__global__ __launch_bounds__(256, 2) void linear_rhs_split_kernel(const float* __restrict__ z, int R, int64_t ldz,
                                                                   const float* __restrict__ Wt, int C, Epi e,
                                                                   const float* __restrict__ bias) {
  constexpr int K = 16 * KS, KH = 8 * KS;
  extern __shared__ __attribute__((aligned(16))) bf16x8_t wfrag[];  // [tile][piece 3][step KS][lane 64]
  constexpr int NT = kLrhsTiles;
  const int col0 = blockIdx.y * (32 * NT);
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  const int r32 = lane & 31, h = lane >> 5;
  const int ntiles = (R + kLinRowsPerWave - 1) / kLinRowsPerWave;
  const int step = gridDim.x * kWavesPerBlock;
  int tile = blockIdx.x * kWavesPerBlock + wv;

  // the wave's first tile goes out before the W staging
  float4 xa[2 * KS];
  {
    const float* __restrict__ zr =
        z + (int64_t)min(min(tile, ntiles - 1) * kLinRowsPerWave + r32, R - 1) * ldz + h * KH;
#pragma unroll
    for (int i = 0; i < 2 * KS; ++i) xa[i] = lin_load4<float>(zr + 4 * i);
  }
  for (int el = threadIdx.x; el < NT * KS * kWave; el += kBlock) {
    const int t = el / (KS * kWave), s = (el / kWave) % KS, l = el % kWave;
    const int n = col0 + 32 * t + (l & 31);
    float4 lo = make_float4(0.f, 0.f, 0.f, 0.f), hi = lo;
    if (n < C) {
      const float* wr = Wt + (int64_t)n * K + (l >> 5) * KH + 8 * s;
      lo = *reinterpret_cast<const float4*>(wr);
      hi = *reinterpret_cast<const float4*>(wr + 4);
    }
    bf16x8_t p0, p1, p2;
    split3(lo, hi, p0, p1, p2);
    wfrag[((t * 3 + 0) * KS + s) * kWave + l] = p0;
    wfrag[((t * 3 + 1) * KS + s) * kWave + l] = p1;
    wfrag[((t * 3 + 2) * KS + s) * kWave + l] = p2;
  }
  __syncthreads();
  if (tile >= ntiles) return;

  const bool need_x = (e.flags & GNPDE_EPI_RHS) != 0;
  const float a = need_x ? epi_alpha(e) : 0.f;
  const float b = (e.flags & GNPDE_ADD_SOURCE) ? *e.beta : 0.f;

  for (; tile < ntiles; tile += step) {
    const int nt = min(tile + step, ntiles - 1);  // clamped: the last pass re-reads a valid row
    const float* __restrict__ zn = z + (int64_t)min(nt * kLinRowsPerWave + r32, R - 1) * ldz + h * KH;
    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f32x16{0};
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      bf16x8_t a0, a1, a2;
      split3(xa[2 * s], xa[2 * s + 1], a0, a1, a2);
      // refill four steps at a time: the lane's 128-byte line of the next tile is
      // read by eight back-to-back loads (linear.hip)
      if (s % 4 == 3 || s == KS - 1) {
#pragma unroll
        for (int s2 = s - s % 4; s2 <= s; ++s2) {
          xa[2 * s2] = lin_load4<float>(zn + 8 * s2);
          xa[2 * s2 + 1] = lin_load4<float>(zn + 8 * s2 + 4);
        }
      }
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const bf16x8_t w0 = wfrag[((t * 3 + 0) * KS + s) * kWave + lane];
        const bf16x8_t w1 = wfrag[((t * 3 + 1) * KS + s) * kWave + lane];
        const bf16x8_t w2 = wfrag[((t * 3 + 2) * KS + s) * kWave + lane];
        // smallest products first
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w0, a2, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w1, a1, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w2, a0, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w0, a1, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w1, a0, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w0, a0, acc[t], 0, 0, 0);
      }
      // keep step s+1's refill behind step s+1's split (linear.hip)
      asm volatile("" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
    }
    // D = Wt z^T in the C layout: lane column = row r32 of the tile, register 4g + i =
    // output column 8g + 4h + i of accumulator tile t.  Per accumulator tile the four
    // runs' epilogue operands are read together, then combined and stored; a tile
    // wholly in range takes no per-lane branch.
    const int row = tile * kLinRowsPerWave + r32;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int n0 = col0 + 32 * t;  // wave-uniform
      if (n0 >= C) break;
      EpiPre<4, float, STG> p[4];
      if constexpr (BIAS) {  // the lane's four runs of this tile: columns n0 + 8g + 4h .. + 3
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int c = n0 + 8 * g + 4 * h;
          float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
          if (c < C) bv = *reinterpret_cast<const float4*>(bias + c);  // C % 4 == 0: a whole run
          acc[t][4 * g] += bv.x;
          acc[t][4 * g + 1] += bv.y;
          acc[t][4 * g + 2] += bv.z;
          acc[t][4 * g + 3] += bv.w;
        }
      }
      if (tile * kLinRowsPerWave + kLinRowsPerWave <= R && n0 + 32 <= C) {
#pragma unroll
        for (int g = 0; g < 4; ++g) epi_prefetch<4, STG, float>(e, row, n0 + 8 * g + 4 * h, p[g]);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const float ax[4] = {acc[t][4 * g], acc[t][4 * g + 1], acc[t][4 * g + 2], acc[t][4 * g + 3]};
          epi_finish<4, STG, float>(e, row, n0 + 8 * g + 4 * h, ax, a, b, p[g]);
        }
      } else {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int c = n0 + 8 * g + 4 * h;
          if (row < R && c < C) epi_prefetch<4, STG, float>(e, row, c, p[g]);
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int c = n0 + 8 * g + 4 * h;
          const float ax[4] = {acc[t][4 * g], acc[t][4 * g + 1], acc[t][4 * g + 2], acc[t][4 * g + 3]};
          if (row < R && c < C) epi_finish<4, STG, float>(e, row, c, ax, a, b, p[g]);
        }
      }
    }
  }
}

// Any K >= 1, C >= 1: one thread per output element, an exact-f32 fma chain over k
// ascending.
template <int STG, bool BIAS>
__global__ __launch_bounds__(256) void linear_rhs_plain_kernel(const float* __restrict__ z, int64_t R, int K,
                                                                int64_t ldz, const float* __restrict__ Wt, int C,
                                                                Epi e, const float* __restrict__ bias) {
  const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (idx >= R * C) return;
  const int64_t row = idx / C;
  const int c = (int)(idx - row * C);
  const float* __restrict__ zr = z + row * ldz;
  const float* __restrict__ wr = Wt + (int64_t)c * K;
  float ax[1] = {0.f};
  for (int k = 0; k < K; ++k) ax[0] = fmaf(zr[k], wr[k], ax[0]);
  if constexpr (BIAS) ax[0] += bias[c];
  const bool need_x = (e.flags & GNPDE_EPI_RHS) != 0;
  const float a = need_x ? epi_alpha(e) : 0.f;
  const float b = (e.flags & GNPDE_ADD_SOURCE) ? *e.beta : 0.f;
  epilogue_store<1, STG, float>(e, row, c, ax, a, b);
}

}  // namespace gnpde

using namespace gnpde;

template <bool BIAS>
static int linear_rhs_impl(const float* z, int64_t R, int64_t K, int64_t ldz, const float* Wt, int64_t C,
                           const float* bias, const float* x, int64_t ldx, const float* x0, int64_t ldx0,
                           const float* alpha, const float* beta, int flags, float* f, int64_t ldf,
                           const gnpde_stage_epilogue_t* stage, void* stream) {
  GNPDE_REQUIRE(z && Wt, GNPDE_EINVAL, "linear_rhs: NULL pointer");
  GNPDE_REQUIRE(R >= 0 && R < INT32_MAX && K >= 1 && K < INT32_MAX && ldz >= K && C >= 1 && C < INT32_MAX,
                GNPDE_EINVAL, "linear_rhs: bad sizes");
  GNPDE_REQUIRE(f || stage, GNPDE_EINVAL, "linear_rhs: NULL f");
  const bool rhs = (flags & GNPDE_EPI_RHS) != 0;
  GNPDE_REQUIRE(!rhs || x, GNPDE_EINVAL, "linear_rhs: NULL x");
  // (the plain product reads no x: the epilogue helpers never touch the stand-in)
  Epi e = make_epi(rhs ? x : z, rhs ? ldx : ldf, x0, ldx0, alpha, beta, flags, f, ldf, stage);
  int rc = check_epi(e, C, 0, nullptr, 0);
  if (rc) return rc;
  if (stage) {
    const gnpde_stage_epilogue_t& st = *stage;
    // the narrow (fixed-grid) stage epilogue only; the caller forms f and applies the others
    GNPDE_REQUIRE(!st.err_rows && !st.dot_rows && !st.dense_out && !st.dense_tab && !st.scale_rows && !st.out_rows &&
                      !st.coef_scale && st.f_lin == 0.f && st.nk <= kStagePre,
                  GNPDE_EUNSUPPORTED,
                  "linear_rhs: only the fixed-grid stage epilogue is fused (outputs, f_out, at most %d operands); "
                  "apply this stage with gnpde_stage_apply_*", kStagePre);
    // other lanes read whole rows of z, and x is the RHS input (include/gnpde.h)
    for (int i = 0; i < st.n_out; ++i)
      GNPDE_REQUIRE(st.o[i].out != z && !(rhs && st.o[i].out == x), GNPDE_EINVAL,
                    "linear_rhs: stage output %d aliases z or x", i);
    GNPDE_REQUIRE(st.f_out != z && !(rhs && st.f_out == x), GNPDE_EINVAL, "linear_rhs: f_out aliases z or x");
  } else {
    GNPDE_REQUIRE(f != z && !(rhs && f == x), GNPDE_EINVAL, "linear_rhs: f aliases z or x");
  }
  if (R == 0) return GNPDE_OK;
  hipStream_t s = as_stream(stream);

  auto row16 = [](const void* p, int64_t ld) { return p == nullptr || (aligned16(p) && ld % 4 == 0); };
  bool fast = K % 16 == 0 && K <= 128 && C % 4 == 0 && row16(z, ldz) && aligned16(Wt) && row16(f, ldf) && ldf % 4 == 0;
  if (BIAS) fast = fast && aligned16(bias);
  if (rhs) fast = fast && row16(x, ldx);
  if (flags & GNPDE_ADD_SOURCE) fast = fast && row16(x0, ldx0);
  if (stage) {
    fast = fast && aligned16(stage->f_out);
    for (int i = 0; i < stage->n_out; ++i) fast = fast && aligned16(stage->o[i].out) && aligned16(stage->o[i].base);
    for (int j = 0; j < stage->nk; ++j) fast = fast && aligned16(stage->k[j]);
  }
  if (fast) {
    // persistent tiles, the projection's wave budget (linear.hip)
    const int64_t ntiles = ceil_div(R, kLinRowsPerWave);
    const int64_t slices = ceil_div(C, 32 * kLrhsTiles);
    const int64_t max_waves = std::max<int64_t>(kWavesPerBlock, 2048 / slices);
    const int64_t per_wave = ceil_div(ntiles, max_waves);
    const int64_t blocks = ceil_div(ceil_div(ntiles, per_wave), kWavesPerBlock);
    const dim3 gt((unsigned)blocks, (unsigned)slices);
    const size_t lds = sizeof(bf16x8_t) * (size_t)kLrhsTiles * 3 * (size_t)(K / 16) * kWave;
#define GNPDE_LRHS_K(KS)                                                                                \
  do {                                                                                                  \
    if (stage)                                                                                          \
      linear_rhs_split_kernel<KS, 2, BIAS><<<gt, kBlock, lds, s>>>(z, (int)R, ldz, Wt, (int)C, e, bias); \
    else                                                                                                \
      linear_rhs_split_kernel<KS, 0, BIAS><<<gt, kBlock, lds, s>>>(z, (int)R, ldz, Wt, (int)C, e, bias); \
  } while (0)
    switch (K / 16) {
      case 1: GNPDE_LRHS_K(1); break;
      case 2: GNPDE_LRHS_K(2); break;
      case 3: GNPDE_LRHS_K(3); break;
      case 4: GNPDE_LRHS_K(4); break;
      case 5: GNPDE_LRHS_K(5); break;
      case 6: GNPDE_LRHS_K(6); break;
      case 7: GNPDE_LRHS_K(7); break;
      default: GNPDE_LRHS_K(8); break;
    }
#undef GNPDE_LRHS_K
    GNPDE_LAUNCH_CHECK();
    return GNPDE_OK;
  }
  const int64_t nblk = ceil_div(R * C, kBlock);
  GNPDE_REQUIRE(nblk < INT32_MAX, GNPDE_EUNSUPPORTED, "linear_rhs: %lld x %lld outputs exceed the plain kernel's grid",
                (long long)R, (long long)C);
  if (stage)
    linear_rhs_plain_kernel<2, BIAS><<<(unsigned)nblk, kBlock, 0, s>>>(z, R, (int)K, ldz, Wt, (int)C, e, bias);
  else
    linear_rhs_plain_kernel<0, BIAS><<<(unsigned)nblk, kBlock, 0, s>>>(z, R, (int)K, ldz, Wt, (int)C, e, bias);
  GNPDE_LAUNCH_CHECK();
  return GNPDE_OK;
}

extern "C" int gnpde_linear_rhs_f32(const float* z, int64_t R, int64_t K, int64_t ldz, const float* Wt, int64_t C,
                                    const float* x, int64_t ldx, const float* x0, int64_t ldx0, const float* alpha,
                                    const float* beta, int flags, float* f, int64_t ldf,
                                    const gnpde_stage_epilogue_t* stage, void* stream) {
  return linear_rhs_impl<false>(z, R, K, ldz, Wt, C, nullptr, x, ldx, x0, ldx0, alpha, beta, flags, f, ldf, stage,
                                stream);
}

// ax = z Wt^T + bias (the transformer layer's Wout, function_transformer_attention.py:31); bias NULL: the entry above
extern "C" int gnpde_linear_rhs_bias_f32(const float* z, int64_t R, int64_t K, int64_t ldz, const float* Wt,
                                         int64_t C, const float* bias, const float* x, int64_t ldx, const float* x0,
                                         int64_t ldx0, const float* alpha, const float* beta, int flags, float* f,
                                         int64_t ldf, const gnpde_stage_epilogue_t* stage, void* stream) {
  if (!bias)
    return linear_rhs_impl<false>(z, R, K, ldz, Wt, C, nullptr, x, ldx, x0, ldx0, alpha, beta, flags, f, ldf, stage,
                                  stream);
  return linear_rhs_impl<true>(z, R, K, ldz, Wt, C, bias, x, ldx, x0, ldx0, alpha, beta, flags, f, ldf, stage, stream);
}
