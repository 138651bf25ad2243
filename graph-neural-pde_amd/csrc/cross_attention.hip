// cross_attention.hip — the second modality's cross-attention (multi_modal,
// src/function_laplacian_diffusion.py:61-63 read as torch.softmax(..., dim=-1)):
//   out[b,n,:] = softmax_m(scale * <q[b,n,:], k[b,m,:]>) v[b,m,:]      (gnpde_cross_attention_f32)
// for q [B,N,C] (row stride ldq), k / v [B,M,C] contiguous, flash style: the [N, M] scores
// of a batch element never reach memory.
//
// A workgroup of 4 waves owns 128 query rows of ONE batch element (grid = B x ceil(N/128)),
// a wave 32 of them, q in registers.  The workgroup walks the M keys in tiles of 32: K and V
// rows are staged in LDS as fp32 ([key][CP + pad], CP = C rounded up to 32, zero beyond C and
// beyond M), the next tile's global loads issued before the current tile's arithmetic.
//
// Both products run on v_mfma_f32_32x32x2_f32 (exact fp32: a k-ordered fmaf chain).
//   S^T = K Q^T  (A = K: lane = key, B = Q^T: lane = query): the result has the QUERY on the
//     lane and 16 keys of the tile in its registers (keys crow(r) + 4 h, h = lane >> 5), so a
//     row's max and sum are in-register plus one exchange with lane ^ 32.
//   O^T += V^T P^T  (A = V^T: lane = channel, B = P^T: lane = query): register r of the score
//     tile is already the B operand of the k-step over keys (crow(r), crow(r) + 4), and O^T
//     keeps the query on the lane, so the online-softmax rescale is one factor per lane.
// O lives in ceil(C/32) accumulators.  No atomics and a fixed reduction order: the result
// does not depend on the launch geometry and two runs give the same bits.  lse (optional)
// = max + ln(sum exp) of the scaled scores, what a backward recomputes P from.
#include "linear_split.hpp"

namespace gnpde {

constexpr int kXaRowsPerWave = 32;                          // query rows of a wave
constexpr int kXaRows = kXaRowsPerWave * kWavesPerBlock;    // 128 of a workgroup
constexpr int kXaTile = 32;                                 // keys of a staged tile
constexpr int kXaMaxC = 256;
// LDS row strides (words): K is read with lane = key at a fixed column (stride = 2 mod 32:
// the 32 rows of a half wave fall on 32 distinct even banks, the other half on the odd ones);
// V with lane = channel, the two halves 4 rows apart (4 * stride = 32 mod 64)
constexpr int kXaPadK = 2;
constexpr int kXaPadV = 8;

__host__ __device__ constexpr int xa_lds_floats(int nc) {
  return kXaTile * (nc * 32 + kXaPadK) + kXaTile * (nc * 32 + kXaPadV);
}

// row of register r inside a 32x32 MFMA result, lane half 0 (half 1: + 4)
__device__ __forceinline__ constexpr int xa_crow(int r) { return (r & 3) + 8 * (r >> 2); }

template <int NC>
__global__ __launch_bounds__(kBlock) void cross_attention_kernel(const float* __restrict__ q, int64_t ldq,
                                                                 const float* __restrict__ k,
                                                                 const float* __restrict__ v, int N, int M, int C,
                                                                 int tiles_n, float scale, float* __restrict__ out,
                                                                 int64_t ldo, float* __restrict__ lse, int vec4) {
  constexpr int CP = NC * 32, LDK = CP + kXaPadK, LDV = CP + kXaPadV;
  constexpr int NLD = kXaTile * CP / kBlock;  // staged words of K (and of V) per thread
  extern __shared__ __attribute__((aligned(16))) float xa_lds[];
  float* Ks = xa_lds;                   // [kXaTile][LDK]
  float* Vs = xa_lds + kXaTile * LDK;   // [kXaTile][LDV]
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int r32 = lane & 31, h = lane >> 5;
  const int b = blockIdx.x / tiles_n;
  const int n0 = (blockIdx.x - b * tiles_n) * kXaRows + wave * kXaRowsPerWave;
  const bool wave_live = n0 < N;  // no early return: every wave stages and takes the barriers
  const int n = n0 + r32;
  const float* __restrict__ kb = k + (int64_t)b * M * C;
  const float* __restrict__ vb = v + (int64_t)b * M * C;

  // q of this lane's row: k-step s of the first product reads columns 2 s and 2 s + 1
  float qf[NC * 16];
  {
    const float* __restrict__ qr = q + ((int64_t)b * N + min(n, N - 1)) * ldq;
#pragma unroll
    for (int s = 0; s < NC * 16; ++s) {
      const int c = 2 * s + h;
      qf[s] = c < C ? qr[c] : 0.f;
    }
  }

  // staging: thread (tid >> 5, tid & 31) takes rows 8 i + (tid >> 5) and columns 32 cb + (tid & 31), so every
  // address is one per-thread base plus a wave-uniform or constant offset
  const int sr = tid >> 5, sc = tid & 31;
  float pk[NLD], pv[NLD];
  auto load = [&](int tile) {
    const int j0 = tile * kXaTile + sr;
    const int64_t base = (int64_t)j0 * C + sc;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int cb = 0; cb < NC; ++cb) {
        const bool ok = j0 + 8 * i < M && sc + 32 * cb < C;
        const int64_t off = base + (int64_t)(8 * i) * C + 32 * cb;
        pk[i * NC + cb] = ok ? kb[off] : 0.f;
        pv[i * NC + cb] = ok ? vb[off] : 0.f;
      }
    }
  };

  f32x16 o[NC];
#pragma unroll
  for (int cb = 0; cb < NC; ++cb) o[cb] = f32x16{0};
  const float ninf = -__builtin_inff();
  float m = ninf, l = 0.f;  // running max (common to the lane pair), this lane's part of the sum

  const int n_tiles = (M + kXaTile - 1) / kXaTile;
  load(0);
  for (int tile = 0; tile < n_tiles; ++tile) {
    __syncthreads();  // the previous tile's readers are done
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int cb = 0; cb < NC; ++cb) {
        Ks[(8 * i + sr) * LDK + 32 * cb + sc] = pk[i * NC + cb];
        Vs[(8 * i + sr) * LDV + 32 * cb + sc] = pv[i * NC + cb];
      }
    }
    __syncthreads();
    if (tile + 1 < n_tiles) load(tile + 1);
    if (!wave_live) continue;

    // S^T[key][query] = sum_c K[key][c] q[query][c]
    f32x16 s = f32x16{0};
    {
      const float* __restrict__ kp = Ks + r32 * LDK + h;
#pragma unroll
      for (int cb = 0; cb < NC; ++cb) {
#pragma unroll
        for (int t = cb * 16; t < cb * 16 + 16; ++t)
          s = __builtin_amdgcn_mfma_f32_32x32x2f32(kp[2 * t], qf[t], s, 0, 0, 0);
        // keep the LDS reads of a group next to its MFMAs: hoisted together they cost NC * 16 registers
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    const int j0 = tile * kXaTile;
    const bool full = j0 + kXaTile <= M;
    float mx = ninf;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float sv = s[r] * scale;
      if (!full) sv = j0 + xa_crow(r) + 4 * h < M ? sv : ninf;  // keys past M take no weight
      s[r] = sv;
      mx = fmaxf(mx, sv);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    // every tile holds a key below M, so m_new is finite; the first tile rescales by exp(-inf) = 0
    const float m_new = fmaxf(m, mx);
    const float alpha = expf(m - m_new);
    m = m_new;
    float ps = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float p = expf(s[r] - m_new);
      s[r] = p;
      ps += p;
    }
    l = l * alpha + ps;
    // O^T[c][query] = alpha O^T + sum_key V[key][c] P[query][key]
    const float* __restrict__ vp = Vs + 4 * h * LDV + r32;
#pragma unroll
    for (int cb = 0; cb < NC; ++cb) {
      o[cb] *= alpha;
#pragma unroll
      for (int r = 0; r < 16; ++r)
        o[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(vp[xa_crow(r) * LDV + cb * 32], s[r], o[cb], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
  }

  if (!wave_live) return;
  const float l_tot = l + __shfl_xor(l, 32);  // the two halves' sums (a + b = b + a: the same bits in both)
  if (n >= N) return;
  float* __restrict__ orow = out + ((int64_t)b * N + n) * ldo;
#pragma unroll
  for (int cb = 0; cb < NC; ++cb) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int c = cb * 32 + 8 * g + 4 * h;  // registers 4 g .. 4 g + 3: four consecutive channels
      if (c >= C) continue;
      const float4 w = make_float4(o[cb][4 * g] / l_tot, o[cb][4 * g + 1] / l_tot, o[cb][4 * g + 2] / l_tot,
                                   o[cb][4 * g + 3] / l_tot);
      if (vec4) {  // C % 4 == 0: the four are below C
        *reinterpret_cast<float4*>(orow + c) = w;
      } else {
        orow[c] = w.x;
        if (c + 1 < C) orow[c + 1] = w.y;
        if (c + 2 < C) orow[c + 2] = w.z;
        if (c + 3 < C) orow[c + 3] = w.w;
      }
    }
  }
  if (lse && h == 0) lse[(int64_t)b * N + n] = m + logf(l_tot);
}

template <int NC>
static int launch_cross_attention(const float* q, int64_t ldq, const float* k, const float* v, int64_t B, int64_t N,
                                  int64_t M, int64_t C, float scale, float* out, int64_t ldo, float* lse,
                                  hipStream_t st) {
  constexpr size_t lds = sizeof(float) * (size_t)xa_lds_floats(NC);
  if constexpr (lds > 64 * 1024) {
    // above the default dynamic LDS limit (C > 224: 65.3 KiB of the 160 KiB)
    static const hipError_t attr =
        hipFuncSetAttribute(reinterpret_cast<const void*>(&cross_attention_kernel<NC>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    GNPDE_HIP(attr);
  }
  const int64_t tiles_n = ceil_div(N, kXaRows);
  const int vec4 = C % 4 == 0 && ldo % 4 == 0 && aligned16(out);
  cross_attention_kernel<NC><<<dim3((unsigned)(B * tiles_n)), kBlock, lds, st>>>(q, ldq, k, v, (int)N, (int)M, (int)C,
                                                                                 (int)tiles_n, scale, out, ldo, lse,
                                                                                 vec4);
  GNPDE_LAUNCH_CHECK();
  return GNPDE_OK;
}

}  // namespace gnpde

using namespace gnpde;

extern "C" {

int gnpde_cross_attention_f32(const float* q, int64_t ldq, const float* k, const float* v, int64_t B, int64_t N,
                              int64_t M, int64_t C, float scale, float* out, int64_t ldo, float* lse, void* stream) {
  GNPDE_REQUIRE(B >= 0 && N >= 0, GNPDE_EINVAL, "cross_attention: B=%lld, N=%lld must be >= 0", (long long)B,
                (long long)N);
  GNPDE_REQUIRE(C >= 1, GNPDE_EINVAL, "cross_attention: C=%lld must be >= 1", (long long)C);
  GNPDE_REQUIRE(M >= 1, GNPDE_EINVAL, "cross_attention: M=%lld must be >= 1 (a softmax over no keys)", (long long)M);
  GNPDE_REQUIRE(ldq >= C && ldo >= C, GNPDE_EINVAL, "cross_attention: ldq=%lld, ldo=%lld must be >= C=%lld",
                (long long)ldq, (long long)ldo, (long long)C);
  GNPDE_REQUIRE(C <= kXaMaxC, GNPDE_EUNSUPPORTED, "cross_attention: C=%lld outside the kernel's range (1 <= C <= %d)",
                (long long)C, kXaMaxC);
  GNPDE_REQUIRE(N < INT32_MAX - kXaRows && M < INT32_MAX - kXaTile, GNPDE_EUNSUPPORTED,
                "cross_attention: N=%lld / M=%lld beyond 32-bit row indices", (long long)N, (long long)M);
  GNPDE_REQUIRE(B * ceil_div(N, kXaRows) <= INT32_MAX, GNPDE_EUNSUPPORTED,
                "cross_attention: B=%lld x ceil(N=%lld / %d) workgroups exceed the grid", (long long)B, (long long)N,
                kXaRows);
  if (B * N == 0) return GNPDE_OK;
  GNPDE_REQUIRE(q && k && v && out, GNPDE_EINVAL, "cross_attention: NULL q / k / v / out");
  hipStream_t st = as_stream(stream);
  switch ((int)ceil_div(C, 32)) {
    case 1: return launch_cross_attention<1>(q, ldq, k, v, B, N, M, C, scale, out, ldo, lse, st);
    case 2: return launch_cross_attention<2>(q, ldq, k, v, B, N, M, C, scale, out, ldo, lse, st);
    case 3: return launch_cross_attention<3>(q, ldq, k, v, B, N, M, C, scale, out, ldo, lse, st);
    case 4: return launch_cross_attention<4>(q, ldq, k, v, B, N, M, C, scale, out, ldo, lse, st);
    case 5: return launch_cross_attention<5>(q, ldq, k, v, B, N, M, C, scale, out, ldo, lse, st);
    case 6: return launch_cross_attention<6>(q, ldq, k, v, B, N, M, C, scale, out, ldo, lse, st);
    case 7: return launch_cross_attention<7>(q, ldq, k, v, B, N, M, C, scale, out, ldo, lse, st);
    default: return launch_cross_attention<8>(q, ldq, k, v, B, N, M, C, scale, out, ldo, lse, st);
  }
}

}  // extern "C"
