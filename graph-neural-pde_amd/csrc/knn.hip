// knn.hip — exact k nearest neighbours of the node embeddings (gnpde.graph_rewiring;
// src/graph_rewiring.py:122-161, the reference's pykeops argKmin): for every row of
// x [B, N, C] the k rows of the same graph with the smallest squared distance
// d_ij = sum_c (x_ic - x_jc)^2 (fp32, the difference form), in ascending (d_ij, j)
// (gnpde_knn_f32).
//
// Two launches.  The mask pre-pass marks the rows that are all zero or hold a
// non-finite value (never a candidate; as a query they return themselves) and counts
// the others per graph.  The main kernel gives one workgroup a tile of 64 queries of
// one graph and lets it scan all N candidates of that graph in tiles of 128: there is
// no merge across workgroups, so the result does not depend on the launch geometry.
// The distance tile and the selection are those of knn_tile.hpp (shared with posdist.hip).
#include "knn_tile.hpp"

namespace gnpde {

// masked[b*N + r] = 1 when row r of graph b is all zero or holds a non-finite value;
// n_valid[b] (zeroed by the caller) += the other rows.  One wave per row, 8 rows a wave.
__global__ __launch_bounds__(kBlock) void knn_mask_kernel(const float* __restrict__ x, int N, int C, int64_t ld,
                                                          uint8_t* __restrict__ masked, int* n_valid) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int b = blockIdx.y;
  const int64_t r0 = ((int64_t)blockIdx.x * kWavesPerBlock + wave) * kKnnMaskRows;
  int cnt = 0;
  for (int t = 0; t < kKnnMaskRows; ++t) {
    const int64_t r = r0 + t;
    if (r >= N) break;
    const float* xr = x + ((int64_t)b * N + r) * ld;
    bool nonzero = false, bad = false;
    for (int c = lane; c < C; c += kWave) {
      const unsigned u = __float_as_uint(xr[c]);
      nonzero |= (u << 1) != 0u;
      bad |= (u & 0x7f800000u) == 0x7f800000u;
    }
    const bool m = __ballot(bad) != 0ull || __ballot(nonzero) == 0ull;
    if (lane == 0) masked[(int64_t)b * N + r] = m ? 1 : 0;
    cnt += m ? 0 : 1;
  }
  if (lane == 0 && cnt) atomicAdd(n_valid + b, cnt);
}

// The kernel of gnpde_knn_f32 keeps its own, monolithic form of knn_tile.hpp's tile loop and
// filter (the same statements; the helpers are the header's).  Written over dist_tile_sweep
// and a functor, as pos_knn_kernel is, the same code allocates 268 - 277 registers where this
// form takes 249: under 256 it runs two waves per SIMD, above it one.
__global__ __launch_bounds__(kBlock) void knn_kernel(const float* __restrict__ x, int N, int C, int64_t ld, int k,
                                                     const uint8_t* __restrict__ masked,
                                                     int* __restrict__ idx_out, float* __restrict__ dist_out) {
  __shared__ __align__(16) float stage[kKnnTQ * kKnnTJ];                      // chunks, then the distance tile
  __shared__ __align__(16) unsigned long long list[kKnnTQ * kKnnMaxK];        // [query][rank]
  float* Qs = stage;                         // [kKnnCK][kKnnLDQ]
  float* Cs = stage + kKnnCK * kKnnLDQ;      // [kKnnCK][kKnnLDC]
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int b = blockIdx.y;
  const int q0 = blockIdx.x * kKnnTQ;
  const float* xb = x + (int64_t)b * N * ld;
  const uint8_t* mb = masked + (int64_t)b * N;
  const int tq = tid >> 4, tj = tid & 15;    // queries 4 tq .. +3; candidates 4 tj .. +3 and 64 + 4 tj .. +3
  const int n_tiles = (N + kKnnTJ - 1) / kKnnTJ;
  const int n_chunks = (C + kKnnCK - 1) / kKnnCK;

  for (int i = tid; i < kKnnTQ * kKnnMaxK; i += kBlock) list[i] = kKnnNone;
  // the wave's queries that take part: in range and unmasked (bit i: query wave * 16 + i)
  unsigned q_live;
  {
    const int qr = q0 + wave * kKnnQPerWave + lane;
    const bool live = lane < kKnnQPerWave && qr < N && mb[qr] == 0;
    q_live = (unsigned)__ballot(live);
  }

  float pq[kKnnQLoads], pc[kKnnCLoads];
  auto load = [&](int tile, int ch) {
    const int c0 = ch * kKnnCK, j0 = tile * kKnnTJ;
#pragma unroll
    for (int i = 0; i < kKnnQLoads; ++i) {
      const int e = tid + kBlock * i;
      const int c = c0 + ((e >> 10) << 4) + (e & 15), r = q0 + ((e >> 4) & (kKnnTQ - 1));
      pq[i] = (r < N && c < C) ? xb[(int64_t)r * ld + c] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < kKnnCLoads; ++i) {
      const int e = tid + kBlock * i;
      const int c = c0 + ((e >> 11) << 4) + (e & 15), r = j0 + ((e >> 4) & (kKnnTJ - 1));
      pc[i] = (r < N && c < C) ? xb[(int64_t)r * ld + c] : 0.f;
    }
  };

  float acc[4][8];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[a][c] = 0.f;

  load(0, 0);
  bool cand_ok0 = false, cand_ok1 = false;
  for (int tile = 0; tile < n_tiles; ++tile) {
    for (int ch = 0; ch < n_chunks; ++ch) {
      __syncthreads();  // the staging area's readers (the previous chunk, the previous tile's selection) are done
#pragma unroll
      for (int i = 0; i < kKnnQLoads; ++i) {
        const int e = tid + kBlock * i;
        Qs[(((e >> 10) << 4) + (e & 15)) * kKnnLDQ + ((e >> 4) & (kKnnTQ - 1))] = pq[i];
      }
#pragma unroll
      for (int i = 0; i < kKnnCLoads; ++i) {
        const int e = tid + kBlock * i;
        Cs[(((e >> 11) << 4) + (e & 15)) * kKnnLDC + ((e >> 4) & (kKnnTJ - 1))] = pc[i];
      }
      __syncthreads();
      if (ch == 0) {  // lane = candidate of each half tile: in range and unmasked
        const int j = tile * kKnnTJ + lane;
        cand_ok0 = j < N && mb[j] == 0;
        cand_ok1 = j + kWave < N && mb[j + kWave] == 0;
      }
      if (ch + 1 < n_chunks) load(tile, ch + 1);
      else if (tile + 1 < n_tiles) load(tile + 1, 0);
      auto column = [&](int c) {
        const float4 qv = *reinterpret_cast<const float4*>(Qs + c * kKnnLDQ + 4 * tq);
        const float4 ca = *reinterpret_cast<const float4*>(Cs + c * kKnnLDC + 4 * tj);
        const float4 cb = *reinterpret_cast<const float4*>(Cs + c * kKnnLDC + kWave + 4 * tj);
        const float qa[4] = {qv.x, qv.y, qv.z, qv.w};
        const float cv[8] = {ca.x, ca.y, ca.z, ca.w, cb.x, cb.y, cb.z, cb.w};
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float df = qa[a] - cv[j];
            acc[a][j] = fmaf(df, df, acc[a][j]);
          }
      };
      const int cols = C - ch * kKnnCK;
      if (cols >= kKnnCK) {
#pragma unroll 4
        for (int c = 0; c < kKnnCK; ++c) column(c);
      } else {  // a short last chunk: its columns only
#pragma unroll 1
        for (int c = 0; c < cols; ++c) column(c);
      }
    }
    __syncthreads();  // the last chunk's reads are done: the distance tile takes the staging area
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      float* dr = stage + (4 * tq + a) * kKnnTJ + 4 * tj;
      *reinterpret_cast<float4*>(dr) = make_float4(acc[a][0], acc[a][1], acc[a][2], acc[a][3]);
      *reinterpret_cast<float4*>(dr + kWave) = make_float4(acc[a][4], acc[a][5], acc[a][6], acc[a][7]);
#pragma unroll
      for (int c = 0; c < 8; ++c) acc[a][c] = 0.f;
    }
    __syncthreads();
    // filter: bit 2 i + h set when a candidate of half h passes query i's k-th key
    const int j0 = tile * kKnnTJ + lane;
    unsigned hits = 0;
#pragma unroll
    for (int i = 0; i < kKnnQPerWave; ++i) {
      const int q = wave * kKnnQPerWave + i;
      const unsigned long long thr = list[q * kKnnMaxK + k - 1];
      const unsigned long long k0 = knn_key(stage[q * kKnnTJ + lane], j0, cand_ok0);
      const unsigned long long k1 = knn_key(stage[q * kKnnTJ + kWave + lane], j0 + kWave, cand_ok1);
      hits |= (__ballot(k0 < thr) != 0ull ? 1u : 0u) << (2 * i);
      hits |= (__ballot(k1 < thr) != 0ull ? 2u : 0u) << (2 * i);
    }
    while (hits) {
      const int bit = __ffs((int)hits) - 1;
      hits &= hits - 1;
      const int i = bit >> 1, h = bit & 1;
      if (!((q_live >> i) & 1u)) continue;
      const int q = wave * kKnnQPerWave + i;
      const unsigned long long key =
          knn_key(stage[q * kKnnTJ + h * kWave + lane], j0 + h * kWave, h ? cand_ok1 : cand_ok0);
      knn_merge(list + q * kKnnMaxK, key, k, lane);
    }
  }
  __syncthreads();
  for (int i = 0; i < kKnnQPerWave; ++i) {
    const int q = wave * kKnnQPerWave + i, qr = q0 + q;
    if (qr >= N || lane >= k) continue;
    int j;
    float d;
    if (!((q_live >> i) & 1u)) {  // a masked query: itself, k times
      j = qr;
      d = 0.f;
    } else {
      const unsigned long long key = list[q * kKnnMaxK + lane];
      j = key == kKnnNone ? -1 : (int)(unsigned)key;   // fewer than k unmasked rows: -1 / +inf
      d = key == kKnnNone ? __uint_as_float(0x7f800000u) : __uint_as_float((unsigned)(key >> 32));
    }
    const int64_t o = ((int64_t)b * N + qr) * k + lane;
    idx_out[o] = j;
    if (dist_out) dist_out[o] = d;
  }
}

}  // namespace gnpde

using namespace gnpde;

extern "C" {

size_t gnpde_knn_workspace_bytes(int64_t B, int64_t N) {
  if (B <= 0 || N <= 0) return 16;
  return ((size_t)B * (size_t)N + 15) & ~(size_t)15;
}

int gnpde_knn_f32(const float* x, int64_t B, int64_t N, int64_t C, int64_t ld, int64_t k, int32_t* idx_out,
                  float* dist_out, int32_t* n_valid, void* workspace, void* stream) {
  GNPDE_REQUIRE(B >= 0 && B <= 65535, GNPDE_EINVAL, "knn: B=%lld must be in [0, 65535]", (long long)B);
  GNPDE_REQUIRE(N >= 0 && N < INT32_MAX - 2 * kKnnTJ, GNPDE_EINVAL, "knn: N=%lld out of range", (long long)N);
  GNPDE_REQUIRE(C >= 1 && C <= ld && C < INT32_MAX - kKnnCK, GNPDE_EINVAL, "knn: C=%lld must be in [1, ld=%lld]",
                (long long)C, (long long)ld);
  GNPDE_REQUIRE(k >= 1, GNPDE_EINVAL, "knn: k=%lld must be >= 1", (long long)k);
  GNPDE_REQUIRE(B * N == 0 || (x && idx_out && n_valid && workspace), GNPDE_EINVAL,
                "knn: NULL x / idx_out / n_valid / workspace");
  GNPDE_REQUIRE(k <= kKnnMaxK, GNPDE_EUNSUPPORTED, "knn: k=%lld outside the kernel's range (1 <= k <= %d)",
                (long long)k, kKnnMaxK);
  if (B * N == 0) return GNPDE_OK;
  hipStream_t st = as_stream(stream);
  uint8_t* masked = static_cast<uint8_t*>(workspace);
  GNPDE_HIP(hipMemsetAsync(n_valid, 0, sizeof(int32_t) * (size_t)B, st));
  const dim3 mgrid((unsigned)ceil_div(N, kWavesPerBlock * kKnnMaskRows), (unsigned)B);
  knn_mask_kernel<<<mgrid, kBlock, 0, st>>>(x, (int)N, (int)C, ld, masked, n_valid);
  GNPDE_LAUNCH_CHECK();
  const dim3 grid((unsigned)ceil_div(N, kKnnTQ), (unsigned)B);
  knn_kernel<<<grid, kBlock, 0, st>>>(x, (int)N, (int)C, ld, (int)k, masked, idx_out, dist_out);
  GNPDE_LAUNCH_CHECK();
  return GNPDE_OK;
}

}  // extern "C"
