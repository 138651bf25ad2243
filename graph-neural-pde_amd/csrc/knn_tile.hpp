// knn_tile.hpp — the distance tile and the exact top-k selection that knn.hip (the kNN of the
// node embeddings) and posdist.hip (the kNN, the rank select and the edge list of the
// positional-encoding distances) share.
//
// Distance tile: an "SGEMM with (a - b)^2 in place of a * b".  A workgroup owns a tile of 64
// rows and sweeps column tiles of 128.  Chunks of 32 columns of the query and the candidate
// rows are staged transposed in LDS ([column][row], rows padded by 4 words: the 16-column x
// 2-row store pattern of a half wave is then 2-way on the 32 store banks, which costs nothing,
// and the per-lane row reads are whole 16-byte slots); a thread accumulates 4 queries x 8
// candidates from three ds_read_b128 per column.  The next chunk's global loads are issued
// before the current chunk's arithmetic.  The last chunk is zero-padded on both sides, so
// padding adds exactly 0; a short last chunk walks only its own columns.  d_ij is an fma chain
// over c ascending whatever the tile: d_ij and d_ji square the same differences in the same
// order and are bit-equal, and the bits do not depend on which workgroup computes them.
//
// Selection: a query's current k smallest keys, sorted, live in LDS, one per lane of the
// wave that owns the query; a key is (float bits of d) << 32 | j, and since d >= 0 the
// unsigned integer order of the keys is the (d, j) order.  After a candidate tile its
// 64 x 128 distances go to LDS (over the staging area), and every wave tests its 16
// queries against their k-th key with lane = candidate: one compare and a ballot per
// (query, half tile), without a branch, so the LDS reads pipeline.  Past the first
// tiles almost no ballot is non-zero; those that are take a rank merge (every survivor
// and every list entry computes its place in the union from ballots and writes itself
// there), O(survivors) steps.  Masked candidates and the j >= N tail carry ~0.
#pragma once
#include "common.hpp"

namespace gnpde {

constexpr int kKnnTQ = 64;            // queries of a workgroup
constexpr int kKnnTJ = 128;           // candidates of a tile (two halves of one wave each)
constexpr int kKnnCK = 32;            // columns of a staged chunk
constexpr int kKnnLDQ = kKnnTQ + 4;   // LDS row strides of the transposed chunks (words)
constexpr int kKnnLDC = kKnnTJ + 4;
constexpr int kKnnMaxK = 64;          // one list entry per lane
constexpr int kKnnQPerWave = kKnnTQ / kWavesPerBlock;  // 16 queries owned by a wave
constexpr int kKnnQLoads = kKnnTQ * kKnnCK / kBlock;   // 8 staged words of the queries per thread
constexpr int kKnnCLoads = kKnnTJ * kKnnCK / kBlock;   // 16 of the candidates
constexpr int kKnnMaskRows = 8;       // rows a wave of the pre-pass walks
constexpr unsigned long long kKnnNone = ~0ull;

static_assert(kKnnCK * (kKnnLDQ + kKnnLDC) <= kKnnTQ * kKnnTJ, "the distance tile covers the staging area");

// What pos_knn_kernel selects on and what it reports: the rank value u of a metric (pair_u),
// reported as the distance D(u).  (kKnnRaw, key d and dist_out d, is gnpde_knn_f32's contract:
// knn.hip keeps that kernel in its own form, see there.)
constexpr int kKnnRaw = 0;       // key d, dist_out d
constexpr int kKnnEuclid = 1;    // key u = d (r = 1), dist_out sqrt(u)
constexpr int kKnnPoincare = 2;  // key u = d r_i r_j, dist_out arccosh(1 + 2 u)

// The rank value of a pair: u_ij = d_ij (r_i r_j), r = 1 / max(1 - |x|^2, eps) for the Poincare
// ball and r = 1 for the Euclidean metric (d * 1 is d).  Both metrics' distances are monotone
// in u.  EVERY kernel that ranks, counts or emits pairs takes u from this one function, on a d
// from dist_tile_sweep: the product r_i r_j commutes, so u_ij and u_ji are bit-equal, and the
// rank select, the count pass and the fill pass of posdist.hip see the same bits for a pair.
__device__ __forceinline__ float pair_u(float d, float ri, float rj) { return d * (ri * rj); }

// The distance of a rank value
template <int OUT>
__device__ __forceinline__ float pair_dist(float u) {
  if constexpr (OUT == kKnnEuclid) return sqrtf(u);
  // arccosh(1 + 2u) = log1p(2u + 2 sqrt(u (u + 1))): no cancellation at small u.  Past 2^40 (pairs
  // with a row at or outside the rim, r up to 2^52) u (u + 1) would leave fp32's range; there
  // arccosh(1 + 2u) = log(4u) + O(1 / u), below fp32's resolution
  if constexpr (OUT == kKnnPoincare)
    return u > 1.0995116e12f ? logf(u) + 1.3862944f : log1pf(2.f * u + 2.f * sqrtf(u * (u + 1.f)));
  return u;
}

// The thread's place in a distance tile: queries 4 tq .. +3; candidates 4 tj .. +3 and 64 + 4 tj .. +3
__device__ __forceinline__ int tile_tq() { return threadIdx.x >> 4; }
__device__ __forceinline__ int tile_tj() { return threadIdx.x & 15; }
__device__ __forceinline__ int tile_col(int tj, int c) { return (c < 4 ? 0 : kWave - 4) + 4 * tj + c; }

// Sweep the column tiles [tile_begin, tile_end) of the rows q0 .. q0 + 63 of xb [N, ld]:
// on_tile(tile, acc) runs once per tile, after a barrier behind the tile's last LDS read (it may
// overwrite `stage`, kKnnTQ * kKnnTJ floats), with acc[a][c] = d of query q0 + 4 tq + a and
// candidate tile * 128 + tile_col(tj, c); rows and columns past N read as zero rows.  The
// accumulators are cleared after it.  Called by all threads of the workgroup.
template <class OnTile>
__device__ __forceinline__ void dist_tile_sweep(const float* __restrict__ xb, int N, int C, int64_t ld, int q0,
                                                int tile_begin, int tile_end, float* stage, OnTile&& on_tile) {
  float* Qs = stage;                         // [kKnnCK][kKnnLDQ]
  float* Cs = stage + kKnnCK * kKnnLDQ;      // [kKnnCK][kKnnLDC]
  const int tid = threadIdx.x;
  const int tq = tile_tq(), tj = tile_tj();
  const int n_chunks = (C + kKnnCK - 1) / kKnnCK;
  if (tile_begin >= tile_end) return;

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

  load(tile_begin, 0);
  for (int tile = tile_begin; tile < tile_end; ++tile) {
    for (int ch = 0; ch < n_chunks; ++ch) {
      __syncthreads();  // the staging area's readers (the previous chunk, the previous tile's on_tile) are done
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
      if (ch + 1 < n_chunks) load(tile, ch + 1);
      else if (tile + 1 < tile_end) load(tile + 1, 0);
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
    __syncthreads();  // the last chunk's reads are done: on_tile may take the staging area
    on_tile(tile, acc);
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 8; ++c) acc[a][c] = 0.f;
  }
}

// acc[a][c] *= r_i r_j (pair_u) for the thread's queries and the tile's candidates; rows past N
// take r = 1 (their entries are never used).
__device__ __forceinline__ void tile_scale(float (&acc)[4][8], const float* __restrict__ rs, int N, int q0, int tile) {
  const int tq = tile_tq(), tj = tile_tj();
  float rq[4], rc[8];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int i = q0 + 4 * tq + a;
    rq[a] = i < N ? rs[i] : 1.f;
  }
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int j = tile * kKnnTJ + tile_col(tj, c);
    rc[c] = j < N ? rs[j] : 1.f;
  }
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[a][c] = pair_u(acc[a][c], rq[a], rc[c]);
}

// The thread's 4 x 8 values into the [64][128] tile over the staging area, then a barrier
__device__ __forceinline__ void tile_store(float* stage, const float (&acc)[4][8]) {
  const int tq = tile_tq(), tj = tile_tj();
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    float* dr = stage + (4 * tq + a) * kKnnTJ + 4 * tj;
    *reinterpret_cast<float4*>(dr) = make_float4(acc[a][0], acc[a][1], acc[a][2], acc[a][3]);
    *reinterpret_cast<float4*>(dr + kWave) = make_float4(acc[a][4], acc[a][5], acc[a][6], acc[a][7]);
  }
  __syncthreads();
}

__device__ __forceinline__ unsigned long long knn_key(float d, int j, bool ok) {
  return ok ? ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)j : kKnnNone;
}

__device__ __forceinline__ unsigned long long knn_readlane(unsigned long long v, int l) {
  const unsigned lo = __builtin_amdgcn_readlane((int)(unsigned)v, l);
  const unsigned hi = __builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
  return ((unsigned long long)hi << 32) | lo;
}

// Merge the keys of one half tile that pass the query's k-th key into its sorted list
// (lst[0..k), one entry per lane).  Keys are distinct (a candidate is scanned once), so
// the place of a key in the union is the number of keys below it.
__device__ __forceinline__ void knn_merge(unsigned long long* lst, unsigned long long key, int k, int lane) {
  const unsigned long long thr = lst[k - 1];
  const bool pass = key < thr;
  unsigned long long m = __ballot(pass);
  if (m == 0ull) return;
  const unsigned long long L = lane < k ? lst[lane] : kKnnNone;
  int below_L = 0, below_S = 0, list_below = 0;
  while (m) {
    const int s = __ffsll((long long)m) - 1;
    m &= m - 1;
    const unsigned long long sk = knn_readlane(key, s);
    below_L += sk < L ? 1 : 0;    // survivors below this lane's list entry
    below_S += sk < key ? 1 : 0;  // survivors below this lane's candidate
    const int nl = __popcll(__ballot(L < sk));
    if (lane == s) list_below = nl;
  }
  const int pl = lane + below_L;
  if (pl < k) lst[pl] = L;        // lane >= k: pl >= k
  if (pass) {
    const int ps = list_below + below_S;
    if (ps < k) lst[ps] = key;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
}

// One workgroup per tile of 64 queries of one graph; it scans all N candidates of that graph,
// so there is no merge across workgroups and the result does not depend on the launch
// geometry.  masked [B, N]: rows that are never a candidate and return themselves; rs [B, N]
// (OUT != kKnnRaw): the rows' r of pair_u.
template <int OUT>
__global__ __launch_bounds__(kBlock) void pos_knn_kernel(const float* __restrict__ x, int N, int C, int64_t ld, int k,
                                                     const uint8_t* __restrict__ masked,
                                                     const float* __restrict__ rs, int* __restrict__ idx_out,
                                                     float* __restrict__ dist_out) {
  __shared__ __align__(16) float stage[kKnnTQ * kKnnTJ];                      // chunks, then the distance tile
  __shared__ __align__(16) unsigned long long list[kKnnTQ * kKnnMaxK];        // [query][rank]
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int b = blockIdx.y;
  const int q0 = blockIdx.x * kKnnTQ;
  const float* xb = x + (int64_t)b * N * ld;
  const uint8_t* mb = masked + (int64_t)b * N;
  const float* rb = OUT != kKnnRaw ? rs + (int64_t)b * N : nullptr;
  const int n_tiles = (N + kKnnTJ - 1) / kKnnTJ;

  for (int i = tid; i < kKnnTQ * kKnnMaxK; i += kBlock) list[i] = kKnnNone;
  // the wave's queries that take part: in range and unmasked (bit i: query wave * 16 + i)
  unsigned q_live;
  {
    const int qr = q0 + wave * kKnnQPerWave + lane;
    const bool live = lane < kKnnQPerWave && qr < N && mb[qr] == 0;
    q_live = (unsigned)__ballot(live);
  }

  dist_tile_sweep(xb, N, C, ld, q0, 0, n_tiles, stage, [&](int tile, float (&acc)[4][8]) {
    if constexpr (OUT != kKnnRaw) tile_scale(acc, rb, N, q0, tile);
    tile_store(stage, acc);
    // lane = candidate of each half tile: in range and unmasked
    const int j0 = tile * kKnnTJ + lane;
    const bool cand_ok0 = j0 < N && mb[j0] == 0;
    const bool cand_ok1 = j0 + kWave < N && mb[j0 + kWave] == 0;
    // filter: bit 2 i + h set when a candidate of half h passes query i's k-th key
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
  });
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
      d = key == kKnnNone ? __uint_as_float(0x7f800000u) : pair_dist<OUT>(__uint_as_float((unsigned)(key >> 32)));
    }
    const int64_t o = ((int64_t)b * N + qr) * k + lane;
    idx_out[o] = j;
    if (dist_out) dist_out[o] = d;
  }
}

}  // namespace gnpde
