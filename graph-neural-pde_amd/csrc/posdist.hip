// posdist.hip — the positional-encoding distance rewiring (gnpde.graph_rewiring
// apply_pos_dist_rewire; src/graph_rewiring.py:318-375): for the rows of x [N, C] inside the
// Poincare ball, or in Euclidean space, either every row's k nearest rows (gnpde_pos_knn_f32)
// or every pair whose distance is at most a quantile of all N^2 distances
// (gnpde_pair_select_f32, gnpde_pair_threshold_count_f32 / _fill_f32).  The [N, N] matrix is
// never stored: every pass recomputes its tiles (knn_tile.hpp's dist_tile_sweep).
//
// Both distances are monotone in the rank value u_ij = d_ij r_i r_j (pair_u), d the squared
// difference-form distance, r = 1 / max(1 - |x|^2, 2^-52) (Poincare) or 1 (Euclid), so all
// ranking runs on the fp32 u, whose non-negative bit patterns order as unsigned integers.
// The pre-pass forms |x|^2, 1 - |x|^2 and r in fp64 (one wave per row, a fixed reduction) and
// rounds r to fp32 once: the cancellation of 1 - |x|^2 near the ball's rim stays at fp64's
// scale.  It also marks the rows that hold a non-finite value.
//
// Rank select (u of a 0-based rank among the N^2 entries, and the count of entries <= it):
// a most-significant-first radix select on the key of u, digits of 11, 11 and 10 bits: three
// histogram sweeps, each followed by a one-workgroup pick that finds the digit holding the
// residual rank on the device.  A sweep covers the tiles on and above the diagonal only and
// counts an entry above the diagonal twice (u_ij and u_ji are bit-equal).  A thread folds runs
// of equal digits among its 32 entries before it touches the workgroup's LDS histogram (pass 1:
// a few exponent bins take everything; later passes: most entries miss the prefix), and the
// workgroup flushes its 32-bit bins once, with 64-bit integer atomics: every count and rank is
// an integer held in 64 bits, so the result is the same on every call.
//
// Edge list: a workgroup owns 64 rows and sweeps all columns in ascending order; per row and
// half tile a ballot of u <= u_thr and a prefix popcount place each column, so the per-row
// count is the only intermediate (count pass, caller's exclusive scan, fill pass).
#include "knn_tile.hpp"

namespace gnpde {

constexpr int kSelPasses = 3;
constexpr int kSelBits[kSelPasses] = {11, 11, 10};
constexpr int kSelShift[kSelPasses] = {21, 10, 0};
constexpr int kSelBins = 1 << 11;
constexpr int64_t kPairMaxN = 1 << 24;   // a workgroup's 32-bit bins hold at most 2 * 64 * N counts
constexpr double kPoincareEps = 2.220446049250313e-16;  // 2^-52, float64 eps (the reference's clamp)

struct SelState {
  unsigned prefix;       // the digits found so far
  unsigned pad;
  long long rank;        // the residual rank inside the prefix
  long long below;       // entries whose key is below every key with the prefix
};

// The integer key of a rank value: the bits of u; a NaN (a pair with a non-finite row) ranks
// with +inf, behind every finite value.
__device__ __forceinline__ unsigned pair_key(float u) {
  const unsigned b = __float_as_uint(u);
  return b > 0x7f800000u ? 0x7f800000u : b;
}

// masked[b*N + r] = 1 when row r of graph b holds a non-finite value (NULL: not written);
// n_valid[b] (NULL: none; zeroed by the caller) += the other rows; rs[b*N + r] = r of pair_u.
// One wave per row, 8 rows a wave; the row's squares are summed in fp64 by a fixed butterfly.
template <bool POINCARE>
__global__ __launch_bounds__(kBlock) void pos_prep_kernel(const float* __restrict__ x, int N, int C, int64_t ld,
                                                          uint8_t* __restrict__ masked, int* n_valid,
                                                          float* __restrict__ rs) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int b = blockIdx.y;
  const int64_t r0 = ((int64_t)blockIdx.x * kWavesPerBlock + wave) * kKnnMaskRows;
  int cnt = 0;
  for (int t = 0; t < kKnnMaskRows; ++t) {
    const int64_t r = r0 + t;
    if (r >= N) break;
    const float* xr = x + ((int64_t)b * N + r) * ld;
    bool bad = false;
    double q = 0.0;
    for (int c = lane; c < C; c += kWave) {
      const float v = xr[c];
      bad |= (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u;
      q = fma((double)v, (double)v, q);
    }
    const bool m = __ballot(bad) != 0ull;
    float rv = 1.f;
    if constexpr (POINCARE) {
      q = wave_sum(q);
      rv = m ? 1.f : (float)(1.0 / fmax(1.0 - q, kPoincareEps));
    }
    if (lane == 0) {
      if (masked) masked[(int64_t)b * N + r] = m ? 1 : 0;
      rs[(int64_t)b * N + r] = rv;
    }
    cnt += m ? 0 : 1;
  }
  if (n_valid && lane == 0 && cnt) atomicAdd(n_valid + b, cnt);
}

__global__ void pair_init_kernel(SelState* st, long long rank, unsigned long long* ghist) {
  for (int i = threadIdx.x; i < kSelBins; i += blockDim.x) ghist[i] = 0ull;
  if (threadIdx.x == 0) {
    st->prefix = 0u;
    st->pad = 0u;
    st->rank = rank;
    st->below = 0;
  }
}

// One digit's histogram of the entries (i, j), j >= i, whose key matches the prefix above the
// digit; an entry with j > i counts twice.  Workgroup = 64 rows, column tiles from the one that
// holds the diagonal.
__global__ __launch_bounds__(kBlock, 2) void pair_hist_kernel(const float* __restrict__ x, int N, int C, int64_t ld,
                                                           const float* __restrict__ rs,
                                                           const SelState* __restrict__ st, int shift, int bits,
                                                           unsigned long long* __restrict__ ghist) {
  __shared__ __align__(16) float stage[kKnnTQ * kKnnTJ];
  __shared__ unsigned hist[kSelBins];
  const int tid = threadIdx.x;
  const int q0 = blockIdx.x * kKnnTQ;
  const int n_tiles = (N + kKnnTJ - 1) / kKnnTJ;
  const int nb = 1 << bits;
  const unsigned prefix = st->prefix;
  const unsigned himask = shift + bits >= 32 ? 0u : ~0u << (shift + bits);
  for (int i = tid; i < nb; i += kBlock) hist[i] = 0u;   // (the sweep's first barrier orders it)
  const int tq = tile_tq(), tj = tile_tj();
  dist_tile_sweep(x, N, C, ld, q0, q0 / kKnnTJ, n_tiles, stage, [&](int tile, float (&acc)[4][8]) {
    tile_scale(acc, rs, N, q0, tile);
    unsigned run_bin = 0u, run_cnt = 0u;   // a run of equal digits, folded before the LDS atomic
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int i = q0 + 4 * tq + a;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int j = tile * kKnnTJ + tile_col(tj, c);
        const unsigned key = pair_key(acc[a][c]);
        const unsigned w = (j < N && j >= i) ? (j > i ? 2u : 1u) : 0u;   // (j >= i and j < N give i < N)
        if (w != 0u && ((key ^ prefix) & himask) == 0u) {
          const unsigned bin = (key >> shift) & (unsigned)(nb - 1);
          if (bin != run_bin && run_cnt != 0u) {
            atomicAdd(&hist[run_bin], run_cnt);
            run_cnt = 0u;
          }
          run_bin = bin;
          run_cnt += w;
        }
      }
    }
    if (run_cnt != 0u) atomicAdd(&hist[run_bin], run_cnt);
  });
  __syncthreads();
  for (int i = tid; i < nb; i += kBlock) {
    const unsigned v = hist[i];
    if (v != 0u) atomicAdd(&ghist[i], (unsigned long long)v);
  }
}

// The digit that holds the residual rank: one workgroup.  Clears the histogram for the next
// sweep; after the last digit writes u and the count of entries <= u.
__global__ __launch_bounds__(kBlock) void pair_pick_kernel(SelState* st, unsigned long long* ghist, int shift,
                                                           int bits, int last, float* u_out, long long* count_le_out) {
  __shared__ unsigned long long h[kSelBins];
  const int nb = 1 << bits;
  for (int i = threadIdx.x; i < nb; i += kBlock) {
    h[i] = ghist[i];
    ghist[i] = 0ull;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const unsigned long long rank = (unsigned long long)st->rank;
  unsigned long long cum = 0ull;
  int bin = nb - 1;
  for (int i = 0; i < nb; ++i) {
    if (cum + h[i] > rank) {
      bin = i;
      break;
    }
    if (i + 1 < nb) cum += h[i];   // (a rank past the total, which the host rules out, stays in the last bin)
  }
  const unsigned prefix = st->prefix | ((unsigned)bin << shift);
  const long long below = st->below + (long long)cum;
  st->prefix = prefix;
  st->rank = (long long)(rank - cum);
  st->below = below;
  if (last) {
    *u_out = __uint_as_float(prefix);
    *count_le_out = below + (long long)h[bin];
  }
}

// Rows q0 .. q0 + 63 against all columns, ascending: per row the entries with u <= *u_thr.
// FILL = false: row_count[i] = their number.  FILL = true: entry number p of row i (columns
// ascending) goes to position row_ptr[i] + p of ei [2, E]: ei[0] = i, ei[1] = j.
// (Two waves per SIMD asked of the count pass and the histogram, which fit 256 registers without
// spilling; the fill pass does not, and runs at one.)
template <bool FILL>
__global__ __launch_bounds__(kBlock, FILL ? 1 : 2) void pair_emit_kernel(const float* __restrict__ x, int N, int C, int64_t ld,
                                                           const float* __restrict__ rs,
                                                           const float* __restrict__ u_thr,
                                                           long long* __restrict__ row_count,
                                                           const long long* __restrict__ row_ptr,
                                                           long long* __restrict__ ei, long long E) {
  __shared__ __align__(16) float stage[kKnnTQ * kKnnTJ];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int q0 = blockIdx.x * kKnnTQ;
  const int n_tiles = (N + kKnnTJ - 1) / kKnnTJ;
  const unsigned thr = pair_key(*u_thr);
  const unsigned long long lt = (1ull << lane) - 1ull;   // the lanes below this one
  // lane i < 16 holds row q0 + wave * 16 + i: its running count and, for the fill, its offset
  const int my_row = q0 + wave * kKnnQPerWave + lane;
  const bool own = lane < kKnnQPerWave && my_row < N;
  int run = 0;
  long long base = 0;
  if constexpr (FILL) base = own ? row_ptr[my_row] : 0;
  dist_tile_sweep(x, N, C, ld, q0, 0, n_tiles, stage, [&](int tile, float (&acc)[4][8]) {
    tile_scale(acc, rs, N, q0, tile);
    tile_store(stage, acc);
    const int j0 = tile * kKnnTJ + lane;
#pragma unroll
    for (int i = 0; i < kKnnQPerWave; ++i) {
      const int q = wave * kKnnQPerWave + i, row = q0 + q;
      if (row >= N) break;   // wave-uniform
      const bool ok0 = j0 < N && pair_key(stage[q * kKnnTJ + lane]) <= thr;
      const bool ok1 = j0 + kWave < N && pair_key(stage[q * kKnnTJ + kWave + lane]) <= thr;
      const unsigned long long b0 = __ballot(ok0), b1 = __ballot(ok1);
      const int n0 = __popcll(b0), n1 = __popcll(b1);
      if constexpr (FILL) {
        const long long p = __shfl(base, i) + __shfl(run, i);
        const long long p0 = p + __popcll(b0 & lt), p1 = p + n0 + __popcll(b1 & lt);
        if (ok0 && p0 >= 0 && p0 < E) {   // (in range whenever row_ptr is the scan of the count pass)
          ei[p0] = row;
          ei[E + p0] = j0;
        }
        if (ok1 && p1 >= 0 && p1 < E) {
          ei[p1] = row;
          ei[E + p1] = j0 + kWave;
        }
      }
      if (lane == i) run += n0 + n1;
    }
  });
  if constexpr (!FILL) {
    if (own) row_count[my_row] = run;
  }
}

inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

struct PairWs {
  float* rs;
  unsigned long long* ghist;
  SelState* st;
};

inline size_t pair_ws_bytes(int64_t N) {
  return align16(sizeof(float) * (size_t)(N > 0 ? N : 0)) + sizeof(unsigned long long) * kSelBins + 64;
}

inline PairWs pair_ws(void* workspace, int64_t N) {
  char* p = static_cast<char*>(workspace);
  PairWs w;
  w.rs = reinterpret_cast<float*>(p);
  p += align16(sizeof(float) * (size_t)N);
  w.ghist = reinterpret_cast<unsigned long long*>(p);
  p += sizeof(unsigned long long) * kSelBins;
  w.st = reinterpret_cast<SelState*>(p);
  return w;
}

// the arguments every pair entry point shares
static int pair_validate(const char* name, const float* x, int64_t N, int64_t C, int64_t ld, int metric,
                         const void* workspace, size_t ws_bytes) {
  GNPDE_REQUIRE(N >= 0, GNPDE_EINVAL, "%s: N=%lld must be >= 0", name, (long long)N);
  GNPDE_REQUIRE(C >= 1 && C <= ld && C < INT32_MAX - kKnnCK, GNPDE_EINVAL, "%s: C=%lld must be in [1, ld=%lld]", name,
                (long long)C, (long long)ld);
  GNPDE_REQUIRE(metric == GNPDE_METRIC_EUCLID || metric == GNPDE_METRIC_POINCARE, GNPDE_EINVAL,
                "%s: metric=%d (GNPDE_METRIC_EUCLID | GNPDE_METRIC_POINCARE)", name, metric);
  GNPDE_REQUIRE(N <= kPairMaxN, GNPDE_EUNSUPPORTED, "%s: N=%lld outside the kernel's range (N <= %lld)", name,
                (long long)N, (long long)kPairMaxN);
  GNPDE_REQUIRE(N == 0 || (x && workspace), GNPDE_EINVAL, "%s: NULL x / workspace", name);
  GNPDE_REQUIRE(N == 0 || aligned16(workspace), GNPDE_EINVAL, "%s: workspace must be 16-byte aligned", name);
  GNPDE_REQUIRE(N == 0 || ws_bytes >= pair_ws_bytes(N), GNPDE_EINVAL, "%s: workspace of %zu bytes, %zu needed", name,
                ws_bytes, pair_ws_bytes(N));
  return GNPDE_OK;
}

static int pair_prep(const float* x, int64_t N, int64_t C, int64_t ld, int metric, float* rs, hipStream_t st) {
  const dim3 grid((unsigned)ceil_div(N, kWavesPerBlock * kKnnMaskRows), 1u);
  if (metric == GNPDE_METRIC_POINCARE)
    pos_prep_kernel<true><<<grid, kBlock, 0, st>>>(x, (int)N, (int)C, ld, nullptr, nullptr, rs);
  else
    pos_prep_kernel<false><<<grid, kBlock, 0, st>>>(x, (int)N, (int)C, ld, nullptr, nullptr, rs);
  GNPDE_LAUNCH_CHECK();
  return GNPDE_OK;
}

}  // namespace gnpde

using namespace gnpde;

extern "C" {

size_t gnpde_pos_knn_workspace_bytes(int64_t B, int64_t N) {
  if (B <= 0 || N <= 0) return 16;
  return align16((size_t)B * (size_t)N) + align16(sizeof(float) * (size_t)B * (size_t)N);
}

int gnpde_pos_knn_f32(const float* x, int64_t B, int64_t N, int64_t C, int64_t ld, int64_t k, int metric,
                      int32_t* idx_out, float* dist_out, int32_t* n_valid, void* workspace, void* stream) {
  GNPDE_REQUIRE(B >= 0 && B <= 65535, GNPDE_EINVAL, "pos_knn: B=%lld must be in [0, 65535]", (long long)B);
  GNPDE_REQUIRE(N >= 0 && N < INT32_MAX - 2 * kKnnTJ, GNPDE_EINVAL, "pos_knn: N=%lld out of range", (long long)N);
  GNPDE_REQUIRE(C >= 1 && C <= ld && C < INT32_MAX - kKnnCK, GNPDE_EINVAL, "pos_knn: C=%lld must be in [1, ld=%lld]",
                (long long)C, (long long)ld);
  GNPDE_REQUIRE(k >= 1, GNPDE_EINVAL, "pos_knn: k=%lld must be >= 1", (long long)k);
  GNPDE_REQUIRE(metric == GNPDE_METRIC_EUCLID || metric == GNPDE_METRIC_POINCARE, GNPDE_EINVAL,
                "pos_knn: metric=%d (GNPDE_METRIC_EUCLID | GNPDE_METRIC_POINCARE)", metric);
  GNPDE_REQUIRE(B * N == 0 || (x && idx_out && n_valid && workspace), GNPDE_EINVAL,
                "pos_knn: NULL x / idx_out / n_valid / workspace");
  GNPDE_REQUIRE(B * N == 0 || aligned16(workspace), GNPDE_EINVAL, "pos_knn: workspace must be 16-byte aligned");
  GNPDE_REQUIRE(k <= kKnnMaxK, GNPDE_EUNSUPPORTED, "pos_knn: k=%lld outside the kernel's range (1 <= k <= %d)",
                (long long)k, kKnnMaxK);
  if (B * N == 0) return GNPDE_OK;
  hipStream_t st = as_stream(stream);
  uint8_t* masked = static_cast<uint8_t*>(workspace);
  float* rs = reinterpret_cast<float*>(static_cast<char*>(workspace) + align16((size_t)B * (size_t)N));
  GNPDE_HIP(hipMemsetAsync(n_valid, 0, sizeof(int32_t) * (size_t)B, st));
  const dim3 mgrid((unsigned)ceil_div(N, kWavesPerBlock * kKnnMaskRows), (unsigned)B);
  const dim3 grid((unsigned)ceil_div(N, kKnnTQ), (unsigned)B);
  if (metric == GNPDE_METRIC_POINCARE) {
    pos_prep_kernel<true><<<mgrid, kBlock, 0, st>>>(x, (int)N, (int)C, ld, masked, n_valid, rs);
    GNPDE_LAUNCH_CHECK();
    pos_knn_kernel<kKnnPoincare><<<grid, kBlock, 0, st>>>(x, (int)N, (int)C, ld, (int)k, masked, rs, idx_out, dist_out);
  } else {
    pos_prep_kernel<false><<<mgrid, kBlock, 0, st>>>(x, (int)N, (int)C, ld, masked, n_valid, rs);
    GNPDE_LAUNCH_CHECK();
    pos_knn_kernel<kKnnEuclid><<<grid, kBlock, 0, st>>>(x, (int)N, (int)C, ld, (int)k, masked, rs, idx_out, dist_out);
  }
  GNPDE_LAUNCH_CHECK();
  return GNPDE_OK;
}

size_t gnpde_pair_workspace_bytes(int64_t N) { return pair_ws_bytes(N); }

int gnpde_pair_select_f32(const float* x, int64_t N, int64_t C, int64_t ld, int metric, int64_t rank, float* u_out,
                          int64_t* count_le_out, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = pair_validate("pair_select", x, N, C, ld, metric, workspace, workspace_bytes)) return rc;
  GNPDE_REQUIRE(N >= 1, GNPDE_EINVAL, "pair_select: N=%lld must be >= 1", (long long)N);
  GNPDE_REQUIRE(rank >= 0 && rank < N * N, GNPDE_EINVAL, "pair_select: rank=%lld must be in [0, N^2=%lld)",
                (long long)rank, (long long)(N * N));
  GNPDE_REQUIRE(u_out && count_le_out && aligned8(count_le_out), GNPDE_EINVAL,
                "pair_select: NULL u_out / count_le_out, or count_le_out not 8-byte aligned");
  hipStream_t st = as_stream(stream);
  const PairWs w = pair_ws(workspace, N);
  if (int rc = pair_prep(x, N, C, ld, metric, w.rs, st)) return rc;
  pair_init_kernel<<<1, kBlock, 0, st>>>(w.st, (long long)rank, w.ghist);
  GNPDE_LAUNCH_CHECK();
  const unsigned grid = (unsigned)ceil_div(N, kKnnTQ);
  for (int p = 0; p < kSelPasses; ++p) {
    pair_hist_kernel<<<grid, kBlock, 0, st>>>(x, (int)N, (int)C, ld, w.rs, w.st, kSelShift[p], kSelBits[p], w.ghist);
    GNPDE_LAUNCH_CHECK();
    pair_pick_kernel<<<1, kBlock, 0, st>>>(w.st, w.ghist, kSelShift[p], kSelBits[p], p + 1 == kSelPasses ? 1 : 0,
                                           u_out, reinterpret_cast<long long*>(count_le_out));
    GNPDE_LAUNCH_CHECK();
  }
  return GNPDE_OK;
}

int gnpde_pair_threshold_count_f32(const float* x, int64_t N, int64_t C, int64_t ld, int metric, const float* u_thr,
                                   int64_t* row_count, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = pair_validate("pair_threshold_count", x, N, C, ld, metric, workspace, workspace_bytes)) return rc;
  GNPDE_REQUIRE(N == 0 || (u_thr && row_count && aligned8(row_count)), GNPDE_EINVAL,
                "pair_threshold_count: NULL u_thr / row_count, or row_count not 8-byte aligned");
  if (N == 0) return GNPDE_OK;
  hipStream_t st = as_stream(stream);
  const PairWs w = pair_ws(workspace, N);
  if (int rc = pair_prep(x, N, C, ld, metric, w.rs, st)) return rc;
  pair_emit_kernel<false><<<(unsigned)ceil_div(N, kKnnTQ), kBlock, 0, st>>>(
      x, (int)N, (int)C, ld, w.rs, u_thr, reinterpret_cast<long long*>(row_count), nullptr, nullptr, 0);
  GNPDE_LAUNCH_CHECK();
  return GNPDE_OK;
}

int gnpde_pair_threshold_fill_f32(const float* x, int64_t N, int64_t C, int64_t ld, int metric, const float* u_thr,
                                  const int64_t* row_ptr, int64_t E, int64_t* ei_out, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  if (int rc = pair_validate("pair_threshold_fill", x, N, C, ld, metric, workspace, workspace_bytes)) return rc;
  GNPDE_REQUIRE(E >= 0 && E <= N * N, GNPDE_EINVAL, "pair_threshold_fill: E=%lld must be in [0, N^2=%lld]",
                (long long)E, (long long)(N * N));
  GNPDE_REQUIRE(N == 0 || (u_thr && row_ptr && aligned8(row_ptr)), GNPDE_EINVAL,
                "pair_threshold_fill: NULL u_thr / row_ptr, or row_ptr not 8-byte aligned");
  GNPDE_REQUIRE(E == 0 || (ei_out && aligned8(ei_out)), GNPDE_EINVAL,
                "pair_threshold_fill: NULL ei_out, or ei_out not 8-byte aligned");
  if (N == 0 || E == 0) return GNPDE_OK;
  hipStream_t st = as_stream(stream);
  const PairWs w = pair_ws(workspace, N);
  if (int rc = pair_prep(x, N, C, ld, metric, w.rs, st)) return rc;
  pair_emit_kernel<true><<<(unsigned)ceil_div(N, kKnnTQ), kBlock, 0, st>>>(
      x, (int)N, (int)C, ld, w.rs, u_thr, nullptr, reinterpret_cast<const long long*>(row_ptr),
      reinterpret_cast<long long*>(ei_out), (long long)E);
  GNPDE_LAUNCH_CHECK();
  return GNPDE_OK;
}

}  // extern "C"
