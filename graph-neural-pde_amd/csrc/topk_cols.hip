// topk_cols.hip — the k largest entries of every COLUMN of a row-major block y [N, ld]
// (gnpde_topk_cols_f32): the sparsification of a GDC diffusion block S[:, J] whose columns
// are the seeds (gnpde.ops.gdc; PyG's GDC `topk` with dim = 0, src/graph_rewiring.py:50-51).
//
// Order.  One integer key per entry, (e(v) << 32) | row, with e the order-preserving map of
// the fp32 bits inverted so that a larger value has a smaller e (-0 counts as +0).  The k
// smallest keys of a column in unsigned order are its k largest values, the lower row first
// on equal values: a total order over distinct keys, so the selected set and its ranks do
// not depend on how the rows are split over workgroups.  Inputs are finite.
//
// Two passes.  The select pass gives a workgroup 32 consecutive columns (one 128-byte line
// of every row) and a run of rows.  Tiles of 64 rows are read coalesced, one row segment
// per half wave, and staged transposed in LDS ([column][row], stride 65 words: the per-lane
// row reads of a column are conflict free, the stores of a half wave's two rows at most
// 2-way).  A wave owns 8 columns, lane = row of the tile: one compare against the column's
// k-th key and a ballot per (column, tile); only tiles with a survivor take the rank merge
// of knn.hip (every survivor and every list entry computes its place in the union from
// ballots), with two list entries per lane for k > 64.  The sorted lists, 32 columns x 128
// keys x 8 B = 32 KB, and the 8 KB tile leave room for three workgroups per CU; the
// alternative, all 128 columns of a block in one workgroup, is 128 KB of lists: one
// resident workgroup whose 4 waves cannot hide the tile loads.  The next tile's global
// loads are issued before the current tile's selection.
// With one run of rows the select pass writes the outputs itself.  Otherwise it stores its
// sorted partial lists (keys) to the workspace and the merge pass, one wave per column,
// merges the runs' lists in the same key order and writes the outputs.
//
// Outputs per column c, rank m < k: idx_out[c, m] the row, val_out[c, m] its value,
// wnorm_out[c, m] = val / (val_0 + val_1 + ... + val_{k-1}), the sum taken sequentially in
// rank order in fp32 (every lane repeats it: no reduction tree, no atomics), 0 when the
// sum is 0.  The same bits on every call and for every split of the rows.
#include <algorithm>

#include "common.hpp"

namespace gnpde {

constexpr int kTkCols = 32;                       // columns of a workgroup
constexpr int kTkRows = 64;                       // rows of a tile (lane = row)
constexpr int kTkLd = kTkRows + 1;                // LDS stride of a staged column (words)
constexpr int kTkMaxK = 128;                      // two list entries per lane
constexpr int kTkColsPerWave = kTkCols / kWavesPerBlock;       // 8
constexpr int kTkLoads = kTkCols * kTkRows / kBlock;           // 8 staged words per thread
constexpr int kTkRowsPerPass = kBlock / kTkCols;               // 8 rows of a tile per load pass
constexpr unsigned long long kTkNone = ~0ull;

// order-preserving map of the fp32 bits, inverted: a larger value gives a smaller code
__device__ __forceinline__ unsigned tk_encode(float v) {
  unsigned u = __float_as_uint(v);
  if ((u << 1) == 0u) u = 0u;  // -0 sorts as +0
  const unsigned m = (u & 0x80000000u) ? ~u : (u ^ 0x80000000u);
  return ~m;
}

__device__ __forceinline__ float tk_decode(unsigned e) {
  const unsigned m = ~e;
  return __uint_as_float((m & 0x80000000u) ? (m ^ 0x80000000u) : ~m);
}

__device__ __forceinline__ unsigned long long tk_readlane(unsigned long long v, int l) {
  const unsigned lo = __builtin_amdgcn_readlane((int)(unsigned)v, l);
  const unsigned hi = __builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
  return ((unsigned long long)hi << 32) | lo;
}

// Merge the lanes' keys that pass the column's k-th key into its sorted list lst[0..k)
// (entry lane, and entry 64 + lane when TWO).  Keys are distinct (a row is scanned once),
// so the place of a key in the union is the number of keys below it.  kTkNone = no key.
template <bool TWO>
__device__ __forceinline__ void tk_merge(unsigned long long* lst, unsigned long long key, int k, int lane) {
  const unsigned long long thr = lst[k - 1];
  const bool pass = key < thr;
  unsigned long long m = __ballot(pass);
  if (m == 0ull) return;
  const unsigned long long L0 = lane < k ? lst[lane] : kTkNone;
  unsigned long long L1 = kTkNone;
  if constexpr (TWO) L1 = kWave + lane < k ? lst[kWave + lane] : kTkNone;
  int below_L0 = 0, below_L1 = 0, below_S = 0, list_below = 0;
  while (m) {
    const int s = __ffsll((long long)m) - 1;
    m &= m - 1;
    const unsigned long long sk = tk_readlane(key, s);
    below_L0 += sk < L0 ? 1 : 0;   // survivors below this lane's list entries
    below_S += sk < key ? 1 : 0;   // survivors below this lane's candidate
    int nl = __popcll(__ballot(L0 < sk));
    if constexpr (TWO) {
      below_L1 += sk < L1 ? 1 : 0;
      nl += __popcll(__ballot(L1 < sk));
    }
    if (lane == s) list_below = nl;
  }
  const int p0 = lane + below_L0;
  if (p0 < k) lst[p0] = L0;        // lane >= k: p0 >= k
  if constexpr (TWO) {
    const int p1 = kWave + lane + below_L1;
    if (p1 < k) lst[p1] = L1;
  }
  if (pass) {
    const int ps = list_below + below_S;
    if (ps < k) lst[ps] = key;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
}

// The outputs of one column from its finished list (k <= N: every entry is a key).
__device__ __forceinline__ void tk_emit(const unsigned long long* lst, int k, int lane, int64_t o,
                                        int32_t* __restrict__ idx_out, float* __restrict__ val_out,
                                        float* __restrict__ wnorm_out) {
  float sum = 0.f;
  if (wnorm_out)
    for (int i = 0; i < k; ++i) sum = __fadd_rn(sum, tk_decode((unsigned)(lst[i] >> 32)));  // rank order
  for (int i = lane; i < k; i += kWave) {
    const unsigned long long key = lst[i];
    const float v = tk_decode((unsigned)(key >> 32));
    idx_out[o + i] = (int32_t)(unsigned)key;
    val_out[o + i] = v;
    if (wnorm_out) wnorm_out[o + i] = sum == 0.f ? 0.f : __fdiv_rn(v, sum);
  }
}

// Select pass: workgroup (x, y) = columns [32 x, 32 x + 32), rows [y rows_per, (y + 1) rows_per).
template <bool TWO>
__global__ __launch_bounds__(kBlock) void topk_cols_select_kernel(const float* __restrict__ y, int N, int ncols,
                                                                  int64_t ld, int k, int rows_per,
                                                                  unsigned long long* __restrict__ part,
                                                                  int32_t* __restrict__ idx_out,
                                                                  float* __restrict__ val_out,
                                                                  float* __restrict__ wnorm_out) {
  __shared__ __align__(16) unsigned long long list[kTkCols * kTkMaxK];   // [column][rank]
  __shared__ float tile[kTkCols * kTkLd];                                // [column][row of the tile]
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int c0 = blockIdx.x * kTkCols;
  // r0 < N (the grid has ceil(N / rows_per) runs); r0 + rows_per may pass 2^31 for a caller's rows_per
  const int r0 = (int)((int64_t)blockIdx.y * rows_per);
  const int r1 = (int)std::min<int64_t>(N, (int64_t)r0 + rows_per);
  const int lc = tid & (kTkCols - 1), lr = tid / kTkCols;   // the thread's column and first row of a tile
  const bool col_ok = c0 + lc < ncols;

  for (int i = tid; i < kTkCols * kTkMaxK; i += kBlock) list[i] = kTkNone;
  __syncthreads();

  float pv[kTkLoads];
  auto load = [&](int rt) {
#pragma unroll
    for (int i = 0; i < kTkLoads; ++i) {
      const int r = rt + lr + kTkRowsPerPass * i;
      pv[i] = (col_ok && r < r1) ? y[(int64_t)r * ld + c0 + lc] : 0.f;
    }
  };

  load(r0);
  for (int rt = r0; rt < r1; rt += kTkRows) {
    __syncthreads();  // the previous tile's readers are done (and the lists are initialised)
#pragma unroll
    for (int i = 0; i < kTkLoads; ++i) tile[lc * kTkLd + lr + kTkRowsPerPass * i] = pv[i];
    __syncthreads();
    if (rt + kTkRows < r1) load(rt + kTkRows);
    const int row = rt + lane;
#pragma unroll 1
    for (int j = 0; j < kTkColsPerWave; ++j) {
      const int c = wave * kTkColsPerWave + j;
      if (c0 + c >= ncols) break;  // wave-uniform
      const float v = tile[c * kTkLd + lane];
      const unsigned long long key =
          row < r1 ? ((unsigned long long)tk_encode(v) << 32) | (unsigned)row : kTkNone;
      tk_merge<TWO>(list + c * kTkMaxK, key, k, lane);
    }
  }
  // (a wave reads only the lists it wrote)
  for (int j = 0; j < kTkColsPerWave; ++j) {
    const int c = wave * kTkColsPerWave + j;
    if (c0 + c >= ncols) break;
    const unsigned long long* lst = list + c * kTkMaxK;
    if (part) {
      unsigned long long* dst = part + ((int64_t)blockIdx.y * ncols + c0 + c) * k;
      for (int i = lane; i < k; i += kWave) dst[i] = lst[i];
    } else {
      tk_emit(lst, k, lane, (int64_t)(c0 + c) * k, idx_out, val_out, wnorm_out);
    }
  }
}

// Merge pass: one wave per column merges the n_parts sorted partial lists.
template <bool TWO>
__global__ __launch_bounds__(kBlock) void topk_cols_merge_kernel(const unsigned long long* __restrict__ part,
                                                                 int ncols, int k, int n_parts,
                                                                 int32_t* __restrict__ idx_out,
                                                                 float* __restrict__ val_out,
                                                                 float* __restrict__ wnorm_out) {
  __shared__ __align__(16) unsigned long long list[kWavesPerBlock * kTkMaxK];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int c = blockIdx.x * kWavesPerBlock + wave;
  if (c >= ncols) return;  // wave-uniform; no workgroup barrier below
  unsigned long long* lst = list + wave * kTkMaxK;
  for (int i = lane; i < kTkMaxK; i += kWave) lst[i] = kTkNone;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  for (int p = 0; p < n_parts; ++p) {
    const unsigned long long* src = part + ((int64_t)p * ncols + c) * k;
    for (int h = 0; h < k; h += kWave) {
      const unsigned long long key = h + lane < k ? src[h + lane] : kTkNone;
      tk_merge<TWO>(lst, key, k, lane);
    }
  }
  tk_emit(lst, k, lane, (int64_t)c * k, idx_out, val_out, wnorm_out);
}

// rows of a workgroup's run: a multiple of the tile; 0 = chosen here (about two workgroups per CU)
static int64_t tk_rows_per(int64_t N, int64_t ncols, int64_t rows_per_wg) {
  int64_t rp = rows_per_wg;
  if (rp <= 0) {
    const int64_t groups = ceil_div(ncols, kTkCols);
    const int64_t parts = std::max<int64_t>(1, 512 / groups);
    rp = std::max<int64_t>(512, ceil_div(N, parts));
  }
  rp = std::min<int64_t>(rp, std::max<int64_t>(N, 1));  // one run at most covers every row (and fits an int)
  rp = ceil_div(rp, kTkRows) * kTkRows;
  // at most 65535 runs (gridDim.y)
  const int64_t least = ceil_div(ceil_div(N, 65535), kTkRows) * kTkRows;
  return std::max(rp, std::max<int64_t>(least, kTkRows));
}

}  // namespace gnpde

using namespace gnpde;

extern "C" {

size_t gnpde_topk_cols_workspace_bytes(int64_t N, int64_t ncols, int64_t k, int64_t rows_per_wg) {
  if (N <= 0 || ncols <= 0 || k <= 0) return 16;
  const int64_t parts = ceil_div(N, tk_rows_per(N, ncols, rows_per_wg));
  if (parts <= 1) return 16;
  return (size_t)parts * (size_t)ncols * (size_t)k * sizeof(unsigned long long);
}

int gnpde_topk_cols_f32(const float* y, int64_t N, int64_t ncols, int64_t ld, int64_t k, int32_t* idx_out,
                        float* val_out, float* wnorm_out, int64_t rows_per_wg, void* workspace,
                        size_t workspace_bytes, void* stream) {
  GNPDE_REQUIRE(N >= 0 && N < INT32_MAX - 2 * kTkRows, GNPDE_EINVAL, "topk_cols: N=%lld out of range", (long long)N);
  GNPDE_REQUIRE(ncols >= 0 && ncols <= ld && ncols <= (int64_t)65535 * kTkCols, GNPDE_EINVAL,
                "topk_cols: ncols=%lld must be in [0, ld=%lld]", (long long)ncols, (long long)ld);
  GNPDE_REQUIRE(k >= 1, GNPDE_EINVAL, "topk_cols: k=%lld must be >= 1", (long long)k);
  GNPDE_REQUIRE(rows_per_wg >= 0, GNPDE_EINVAL, "topk_cols: rows_per_wg=%lld must be >= 0", (long long)rows_per_wg);
  GNPDE_REQUIRE(k <= kTkMaxK, GNPDE_EUNSUPPORTED, "topk_cols: k=%lld outside the kernel's range (1 <= k <= %d)",
                (long long)k, kTkMaxK);
  GNPDE_REQUIRE(k <= N || ncols == 0, GNPDE_EINVAL, "topk_cols: k=%lld exceeds the %lld rows of the block",
                (long long)k, (long long)N);
  if (ncols == 0) return GNPDE_OK;
  GNPDE_REQUIRE(y && idx_out && val_out, GNPDE_EINVAL, "topk_cols: NULL y / idx_out / val_out");
  const int64_t rows_per = tk_rows_per(N, ncols, rows_per_wg);
  const int64_t parts = ceil_div(N, rows_per);
  const size_t need = gnpde_topk_cols_workspace_bytes(N, ncols, k, rows_per_wg);
  GNPDE_REQUIRE(parts <= 1 || (workspace && workspace_bytes >= need && aligned8(workspace)), GNPDE_EINVAL,
                "topk_cols: workspace of %zu bytes (8-byte aligned) needed, got %zu", need, workspace_bytes);
  hipStream_t st = as_stream(stream);
  unsigned long long* part = parts > 1 ? static_cast<unsigned long long*>(workspace) : nullptr;
  const dim3 grid((unsigned)ceil_div(ncols, kTkCols), (unsigned)parts);
  const bool two = k > kWave;
  if (two)
    topk_cols_select_kernel<true><<<grid, kBlock, 0, st>>>(y, (int)N, (int)ncols, ld, (int)k, (int)rows_per, part,
                                                           idx_out, val_out, wnorm_out);
  else
    topk_cols_select_kernel<false><<<grid, kBlock, 0, st>>>(y, (int)N, (int)ncols, ld, (int)k, (int)rows_per, part,
                                                            idx_out, val_out, wnorm_out);
  GNPDE_LAUNCH_CHECK();
  if (parts > 1) {
    const unsigned mgrid = (unsigned)ceil_div(ncols, kWavesPerBlock);
    if (two)
      topk_cols_merge_kernel<true><<<mgrid, kBlock, 0, st>>>(part, (int)ncols, (int)k, (int)parts, idx_out, val_out,
                                                             wnorm_out);
    else
      topk_cols_merge_kernel<false><<<mgrid, kBlock, 0, st>>>(part, (int)ncols, (int)k, (int)parts, idx_out,
                                                              val_out, wnorm_out);
    GNPDE_LAUNCH_CHECK();
  }
  return GNPDE_OK;
}

}  // extern "C"
