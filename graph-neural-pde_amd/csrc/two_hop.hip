// two_hop.hip — the two-hop product of the rewire_attention block (gnpde.block_transformer_rewiring;
// src/block_transformer_rewiring.py:65-93): for a coalesced CSR W (columns ascending inside a row,
// no duplicates, fp32 values) the structural positions of W·W as a CSR with ascending columns and
//   S[i, j] = 0.5 * ((sum_m W[i, m] W[m, j]) + W[i, j]),   S[i, i] = 0
// on them, plus the COO edge list in the same order.  The reference densifies to [N, N] and calls
// matmul; this is Gustavson's row-by-row form.
//
// One WAVEFRONT owns output row i in every pass.  It walks the stored m of row i in CSR order, one
// after another; its lanes spread over the stored j of row m.  W is coalesced, so the j of one step
// are distinct: every step is a conflict-free read-modify-write of the row's accumulator, and the
// steps of a wavefront follow each other in program order.  The value of a position is therefore
// the fma chain acc = fma(W[i, m], W[m, j], acc) over the m of row i IN CSR ORDER (the first product
// stored as it is), then acc + W[i, j] where W stores (i, j), then the exact halving — a fixed order,
// no floating-point atomic, the same bits on every call and for every launch geometry.
//
// Passes: gnpde_two_hop_bound_i32 (ub[i] = sum over the m of row i of len(row m), the cheap upper
// bound of the row's width), gnpde_two_hop_count_i32 (symbolic: distinct columns per row),
// the caller's exclusive scan, gnpde_two_hop_fill_f32 (numeric).  The symbolic and the numeric pass
// run the same two regimes, chosen per row from ub[i]:
//   ub == 0            nothing to do (an empty row, or only empty neighbour rows);
//   ub <= lds_max      a hash table of the wavefront in LDS (open addressing, linear probing, at
//                      most half full: 2 * ub rounded up to a power of two, <= kThTable slots).  A
//                      lane that claims a slot appends its column to the row's list; the list is
//                      rank-sorted (its length is the row's count) and written in ascending order;
//   ub >  lds_max      a dense accumulator of N floats and a bitmap of N bits in global scratch per
//                      resident wavefront.  The bitmap's atomic OR tells the first touch of a
//                      column, which stores instead of adding, so the accumulator is never cleared;
//                      the extraction sweeps the bitmap's N / 32 words in order (ascending columns
//                      for free) and zeroes the words it found set.
// LDS: 4 wavefronts x (kThTable keys + kThTable values + kThList columns) = 40 KB per workgroup,
// four workgroups per CU of 160 KB.  Hashed slots fall on random banks: conflicts are data
// dependent; the rank sort's reads are broadcasts (one address per instruction).
//
// gnpde_coalesce_sum_f32 is the prep pass: the duplicates of a (row, column)-sorted edge list summed
// one after another in sorted (= COO) order by the thread of the run's first entry.
#include "common.hpp"

namespace gnpde {

constexpr int kThTable = 1024;            // hash slots of a wavefront
constexpr int kThList = kThTable / 2;     // columns a row of the LDS regime can hold (= the largest lds_max)
constexpr int kThEmpty = -1;

__global__ __launch_bounds__(kBlock) void coalesce_sum_kernel(const float* __restrict__ w, const uint8_t* __restrict__ first,
                                                              const int64_t* __restrict__ uid, int64_t E,
                                                              float* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= E || !first[p]) return;
  float s = w[p];
  for (int64_t q = p + 1; q < E && !first[q]; ++q) s += w[q];
  out[uid[p]] = s;
}

// ub[i] = sum_{m in row i} len(row m): one wavefront per row
__global__ __launch_bounds__(kBlock) void two_hop_bound_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                               int N, int* __restrict__ ub) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t i = (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
  if (i >= N) return;
  const int b = rowptr[i], e = rowptr[i + 1];
  int s = 0;
  for (int p = b + lane; p < e; p += kWave) {
    const int m = col[p];
    s += rowptr[m + 1] - rowptr[m];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (lane == 0) ub[i] = s;
}

__device__ __forceinline__ void wave_fence() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); }

__device__ __forceinline__ int lanes_below(unsigned long long mask, int lane) {
  return __popcll(mask & ((1ull << lane) - 1ull));
}

// The slot of column j in the wavefront's table (claiming an empty one); fresh: this lane claimed it.
__device__ __forceinline__ int th_slot(int* keys, int j, int shift, int mask, bool& fresh) {
  int s = (int)(((unsigned)j * 2654435761u) >> shift) & mask;
  fresh = false;
  for (;;) {
    const int k = keys[s];
    if (k == j) return s;
    if (k == kThEmpty) {
      const int old = atomicCAS(&keys[s], kThEmpty, j);
      if (old == kThEmpty) {
        fresh = true;
        return s;
      }
      if (old == j) return s;
    }
    s = (s + 1) & mask;
  }
}

// The slot of column j, or -1 (lookup only)
__device__ __forceinline__ int th_find(const int* keys, int j, int shift, int mask) {
  int s = (int)(((unsigned)j * 2654435761u) >> shift) & mask;
  for (;;) {
    const int k = keys[s];
    if (k == j) return s;
    if (k == kThEmpty) return -1;
    s = (s + 1) & mask;
  }
}

// The LDS regime: rows with 0 < ub <= lds_max, one wavefront per row (grid-stride over all rows).
// NUMERIC false: count[i] = distinct columns.  true: columns, values and COO positions at out_ptr[i].
template <bool NUMERIC>
__global__ __launch_bounds__(kBlock) void two_hop_lds_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                             const float* __restrict__ val, int N,
                                                             const int* __restrict__ ub, int lds_max,
                                                             int* __restrict__ count, const int* __restrict__ out_ptr,
                                                             int* __restrict__ out_col, float* __restrict__ out_val,
                                                             int64_t* __restrict__ out_ei, int64_t nnz_out) {
  __shared__ int keys_s[kWavesPerBlock][kThTable];
  __shared__ float vals_s[NUMERIC ? kWavesPerBlock : 1][NUMERIC ? kThTable : 1];
  __shared__ int list_s[NUMERIC ? kWavesPerBlock : 1][NUMERIC ? kThList : 1];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  int* keys = keys_s[wave];
  float* vals = vals_s[NUMERIC ? wave : 0];
  int* list = list_s[NUMERIC ? wave : 0];
  const int64_t stride = (int64_t)gridDim.x * kWavesPerBlock;
  for (int64_t i64 = (int64_t)blockIdx.x * kWavesPerBlock + wave; i64 < N; i64 += stride) {
    const int i = (int)i64;
    const int u = ub[i];
    if (u <= 0 || u > lds_max) continue;   // wave-uniform
    // at most half full: the smallest power of two >= 2 u, at least one slot per lane
    int lg = 6;
    while ((1 << lg) < 2 * u) ++lg;
    const int slots = 1 << lg, mask = slots - 1, shift = 32 - lg;
    for (int t = lane; t < slots; t += kWave) keys[t] = kThEmpty;
    wave_fence();
    int cnt = 0;
    const int b = rowptr[i], e = rowptr[i + 1];
    for (int p = b; p < e; ++p) {
      const int m = col[p];
      const float a = NUMERIC ? val[p] : 0.f;
      const int mb = rowptr[m], me = rowptr[m + 1];
      for (int q0 = mb; q0 < me; q0 += kWave) {
        const int q = q0 + lane;
        const bool on = q < me;
        bool fresh = false;
        int j = 0;
        if (on) {
          j = col[q];
          const int s = th_slot(keys, j, shift, mask, fresh);
          if constexpr (NUMERIC) {
            const float w = val[q];
            vals[s] = fresh ? a * w : fmaf(a, w, vals[s]);
          }
        }
        const unsigned long long fm = __ballot(fresh);
        if constexpr (NUMERIC) {
          if (fresh) list[cnt + lanes_below(fm, lane)] = j;
        }
        cnt += __popcll(fm);
        wave_fence();
      }
    }
    if constexpr (!NUMERIC) {
      if (lane == 0) count[i] = cnt;
    } else {
      // + W[i, j] on the positions W stores, after every product
      for (int p = b + lane; p < e; p += kWave) {
        const int s = th_find(keys, col[p], shift, mask);
        if (s >= 0) vals[s] += val[p];
      }
      wave_fence();
      const int64_t base = out_ptr[i];
      for (int t = lane; t < cnt; t += kWave) {
        const int j = list[t];
        int rank = 0;
        for (int f = 0; f < cnt; ++f) rank += list[f] < j ? 1 : 0;
        const int s = th_find(keys, j, shift, mask);
        const int64_t o = base + rank;
        if (o < nnz_out) {   // (always, for the out_ptr of the symbolic pass)
          out_col[o] = j;
          out_val[o] = j == i ? 0.f : 0.5f * vals[s];
          out_ei[o] = i;
          out_ei[nnz_out + o] = j;
        }
      }
      wave_fence();
    }
  }
}

// The bitmap is set by atomics, which execute in the L2: it is read and cleared at agent scope too, so
// that no read is served by a line the CU's vector cache kept from before the atomics.
__device__ __forceinline__ unsigned bits_load(const unsigned* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The global regime: rows with ub > lds_max, one wavefront per row, wavefront w of n_waves walks the
// rows w, w + n_waves, ... and owns acc[w * N ..) and bits[w * words ..) (bits zero on entry and on exit).
template <bool NUMERIC>
__global__ __launch_bounds__(kBlock) void two_hop_dense_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                               const float* __restrict__ val, int N,
                                                               const int* __restrict__ ub, int lds_max, int n_waves,
                                                               float* acc_all, unsigned* bits_all,
                                                               int* __restrict__ count, const int* __restrict__ out_ptr,
                                                               int* __restrict__ out_col, float* __restrict__ out_val,
                                                               int64_t* __restrict__ out_ei, int64_t nnz_out) {
  const int lane = threadIdx.x & (kWave - 1);
  const int gw = blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
  if (gw >= n_waves) return;
  const int words = (N + 31) >> 5;
  float* acc = acc_all + (int64_t)gw * N;
  unsigned* bits = bits_all + (int64_t)gw * words;
  for (int64_t i64 = gw; i64 < N; i64 += n_waves) {
    const int i = (int)i64;
    if (ub[i] <= lds_max || ub[i] <= 0) continue;   // wave-uniform
    const int b = rowptr[i], e = rowptr[i + 1];
    for (int p = b; p < e; ++p) {
      const int m = col[p];
      const float a = NUMERIC ? val[p] : 0.f;
      const int mb = rowptr[m], me = rowptr[m + 1];
      for (int q = mb + lane; q < me; q += kWave) {
        const int j = col[q];
        const unsigned bit = 1u << (j & 31);
        const unsigned old = atomicOr(bits + (j >> 5), bit);
        if constexpr (NUMERIC) {
          const float w = val[q];
          acc[j] = (old & bit) ? fmaf(a, w, acc[j]) : a * w;
        }
      }
      wave_fence();
    }
    if constexpr (NUMERIC) {
      for (int p = b + lane; p < e; p += kWave) {
        const int j = col[p];
        if (bits_load(bits + (j >> 5)) & (1u << (j & 31))) acc[j] += val[p];
      }
      wave_fence();
    }
    // sweep the bitmap in word order: the count, or the positions in ascending columns
    int64_t run = NUMERIC ? (int64_t)out_ptr[i] : 0;
    int cnt = 0;
    for (int w0 = 0; w0 < words; w0 += kWave) {
      const int w = w0 + lane;
      unsigned v = w < words ? bits_load(bits + w) : 0u;
      if (v) __hip_atomic_store(bits + w, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int pc = __popc(v);
      if constexpr (!NUMERIC) {
        cnt += pc;
      } else {
        int incl = pc;   // inclusive prefix over the lanes
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
          const int t = __shfl_up(incl, o);
          if (lane >= o) incl += t;
        }
        int64_t o = run + incl - pc;
        while (v) {
          const int bpos = __ffs((int)v) - 1;
          v &= v - 1;
          const int j = (w << 5) + bpos;
          if (o < nnz_out) {   // (always, for the out_ptr of the symbolic pass)
            out_col[o] = j;
            out_val[o] = j == i ? 0.f : 0.5f * acc[j];
            out_ei[o] = i;
            out_ei[nnz_out + o] = j;
          }
          ++o;
        }
        run += __shfl(incl, kWave - 1);
      }
    }
    if constexpr (!NUMERIC) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
      if (lane == 0) count[i] = cnt;
    }
    wave_fence();
  }
}

static int two_hop_grid_lds(int64_t N) {
  const int64_t g = ceil_div(N, kWavesPerBlock);
  return (int)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

}  // namespace gnpde

using namespace gnpde;

extern "C" {

int gnpde_two_hop_lds_max(void) { return kThList; }

int gnpde_coalesce_sum_f32(const float* w_sorted, const uint8_t* first, const int64_t* uid, int64_t E, float* out,
                           void* stream) {
  GNPDE_REQUIRE(E >= 0, GNPDE_EINVAL, "coalesce_sum: E=%lld", (long long)E);
  if (E == 0) return GNPDE_OK;
  GNPDE_REQUIRE(w_sorted && first && uid && out, GNPDE_EINVAL, "coalesce_sum: NULL argument");
  GNPDE_REQUIRE(ceil_div(E, kBlock) <= INT32_MAX, GNPDE_EINVAL, "coalesce_sum: E=%lld out of range", (long long)E);
  coalesce_sum_kernel<<<(unsigned)ceil_div(E, kBlock), kBlock, 0, as_stream(stream)>>>(w_sorted, first, uid, E, out);
  GNPDE_LAUNCH_CHECK();
  return GNPDE_OK;
}

int gnpde_two_hop_bound_i32(const int32_t* rowptr, const int32_t* col, int64_t N, int32_t* ub, void* stream) {
  GNPDE_REQUIRE(N >= 0 && N < INT32_MAX - kBlock, GNPDE_EINVAL, "two_hop_bound: N=%lld out of range", (long long)N);
  if (N == 0) return GNPDE_OK;
  GNPDE_REQUIRE(rowptr && col && ub, GNPDE_EINVAL, "two_hop_bound: NULL argument");
  two_hop_bound_kernel<<<(unsigned)ceil_div(N, kWavesPerBlock), kBlock, 0, as_stream(stream)>>>(rowptr, col, (int)N, ub);
  GNPDE_LAUNCH_CHECK();
  return GNPDE_OK;
}

static int two_hop_args(const char* who, const void* rowptr, const void* col, int64_t N, const void* ub,
                        int64_t lds_max, int64_t n_waves, const void* acc, const void* bits) {
  GNPDE_REQUIRE(N >= 0 && N < INT32_MAX - kBlock, GNPDE_EINVAL, "%s: N=%lld out of range", who, (long long)N);
  GNPDE_REQUIRE(lds_max >= 0 && lds_max <= kThList, GNPDE_EINVAL, "%s: lds_max=%lld must be in [0, %d]", who,
                (long long)lds_max, kThList);
  GNPDE_REQUIRE(n_waves >= 1 && n_waves <= 65536, GNPDE_EINVAL, "%s: n_waves=%lld must be in [1, 65536]", who,
                (long long)n_waves);
  GNPDE_REQUIRE(N == 0 || (rowptr && col && ub && acc && bits), GNPDE_EINVAL, "%s: NULL argument", who);
  return GNPDE_OK;
}

int gnpde_two_hop_count_i32(const int32_t* rowptr, const int32_t* col, int64_t N, const int32_t* ub, int64_t lds_max,
                            int64_t n_waves, float* acc, uint32_t* bits, int32_t* count, void* stream) {
  const int rc = two_hop_args("two_hop_count", rowptr, col, N, ub, lds_max, n_waves, acc, bits);
  if (rc != GNPDE_OK) return rc;
  if (N == 0) return GNPDE_OK;
  GNPDE_REQUIRE(count, GNPDE_EINVAL, "two_hop_count: NULL count");
  hipStream_t st = as_stream(stream);
  GNPDE_HIP(hipMemsetAsync(count, 0, sizeof(int32_t) * (size_t)N, st));
  two_hop_lds_kernel<false><<<two_hop_grid_lds(N), kBlock, 0, st>>>(rowptr, col, nullptr, (int)N, ub, (int)lds_max, count,
                                                                   nullptr, nullptr, nullptr, nullptr, 0);
  GNPDE_LAUNCH_CHECK();
  two_hop_dense_kernel<false><<<(unsigned)ceil_div(n_waves, kWavesPerBlock), kBlock, 0, st>>>(
      rowptr, col, nullptr, (int)N, ub, (int)lds_max, (int)n_waves, acc, bits, count, nullptr, nullptr, nullptr, nullptr,
      0);
  GNPDE_LAUNCH_CHECK();
  return GNPDE_OK;
}

int gnpde_two_hop_fill_f32(const int32_t* rowptr, const int32_t* col, const float* val, int64_t N, const int32_t* ub,
                           int64_t lds_max, int64_t n_waves, float* acc, uint32_t* bits, const int32_t* out_ptr,
                           int64_t nnz_out, int32_t* out_col, float* out_val, int64_t* out_ei, void* stream) {
  const int rc = two_hop_args("two_hop_fill", rowptr, col, N, ub, lds_max, n_waves, acc, bits);
  if (rc != GNPDE_OK) return rc;
  GNPDE_REQUIRE(nnz_out >= 0 && nnz_out < INT32_MAX, GNPDE_EINVAL, "two_hop_fill: nnz_out=%lld out of range",
                (long long)nnz_out);
  if (N == 0 || nnz_out == 0) return GNPDE_OK;
  GNPDE_REQUIRE(val && out_ptr && out_col && out_val && out_ei, GNPDE_EINVAL, "two_hop_fill: NULL argument");
  hipStream_t st = as_stream(stream);
  two_hop_lds_kernel<true><<<two_hop_grid_lds(N), kBlock, 0, st>>>(rowptr, col, val, (int)N, ub, (int)lds_max, nullptr,
                                                                  out_ptr, out_col, out_val, out_ei, nnz_out);
  GNPDE_LAUNCH_CHECK();
  two_hop_dense_kernel<true><<<(unsigned)ceil_div(n_waves, kWavesPerBlock), kBlock, 0, st>>>(
      rowptr, col, val, (int)N, ub, (int)lds_max, (int)n_waves, acc, bits, nullptr, out_ptr, out_col, out_val, out_ei,
      nnz_out);
  GNPDE_LAUNCH_CHECK();
  return GNPDE_OK;
}

}  // extern "C"
