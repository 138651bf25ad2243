// head_aggregate.hip — the per-head value aggregation of the transformer layer's
// mix_features branch (reference src/function_transformer_attention.py:23-32: the
// [B,h,N,N] attention times the [B,h,N,dk] values, head mean, then Wout):
//   z[r, d] = (1/H) sum over CSR positions p of row r, sum over heads h:
//                 w[p, h] * v[col[p], h*dk + d]                      z [R, dk]
// v [R, att = H*dk] is the value projection (head h owns columns h*dk .. h*dk+dk-1),
// w the per-head attention of every edge: in aggregation-CSR order [nnz, H] (perm NULL:
// what the RHS hands over, gnpde_edge_attention_csr_f32 / gnpde_squareplus_attention_csr_f32
// — measured 23-33 % faster with its producer than the other form), or an
// attention given in COO order [B,E,H], read through the CSR's perm (w[perm[p], h]).
// K1 (aggregate.hpp) takes one scalar weight per edge; this is the multi-head product.
//
// Work items are K1's (the plan of the aggregation CSR: a row of at most `chunk`
// edges, or a chunk of a hub row).  Fast path (dk % 4 == 0, att/4 a power of two up to
// 64 lanes, i.e. att <= 256, 16-byte aligned rows): one wavefront per item; NL = att/4
// lanes cover the att columns of an edge in 16-byte runs — a run lies inside one head,
// S = dk/4 runs per head — and the G = 64/NL lane groups take edges side by side, U per
// group in flight.  Per batch of 64 edges the loads go out in the order of their
// dependence: column ids (and perm), then each lane's weight of its edge and head (no
// dependence on the gathers: its latency lies behind them), then the v rows.  A lane
// accumulates w * v in fp32; at the end of the item the lanes holding the same d — the H
// heads of a group and the G groups — are summed by one xor tree over lane bits
// log2(S) .. 5 (fixed order), scaled by 1/H, and lanes 0 .. S-1 store the dk-wide row.
// Hub rows: each chunk stores its unscaled partial row write-through to its slot, takes
// an arrival ticket on the hub's plan entry (heavy[].w), and the last arrival sums the
// partials — lane groups of S lanes take chunks g, g + 64/S, ..., joined by the same xor
// tree — exactly K1's hand-off (hub_claim).  No float atomics, fixed summation orders:
// repeated launches give the same bits.
//
// Every other shape (dk % 4 != 0, heads not a power of two, att > 256, unaligned rows):
// head_agg_plain_kernel, one fp32 fma chain per output element over the row's edges in
// CSR order, heads innermost (correctness only).
#include "aggregate.hpp"

namespace gnpde {

constexpr int kHeadAggU = 4;  // edges in flight per lane group

template <int NL, int U>
__global__ __launch_bounds__(256) void head_agg_kernel(const int4* __restrict__ items, int n_items, int4* heavy,
                                                        int n_heavy, const int* __restrict__ col,
                                                        const int* __restrict__ perm, const float* __restrict__ wh,
                                                        int H, int lgS, const float* __restrict__ v, int64_t ldv,
                                                        float* __restrict__ z, int64_t ldz, float inv_h,
                                                        float* __restrict__ partials) {
  constexpr int G = kWave / NL;
  const int lane = threadIdx.x & 63;
  const int g = lane / NL, gl = lane % NL;
  const int wid = uniform(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
  if (wid >= n_items) return;
  const int4 it = items[wid];
  const int row = uniform(it.x), beg = uniform(it.y), end = uniform(it.z), slot = uniform(it.w);
  const int S = 1 << lgS;
  const int h = gl >> lgS;  // the head of this lane's 16-byte run

  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int e0 = beg; e0 < end; e0 += kWave) {
    const int n = min(kWave, end - e0);
    int mc = 0, mp = 0;
    if (lane < n) {
      mc = col[e0 + lane];
      mp = perm ? perm[e0 + lane] : e0 + lane;
    }
    for (int j = 0; j < n; j += G * U) {
      float ww[U];
      float4 vv[U];
      int c[U];
      bool ok[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int jj = j + u * G + g;
        ok[u] = jj < n;
        const int src = ok[u] ? jj : 0;
        const int p = __shfl(mp, src);
        c[u] = __shfl(mc, src);
        ww[u] = ok[u] ? wh[(int64_t)p * H + h] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        vv[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok[u]) vv[u] = *reinterpret_cast<const float4*>(v + (int64_t)c[u] * ldv + gl * 4);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        acc[0] = fmaf(ww[u], vv[u].x, acc[0]);
        acc[1] = fmaf(ww[u], vv[u].y, acc[1]);
        acc[2] = fmaf(ww[u], vv[u].z, acc[2]);
        acc[3] = fmaf(ww[u], vv[u].w, acc[3]);
      }
    }
  }
  // the lanes holding the same d: the heads of a group (bits log2 S .. log2 NL - 1) and the groups
  for (int o = S; o < kWave; o <<= 1)
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] += __shfl_xor(acc[t], o);

  if (slot < 0) {  // a whole row
    if (lane < S)
      *reinterpret_cast<float4*>(z + (int64_t)row * ldz + lane * 4) =
          make_float4(acc[0] * inv_h, acc[1] * inv_h, acc[2] * inv_h, acc[3] * inv_h);
    return;
  }
  if (n_heavy <= 0) return;  // (no plan holds a chunk without its hub entry)
  // a hub chunk: the unscaled partial row write-through, then the arrival ticket (K1's hub_claim)
  const int dk = 4 * S;
  const __amdgpu_buffer_rsrc_t rp = buf_rsrc(partials);
  buf_store_wt<4>(rp, lane < S ? (uint32_t)(((int64_t)slot * dk + lane * 4) * 4) : kBufNone, acc);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  int lo = 0, hi = n_heavy - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (heavy[mid].y <= slot)
      lo = mid;
    else
      hi = mid - 1;
  }
  int won = 0;
  if (lane == 0) {
    const int t = __hip_atomic_fetch_add(&heavy[lo].w, 1, kHubTicketOrder, __HIP_MEMORY_SCOPE_AGENT);
    won = t == heavy[lo].z - 1;
  }
  if (!__shfl(won, 0)) return;  // wave-uniform
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  const int4 hv = heavy[lo];
  const int hrow = uniform(hv.x), first = uniform(hv.y), nch = uniform(hv.z);
  const int gs = lane & (S - 1);
  float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int ch = lane >> lgS; ch < nch; ch += kWave >> lgS) {
    const float4 pv = *reinterpret_cast<const float4*>(partials + (int64_t)(first + ch) * dk + gs * 4);
    s[0] += pv.x;
    s[1] += pv.y;
    s[2] += pv.z;
    s[3] += pv.w;
  }
  for (int o = S; o < kWave; o <<= 1)
#pragma unroll
    for (int t = 0; t < 4; ++t) s[t] += __shfl_xor(s[t], o);
  if (lane < S)
    *reinterpret_cast<float4*>(z + (int64_t)hrow * ldz + lane * 4) =
        make_float4(s[0] * inv_h, s[1] * inv_h, s[2] * inv_h, s[3] * inv_h);
  if (lane == 0) __hip_atomic_store(&heavy[lo].w, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Any heads >= 1, dk >= 1: one thread per output element, the row's edges in CSR order, heads innermost.
__global__ __launch_bounds__(256) void head_agg_plain_kernel(const int* __restrict__ rowptr,
                                                              const int* __restrict__ col,
                                                              const int* __restrict__ perm, int64_t R,
                                                              const float* __restrict__ wh, int H, int dk,
                                                              const float* __restrict__ v, int64_t ldv,
                                                              float* __restrict__ z, int64_t ldz, float inv_h) {
  const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (idx >= R * dk) return;
  const int64_t row = idx / dk;
  const int d = (int)(idx - row * dk);
  float acc = 0.f;
  for (int p = rowptr[row]; p < rowptr[row + 1]; ++p) {
    const float* __restrict__ vr = v + (int64_t)col[p] * ldv + d;
    const float* __restrict__ wr = wh + (int64_t)(perm ? perm[p] : p) * H;
    for (int h = 0; h < H; ++h) acc = fmaf(wr[h], vr[h * dk], acc);
  }
  z[row * ldz + d] = acc * inv_h;
}

static bool head_agg_shape_fast(int64_t heads, int64_t dk) {
  const int64_t att = heads * dk;
  if (heads < 1 || dk < 4 || dk % 4 || att > 4 * kWave) return false;
  const int64_t nl = att / 4;
  return (nl & (nl - 1)) == 0 && (heads & (heads - 1)) == 0;
}

}  // namespace gnpde

using namespace gnpde;

extern "C" {

int gnpde_head_aggregate_fast(int64_t heads, int64_t dk) { return head_agg_shape_fast(heads, dk) ? 1 : 0; }

int64_t gnpde_head_aggregate_workspace_floats(int64_t dk, int64_t n_slots) {
  return (dk < 1 || n_slots < 1) ? 0 : n_slots * dk;
}

int gnpde_head_aggregate_f32(const int32_t* items, int64_t n_items, int32_t* heavy, int64_t n_heavy,
                             const int32_t* rowptr, const int32_t* col, const int32_t* perm, int64_t R,
                             const float* wh, int64_t heads, int64_t dk, const float* v, int64_t ldv, float* z,
                             int64_t ldz, float* workspace, int64_t n_slots, void* stream) {
  GNPDE_REQUIRE(heads >= 1 && heads < (1 << 20) && dk >= 1 && dk < (1 << 20), GNPDE_EINVAL,
                "head_aggregate: bad heads / dk");
  GNPDE_REQUIRE(R >= 0 && R < INT32_MAX && n_items >= 0 && n_items < INT32_MAX && n_heavy >= 0 &&
                    n_heavy < INT32_MAX && n_slots >= 0,
                GNPDE_EINVAL, "head_aggregate: bad sizes");
  GNPDE_REQUIRE(ldv >= heads * dk && ldz >= dk, GNPDE_EINVAL, "head_aggregate: leading dimensions below the widths");
  if (R == 0) return GNPDE_OK;
  GNPDE_REQUIRE(rowptr && col && wh && v && z, GNPDE_EINVAL, "head_aggregate: NULL pointer");
  GNPDE_REQUIRE(z != v && z != wh, GNPDE_EINVAL, "head_aggregate: z aliases an input");
  hipStream_t s = as_stream(stream);
  const float inv_h = 1.f / (float)heads;
  const bool fast = head_agg_shape_fast(heads, dk) && items && aligned16(v) && ldv % 4 == 0 && aligned16(z) &&
                    ldz % 4 == 0 && (n_heavy == 0 || aligned16(workspace));
  if (fast) {
    GNPDE_REQUIRE(n_heavy == 0 || (heavy && workspace && n_slots > 0), GNPDE_EINVAL,
                  "head_aggregate: hub rows need heavy and the workspace");
    GNPDE_REQUIRE(n_slots * dk * 4 < (int64_t)kBufRecords, GNPDE_EUNSUPPORTED,
                  "head_aggregate: %lld partial slots exceed the 4 GiB of 32-bit buffer offsets", (long long)n_slots);
    if (n_items == 0) return GNPDE_OK;
    const int4* it = reinterpret_cast<const int4*>(items);
    int4* hv = reinterpret_cast<int4*>(heavy);
    const int S = (int)(dk / 4);
    int lgS = 0;
    while ((1 << lgS) < S) ++lgS;
    const unsigned grid = (unsigned)ceil_div(n_items, (int64_t)kWavesPerBlock);
#define GNPDE_HAGG(NL)                                                                                     \
  head_agg_kernel<NL, kHeadAggU><<<grid, kBlock, 0, s>>>(it, (int)n_items, hv, (int)n_heavy, col, perm, wh, \
                                                         (int)heads, lgS, v, ldv, z, ldz, inv_h, workspace)
    switch ((int)(heads * dk / 4)) {
      case 1: GNPDE_HAGG(1); break;
      case 2: GNPDE_HAGG(2); break;
      case 4: GNPDE_HAGG(4); break;
      case 8: GNPDE_HAGG(8); break;
      case 16: GNPDE_HAGG(16); break;
      case 32: GNPDE_HAGG(32); break;
      default: GNPDE_HAGG(64); break;
    }
#undef GNPDE_HAGG
    GNPDE_LAUNCH_CHECK();
    return GNPDE_OK;
  }
  const int64_t nblk = ceil_div(R * dk, (int64_t)kBlock);
  GNPDE_REQUIRE(nblk < INT32_MAX, GNPDE_EUNSUPPORTED,
                "head_aggregate: %lld x %lld outputs exceed the plain kernel's grid", (long long)R, (long long)dk);
  head_agg_plain_kernel<<<(unsigned)nblk, kBlock, 0, s>>>(rowptr, col, perm, R, wh, (int)heads, (int)dk, v, ldv, z,
                                                          ldz, inv_h);
  GNPDE_LAUNCH_CHECK();
  return GNPDE_OK;
}

}  // extern "C"
