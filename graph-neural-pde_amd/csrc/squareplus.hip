// squareplus.hip — the squareplus attention normaliser (opt['square_plus'], src/utils.py:129-140).
//
//   M_b      = max over all edges e and heads h of s[b,e,h]        (one scalar per batch element)
//   p        = squareplus_p(s - M_b)                               (scores.hpp; in (0, 1])
//   L[g,h]   = sum of p over the edges of group g,  rl = 1 / (L + 1e-16)
//   att[e,h] = p[e,h] * rl[g(e),h],   w[e] = mean_h att[e,h]
//
// Unlike the softmax, the shift M_b is part of the function (squareplus is not
// shift-invariant), it is global per batch element, and it is one more dependency in front
// of the statistics.  The passes:
//   1. gnpde_score_max_f32        M [B] (fp64) and the first arg-max position; workgroup
//                                 partials + a final pass (a total order on (value, index):
//                                 any reduction order gives the same result; no atomics).
//                                 Per-edge score modes store the scores [nnz, H] (COO order)
//                                 once, so no later pass repeats the dk-long products.
//   2. gnpde_squareplus_stats_f32 rl [R,H] over a plan of the groups' rows (hub groups in
//                                 chunk items + a fixed-order merge).  Reference scores: p is
//                                 a per-node array pn [R,H] (formed here), the statistics a
//                                 gather-sum of it.
//   3. gnpde_squareplus_weights_f32 / _attention_f32: edge-parallel from (M, rl); the fused K1
//                                 (gnpde_attn_sp_rhs_f32: RefDstSquareplusWeights, aggregate.hpp)
//                                 forms the reference-score weights in its gather loop.
//   4. gnpde_squareplus_backward_f32: dL/ds from dL/datt, including the max term.
#include <algorithm>
#include <climits>

#include "aggregate.hpp"
#include "rhs_host.hpp"

namespace gnpde {

constexpr int kSpMaxBlocks = 1024;  // workgroup partials per batch element (score max, backward sum)
constexpr int kSpTeamEdges = 4;    // edges a team scores side by side (their q / k rows in flight together)

// (value, index) pairs ordered by value, ties by the smaller index: a total order, so the
// maximum does not depend on the order of the reduction.
__device__ __forceinline__ void mi_take(double& v, long long& i, double v2, long long i2) {
  if (v2 > v || (v2 == v && i2 < i)) {
    v = v2;
    i = i2;
  }
}

__device__ __forceinline__ void mi_block(double& v, long long& i, double* sv, long long* si) {
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const double v2 = __shfl_xor(v, o);
    const long long i2 = __shfl_xor(i, o);
    mi_take(v, i, v2, i2);
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) {
    sv[w] = v;
    si[w] = i;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < kWavesPerBlock; ++k) mi_take(v, i, sv[k], si[k]);
  }
}

// NODE (reference scores): batch element blockIdx.y, its rows with at least one out-edge;
// the index of node score (r, h) is the COO position of the row's first edge.
// !NODE (per-edge scores): the CSR positions of batch element blockIdx.y; scores stored to
// sc[e*H + h] (COO order) when sc is given.
template <bool NODE>
__global__ __launch_bounds__(256) void score_max_kernel(const int* __restrict__ rowptr, const int* __restrict__ rowidx,
                                                         const int* __restrict__ col, const int* __restrict__ perm,
                                                         int64_t N, ScoreArgs sa, float* __restrict__ sc,
                                                         double* __restrict__ pv, long long* __restrict__ pi) {
  __shared__ double sv[kWavesPerBlock];
  __shared__ long long si[kWavesPerBlock];
  const int64_t b = blockIdx.y;
  const int H = sa.H;
  double v = -INFINITY;
  long long i = LLONG_MAX;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if constexpr (NODE) {
    for (int64_t r = b * N + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < (b + 1) * N; r += stride) {
      const int p0 = rowptr[r];
      if (rowptr[r + 1] <= p0) continue;
      const long long e = perm[p0];
      for (int h = 0; h < H; ++h) mi_take(v, i, sa.cs[r * H + h], e * H + h);
    }
  } else {
    const int64_t beg = rowptr[b * N], end = rowptr[(b + 1) * N];
    for (int64_t p = beg + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < end; p += stride) {
      const int r = rowidx[p], c = col[p];
      const long long e = perm[p];
      for (int h = 0; h < H; ++h) {
        const float s = pair_score(sa.mode, sa.q + (int64_t)r * sa.ldqk + h * sa.dk,
                                   sa.k + (int64_t)c * sa.ldqk + h * sa.dk, sa.dk, sa.p0, sa.p1);
        if (sc) sc[e * H + h] = s;
        mi_take(v, i, (double)s, e * H + h);
      }
    }
  }
  mi_block(v, i, sv, si);
  if (threadIdx.x == 0) {
    pv[b * gridDim.x + blockIdx.x] = v;
    pi[b * gridDim.x + blockIdx.x] = i;
  }
}

// Per-edge scores in team mode (scores.hpp: T lanes per edge, 16-byte slices of the q / k
// rows, so an edge's rows are read as whole cache lines instead of one float per lane and
// step): a team takes T consecutive CSR positions of batch element blockIdx.y (indices
// loaded one per lane), then scores them kSpTeamEdges at a time.  Trip counts are
// wave-uniform (the shuffles of team_score_regs run with every lane active), as in
// attn_team_kernel (node_scores.hip); the scores are those of the team-mode weights kernels.
template <int VEC>
__global__ __launch_bounds__(256) void score_max_team_kernel(const int* __restrict__ rowptr,
                                                              const int* __restrict__ rowidx,
                                                              const int* __restrict__ col,
                                                              const int* __restrict__ perm, int64_t N, ScoreArgs sa,
                                                              Team tm, float* __restrict__ sc,
                                                              double* __restrict__ pv, long long* __restrict__ pi) {
  __shared__ double sv[kWavesPerBlock];
  __shared__ long long si[kWavesPerBlock];
  const int lane = threadIdx.x & 63;
  const int T = tm.T, S = tm.S, tpw = kWave / T;
  const int team = lane / T, t = lane % T, h = t / S;
  const int H = sa.H;
  const bool leader = (t % S) == 0;
  const int64_t b = blockIdx.y;
  const int64_t beg = rowptr[b * N], end = rowptr[(b + 1) * N];
  double v = -INFINITY;
  long long i = LLONG_MAX;
  const int64_t wave_first = beg + (int64_t)(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6)) * tpw * T;
  const int64_t sweep = (int64_t)gridDim.x * kWavesPerBlock * tpw * T;
  for (int64_t w0 = wave_first; w0 < end; w0 += sweep) {
    const int64_t p0 = w0 + (int64_t)team * T;
    const int cnt = (int)max((int64_t)0, min((int64_t)T, end - p0));
    int my_r = 0, my_c = 0, my_e = 0;
    if (cnt > 0) {
      const int64_t pm = p0 + min(t, cnt - 1);
      my_r = rowidx[pm];
      my_c = col[pm];
      my_e = perm[pm];
    }
    const int jmax = wave_max_int(cnt);
    for (int j = 0; j < jmax; j += kSpTeamEdges) {
      float qv[kSpTeamEdges][VEC], kv[kSpTeamEdges][VEC];
      int ev[kSpTeamEdges];
#pragma unroll
      for (int u = 0; u < kSpTeamEdges; ++u) {
        const int src = team * T + max(0, min(j + u, cnt - 1));
        const int r = __shfl(my_r, src), c = __shfl(my_c, src);
        ev[u] = __shfl(my_e, src);
        team_row<VEC>(sa, sa.q, r, t, qv[u]);
        team_row<VEC>(sa, sa.k, c, t, kv[u]);
      }
#pragma unroll
      for (int u = 0; u < kSpTeamEdges; ++u) {
        const float s = team_score_regs<VEC>(sa, qv[u], kv[u], S);
        if (leader && j + u < cnt) {
          const long long at = (long long)ev[u] * H + h;
          if (sc) sc[at] = s;
          mi_take(v, i, (double)s, at);
        }
      }
    }
  }
  mi_block(v, i, sv, si);
  if (threadIdx.x == 0) {
    pv[b * gridDim.x + blockIdx.x] = v;
    pi[b * gridDim.x + blockIdx.x] = i;
  }
}

// one workgroup per batch element: M[b], amax[b] from its nb partials (0, -1 without edges)
__global__ __launch_bounds__(256) void score_max_final_kernel(const double* __restrict__ pv,
                                                               const long long* __restrict__ pi, int nb,
                                                               double* __restrict__ M, long long* __restrict__ amax) {
  __shared__ double sv[kWavesPerBlock];
  __shared__ long long si[kWavesPerBlock];
  const int64_t b = blockIdx.x;
  double v = -INFINITY;
  long long i = LLONG_MAX;
  for (int k = threadIdx.x; k < nb; k += blockDim.x) mi_take(v, i, pv[b * nb + k], pi[b * nb + k]);
  mi_block(v, i, sv, si);
  if (threadIdx.x == 0) {
    const bool any = i != LLONG_MAX;
    M[b] = any ? v : 0.0;
    if (amax) amax[b] = any ? i : -1;
  }
}

// pn[r,h] = squareplus_p(cs[r,h] - M_b): the difference in fp64, then cast.  Rows without
// out-edges are outside the max and may exceed it: clamped to 0 (never gathered).
__global__ __launch_bounds__(256) void squareplus_node_kernel(const double* __restrict__ cs, int64_t R, int64_t N,
                                                               int H, const double* __restrict__ M,
                                                               float* __restrict__ pn) {
  const int64_t n = R * H;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = (i / H) / N;
    pn[i] = squareplus_p(fminf((float)(cs[i] - M[b]), 0.f));
  }
}

// Group sums over a plan of the groups' rows (items {row, e_begin, e_end, slot}): 16 lanes
// per item, four items per wavefront; lanes take the item's edges strided — the index once,
// then every head (H <= MAXH) — fp64 partial sums, a fixed xor tree.  Whole rows (slot < 0)
// store rl; chunks of a hub row store their sums to partials[slot*H + h] for
// squareplus_hub_kernel.
template <bool NODE, int MAXH>
__global__ __launch_bounds__(256) void squareplus_stats_kernel(const int4* __restrict__ items, int n_items,
                                                                const int* __restrict__ gcol,
                                                                const int* __restrict__ gperm, int group_is_dst,
                                                                int64_t N, int H, const float* __restrict__ pn,
                                                                const float* __restrict__ sc,
                                                                const double* __restrict__ M, float* __restrict__ rl,
                                                                double* __restrict__ partials) {
  constexpr int SL = 16;
  const int lane = threadIdx.x & 63, sl = lane % SL;
  const int64_t item = ((int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6)) * (kWave / SL) + lane / SL;
  const bool live = item < n_items;
  const int4 it = live ? items[item] : make_int4(0, 0, 0, -1);
  const int row = it.x;
  const float Mb = NODE ? 0.f : (float)M[row / N];
  double s[MAXH];
#pragma unroll
  for (int h = 0; h < MAXH; ++h) s[h] = 0.0;
  for (int p = it.y + sl; p < it.z; p += SL) {
    const int64_t at = NODE ? (group_is_dst ? gcol[p] : row) : gperm[p];
    const float* __restrict__ src = (NODE ? pn : sc) + at * H;
#pragma unroll
    for (int h = 0; h < MAXH; ++h)
      if (h < H) s[h] += (double)(NODE ? src[h] : squareplus_p(src[h] - Mb));
  }
#pragma unroll
  for (int h = 0; h < MAXH; ++h) {
#pragma unroll
    for (int o = 1; o < SL; o <<= 1) s[h] += __shfl_xor(s[h], o);
    if (live && sl == 0 && h < H) {
      if (it.w < 0)
        rl[(int64_t)row * H + h] = (float)(1.0 / (s[h] + 1e-16));
      else
        partials[(int64_t)it.w * H + h] = s[h];
    }
  }
}

template <bool NODE>
static void launch_sp_stats(unsigned grid, hipStream_t s, const int4* it, int n_items, const int* gcol,
                            const int* gperm, int group_is_dst, int64_t N, int H, const float* pn, const float* sc,
                            const double* M, float* rl, double* partials) {
#define GNPDE_SPS(MH) \
  squareplus_stats_kernel<NODE, MH><<<grid, kBlock, 0, s>>>(it, n_items, gcol, gperm, group_is_dst, N, H, pn, sc, M, rl, \
                                                            partials)
  if (H <= 2)
    GNPDE_SPS(2);
  else if (H <= 4)
    GNPDE_SPS(4);
  else if (H <= 8)
    GNPDE_SPS(8);
  else
    GNPDE_SPS(16);
#undef GNPDE_SPS
}

// one wavefront per hub group {row, first_slot, n_chunks, -}: its chunk sums in a fixed order
__global__ __launch_bounds__(256) void squareplus_hub_kernel(const int4* __restrict__ heavy, int n_heavy, int H,
                                                              const double* __restrict__ partials,
                                                              float* __restrict__ rl) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (w >= n_heavy) return;
  const int4 hv = heavy[w];
  for (int h = 0; h < H; ++h) {
    double s = 0.0;
    for (int c = lane; c < hv.z; c += kWave) s += partials[(int64_t)(hv.y + c) * H + h];
    s = wave_sum(s);
    if (lane == 0) rl[(int64_t)hv.x * H + h] = (float)(1.0 / (s + 1e-16));
  }
}

// Edge-parallel over the aggregation CSR (rowidx = source, col = destination, perm -> COO):
// att[e,h] = p * rl[g,h] (COO; att_csr: att[p,h], CSR order — the per-head weights of
// gnpde_head_aggregate_f32) and / or the head-mean weight w[p] (CSR order).
template <bool NODE>
__global__ __launch_bounds__(256) void squareplus_edge_kernel(const int* __restrict__ rowidx,
                                                               const int* __restrict__ col,
                                                               const int* __restrict__ perm, int64_t nnz, int64_t N,
                                                               int norm_idx, int H, const float* __restrict__ pn,
                                                               const float* __restrict__ sc,
                                                               const double* __restrict__ M,
                                                               const float* __restrict__ rl, float* __restrict__ w_out,
                                                               float* __restrict__ att, int att_csr) {
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < nnz; p += (int64_t)gridDim.x * blockDim.x) {
    const int r = rowidx[p], c = col[p];
    const int64_t e = perm[p];
    const int64_t g = norm_idx ? c : r;
    const float Mb = NODE ? 0.f : (float)M[r / N];
    float acc = 0.f;
    for (int h = 0; h < H; ++h) {
      const float pv = NODE ? pn[(int64_t)r * H + h] : squareplus_p(sc[e * H + h] - Mb);
      const float rg = rl[g * H + h];
      if (att) att[(att_csr ? p : e) * H + h] = pv * rg;
      acc = squareplus_mean_step(pv, rg, acc);
    }
    if (w_out) w_out[p] = acc / (float)H;
  }
}

// Backward, first pass: one wavefront per group, every head.  With p = att / rl and
// r = sqrt(s'^2 + 4) = p + 1/p:  gs'[e,h] = att / r * (g - sum over the group of att * g).
__global__ __launch_bounds__(256) void squareplus_backward_kernel(const int* __restrict__ rowptr,
                                                                   const int* __restrict__ perm, int64_t R, int H,
                                                                   const float* __restrict__ att,
                                                                   const float* __restrict__ g,
                                                                   const float* __restrict__ rl,
                                                                   float* __restrict__ gs) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / kWave;
  const int64_t nwaves = (int64_t)gridDim.x * blockDim.x / kWave;
  for (int64_t r = wave; r < R; r += nwaves) {
    const int b = rowptr[r], e = rowptr[r + 1];
    for (int h = 0; h < H; ++h) {
      double d = 0.0;
      for (int p = b + lane; p < e; p += kWave) {
        const int64_t i = (int64_t)perm[p] * H + h;
        d = fma((double)att[i], (double)g[i], d);
      }
      d = wave_sum(d);
      const double rg = (double)rl[r * H + h];
      for (int p = b + lane; p < e; p += kWave) {
        const int64_t i = (int64_t)perm[p] * H + h;
        const double a = (double)att[i];
        const double pv = a / rg;
        const double rr = pv + 1.0 / pv;  // att = 0 (p underflowed): rr = inf, gs' = 0
        gs[i] = a > 0.0 ? (float)(a / rr * ((double)g[i] - d)) : 0.f;
      }
    }
  }
}

// Backward, the max term: part[b][blk] = the block's share of sum_{e,h} gs'[b] (fp64, fixed order)
__global__ __launch_bounds__(256) void squareplus_gsum_kernel(const float* __restrict__ gs, int64_t per_batch,
                                                               double* __restrict__ part) {
  __shared__ double sw[kWavesPerBlock];
  const int64_t b = blockIdx.y;
  const float* __restrict__ v = gs + b * per_batch;
  double s = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < per_batch; i += (int64_t)gridDim.x * blockDim.x)
    s += (double)v[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int k = 0; k < kWavesPerBlock; ++k) t += sw[k];
    part[b * gridDim.x + blockIdx.x] = t;
  }
}

// gs[amax[b]] -= sum of the batch element's gs' (the derivative of -M_b lands on the arg-max)
__global__ __launch_bounds__(64) void squareplus_gmax_kernel(const double* __restrict__ part, int nb,
                                                              const long long* __restrict__ amax,
                                                              float* __restrict__ gs) {
  const int64_t b = blockIdx.x;
  double s = 0.0;
  for (int k = threadIdx.x; k < nb; k += kWave) s += part[b * nb + k];
  s = wave_sum(s);
  if (threadIdx.x == 0 && amax[b] >= 0) gs[amax[b]] = (float)((double)gs[amax[b]] - s);
}

static unsigned sp_grid(int64_t n, int64_t cap) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(n, kBlock), cap));
}

static int sp_mode_check(int mode, const char* what) {
  GNPDE_REQUIRE(mode >= GNPDE_SCORE_REFERENCE && mode <= GNPDE_SCORE_GAT, GNPDE_EINVAL, "%s: unknown score mode %d",
                what, mode);
  GNPDE_REQUIRE(mode != GNPDE_SCORE_UNIFORM && mode != GNPDE_SCORE_GAT, GNPDE_EUNSUPPORTED,
                "%s: squareplus takes the transformer score modes (uniform scores keep 1/outdeg; GAT is softmax only)",
                what);
  return GNPDE_OK;
}

}  // namespace gnpde

using namespace gnpde;

extern "C" {

size_t gnpde_score_max_workspace_bytes(int64_t B) {
  return (sizeof(double) + sizeof(long long)) * (size_t)kSpMaxBlocks * (size_t)(B > 0 ? B : 1);
}

int gnpde_score_max_f32(const int32_t* rowptr, const int32_t* rowidx, const int32_t* col, const int32_t* perm,
                        int64_t B, int64_t N, int64_t E, int mode, int64_t heads, int64_t dk, const double* cs,
                        const float* q, const float* k, int64_t ldqk, float score_p0, float score_p1, double* M,
                        int64_t* amax, float* sc, void* workspace, size_t workspace_bytes, void* stream) {
  int rc = sp_mode_check(mode, "score_max");
  if (rc) return rc;
  rc = check_score_args(mode, heads, dk, cs, q, k);
  if (rc) return rc;
  GNPDE_REQUIRE(B >= 1 && N >= 1 && E >= 0 && B <= 65535, GNPDE_EINVAL, "score_max: bad sizes");
  GNPDE_REQUIRE(B * E * heads < (int64_t)INT32_MAX * 64, GNPDE_EUNSUPPORTED, "score_max: too many scores");
  GNPDE_REQUIRE(M && workspace && workspace_bytes >= gnpde_score_max_workspace_bytes(B), GNPDE_EINVAL,
                "score_max: NULL output or workspace too small");
  GNPDE_REQUIRE(E == 0 || (rowptr && rowidx && col && perm), GNPDE_EINVAL, "score_max: NULL graph");
  hipStream_t s = as_stream(stream);
  const ScoreArgs sa = make_score_args(mode, heads, dk, cs, q, k, ldqk, score_p0, score_p1);
  double* pv = static_cast<double*>(workspace);
  long long* pi = reinterpret_cast<long long*>(pv + (size_t)kSpMaxBlocks * B);
  const bool node = mode == GNPDE_SCORE_REFERENCE;
  const unsigned nb = sp_grid(node ? N : E, kSpMaxBlocks);
  const dim3 grid(nb, (unsigned)B);
  const Team tm = node ? Team{0, 0} : team_geometry(sa);
  if (node)
    score_max_kernel<true><<<grid, kBlock, 0, s>>>(rowptr, rowidx, col, perm, N, sa, nullptr, pv, pi);
  else if (tm.T > 0)  // a block sweeps kBlock edges at a time in either form: the same grid
    score_max_team_kernel<4><<<grid, kBlock, 0, s>>>(rowptr, rowidx, col, perm, N, sa, tm, sc, pv, pi);
  else
    score_max_kernel<false><<<grid, kBlock, 0, s>>>(rowptr, rowidx, col, perm, N, sa, sc, pv, pi);
  GNPDE_LAUNCH_CHECK();
  score_max_final_kernel<<<(unsigned)B, kBlock, 0, s>>>(pv, pi, (int)nb, M, reinterpret_cast<long long*>(amax));
  GNPDE_LAUNCH_CHECK();
  return GNPDE_OK;
}

int gnpde_squareplus_stats_f32(const int32_t* items, int64_t n_items, const int32_t* heavy, int64_t n_heavy,
                               const int32_t* gcol, const int32_t* gperm, int group_is_dst, int64_t R, int64_t N,
                               int mode, int64_t heads, const double* cs, const float* sc, const double* M, float* pn,
                               float* rl, double* partials, void* stream) {
  int rc = sp_mode_check(mode, "squareplus_stats");
  if (rc) return rc;
  GNPDE_REQUIRE(heads >= 1 && heads <= 16, GNPDE_EUNSUPPORTED, "squareplus_stats: heads=%lld not in [1,16]",
                (long long)heads);
  GNPDE_REQUIRE(R >= 1 && N >= 1 && R % N == 0 && n_items >= 0 && n_items < INT32_MAX && n_heavy >= 0 &&
                n_heavy < INT32_MAX, GNPDE_EINVAL, "squareplus_stats: bad sizes");
  GNPDE_REQUIRE(M && rl, GNPDE_EINVAL, "squareplus_stats: NULL M / rl");
  GNPDE_REQUIRE(n_heavy == 0 || (heavy && partials), GNPDE_EINVAL, "squareplus_stats: hub groups need partials");
  const bool node = mode == GNPDE_SCORE_REFERENCE;
  GNPDE_REQUIRE(node ? (cs && pn) : (sc != nullptr), GNPDE_EINVAL,
                "squareplus_stats: reference scores need cs and pn, per-edge scores the stored scores");
  hipStream_t s = as_stream(stream);
  if (node) {
    squareplus_node_kernel<<<sp_grid(R * heads, 4096), kBlock, 0, s>>>(cs, R, N, (int)heads, M, pn);
    GNPDE_LAUNCH_CHECK();
  }
  if (n_items == 0) return GNPDE_OK;
  GNPDE_REQUIRE(items && gcol && gperm, GNPDE_EINVAL, "squareplus_stats: NULL plan / graph");
  const int4* it = reinterpret_cast<const int4*>(items);
  const unsigned grid = (unsigned)ceil_div(n_items, (int64_t)kWavesPerBlock * (kWave / 16));
  if (node)
    launch_sp_stats<true>(grid, s, it, (int)n_items, gcol, gperm, group_is_dst, N, (int)heads, pn, sc, M, rl, partials);
  else
    launch_sp_stats<false>(grid, s, it, (int)n_items, gcol, gperm, group_is_dst, N, (int)heads, pn, sc, M, rl, partials);
  GNPDE_LAUNCH_CHECK();
  if (n_heavy > 0) {
    squareplus_hub_kernel<<<(unsigned)ceil_div(n_heavy, kWavesPerBlock), kBlock, 0, s>>>(
        reinterpret_cast<const int4*>(heavy), (int)n_heavy, (int)heads, partials, rl);
    GNPDE_LAUNCH_CHECK();
  }
  return GNPDE_OK;
}

static int squareplus_edges(const char* what, const int32_t* rowidx, const int32_t* col, const int32_t* perm,
                            int64_t nnz, int64_t N, int norm_idx, int mode, int64_t heads, const float* pn,
                            const float* sc, const double* M, const float* rl, float* w_out, float* att, void* stream,
                            bool att_csr = false) {
  int rc = sp_mode_check(mode, what);
  if (rc) return rc;
  GNPDE_REQUIRE(heads >= 1 && heads <= 16, GNPDE_EUNSUPPORTED, "%s: heads=%lld not in [1,16]", what, (long long)heads);
  GNPDE_REQUIRE(norm_idx == 0 || norm_idx == 1, GNPDE_EINVAL, "%s: norm_idx must be 0 or 1", what);
  GNPDE_REQUIRE(nnz >= 0 && N >= 1, GNPDE_EINVAL, "%s: bad sizes", what);
  if (nnz == 0) return GNPDE_OK;
  const bool node = mode == GNPDE_SCORE_REFERENCE;
  GNPDE_REQUIRE(rowidx && col && perm && M && rl && (w_out || att) && (node ? pn != nullptr : sc != nullptr),
                GNPDE_EINVAL, "%s: NULL pointer", what);
  const unsigned grid = sp_grid(nnz, 16384);
  if (node)
    squareplus_edge_kernel<true><<<grid, kBlock, 0, as_stream(stream)>>>(rowidx, col, perm, nnz, N, norm_idx,
                                                                         (int)heads, pn, sc, M, rl, w_out, att,
                                                                         (int)att_csr);
  else
    squareplus_edge_kernel<false><<<grid, kBlock, 0, as_stream(stream)>>>(rowidx, col, perm, nnz, N, norm_idx,
                                                                          (int)heads, pn, sc, M, rl, w_out, att,
                                                                          (int)att_csr);
  GNPDE_LAUNCH_CHECK();
  return GNPDE_OK;
}

int gnpde_squareplus_weights_f32(const int32_t* rowidx, const int32_t* col, const int32_t* perm, int64_t nnz,
                                 int64_t N, int norm_idx, int mode, int64_t heads, const float* pn, const float* sc,
                                 const double* M, const float* rl, float* w_out, void* stream) {
  return squareplus_edges("squareplus_weights", rowidx, col, perm, nnz, N, norm_idx, mode, heads, pn, sc, M, rl,
                          w_out, nullptr, stream);
}

int gnpde_squareplus_attention_f32(const int32_t* rowidx, const int32_t* col, const int32_t* perm, int64_t nnz,
                                   int64_t N, int norm_idx, int mode, int64_t heads, const float* pn, const float* sc,
                                   const double* M, const float* rl, float* att, void* stream) {
  return squareplus_edges("squareplus_attention", rowidx, col, perm, nnz, N, norm_idx, mode, heads, pn, sc, M, rl,
                          nullptr, att, stream);
}

int gnpde_squareplus_attention_csr_f32(const int32_t* rowidx, const int32_t* col, const int32_t* perm, int64_t nnz,
                                       int64_t N, int norm_idx, int mode, int64_t heads, const float* pn,
                                       const float* sc, const double* M, const float* rl, float* att, void* stream) {
  return squareplus_edges("squareplus_attention_csr", rowidx, col, perm, nnz, N, norm_idx, mode, heads, pn, sc, M, rl,
                          nullptr, att, stream, true);
}

int gnpde_attn_sp_rhs_f32(const int32_t* items, int64_t n_items, int32_t* heavy, int64_t n_heavy, const int32_t* col,
                          const float* pn, const float* rl, int64_t heads, int64_t C, const float* x, int64_t ldx,
                          const float* x0, int64_t ldx0, const float* alpha, const float* beta, int flags, float* f,
                          int64_t ldf, float* partials, int64_t n_slots, const gnpde_stage_epilogue_t* stage,
                          void* stream) {
  const Epi ep = make_epi(x, ldx, x0, ldx0, alpha, beta, flags, f, ldf, stage);
  int rc = check_epi(ep, C, n_heavy, partials, n_slots);
  if (rc) return rc;
  GNPDE_REQUIRE(heads >= 1 && heads <= 16, GNPDE_EUNSUPPORTED, "attn_sp_rhs: heads=%lld not in [1,16]",
                (long long)heads);
  GNPDE_REQUIRE(n_items >= 0 && n_items < INT32_MAX && n_heavy >= 0, GNPDE_EINVAL, "attn_sp_rhs: bad item counts");
  GNPDE_REQUIRE(n_items == 0 || (items && col && pn && rl), GNPDE_EINVAL, "attn_sp_rhs: NULL plan/col/p/statistics");
  if (heads <= 2) {
    RefDstSquareplusWeights<2> wp{pn, rl, (int)heads};
    return launch_agg(items, n_items, heavy, n_heavy, col, wp, C, ep, partials, as_stream(stream));
  }
  RefDstSquareplusWeights<0> wp{pn, rl, (int)heads};
  return launch_agg(items, n_items, heavy, n_heavy, col, wp, C, ep, partials, as_stream(stream));
}

size_t gnpde_squareplus_backward_workspace_bytes(int64_t B) {
  return sizeof(double) * (size_t)kSpMaxBlocks * (size_t)(B > 0 ? B : 1);
}

int gnpde_squareplus_backward_f32(const int32_t* rowptr, const int32_t* perm, int64_t R, int64_t nnz, int64_t B,
                                  int heads, const float* att, const float* g_att, const float* rl,
                                  const int64_t* amax, float* gs, void* workspace, size_t workspace_bytes,
                                  void* stream) {
  GNPDE_REQUIRE(R >= 1 && nnz >= 0 && heads >= 1 && heads <= 16 && B >= 1 && B <= 65535 && nnz % B == 0,
                GNPDE_EINVAL, "squareplus_backward: bad sizes");
  if (nnz == 0) return GNPDE_OK;
  GNPDE_REQUIRE(rowptr && perm && att && g_att && rl && amax && gs && workspace, GNPDE_EINVAL,
                "squareplus_backward: NULL pointer");
  GNPDE_REQUIRE(workspace_bytes >= gnpde_squareplus_backward_workspace_bytes(B), GNPDE_EINVAL,
                "squareplus_backward: workspace too small");
  hipStream_t s = as_stream(stream);
  const int64_t blocks = ceil_div(R, (int64_t)kWavesPerBlock);
  squareplus_backward_kernel<<<(int)(blocks < 65536 ? blocks : 65536), kBlock, 0, s>>>(rowptr, perm, R, heads, att,
                                                                                         g_att, rl, gs);
  GNPDE_LAUNCH_CHECK();
  const int64_t per_batch = nnz / B * heads;
  const unsigned nb = sp_grid(per_batch, kSpMaxBlocks);
  double* part = static_cast<double*>(workspace);
  squareplus_gsum_kernel<<<dim3(nb, (unsigned)B), kBlock, 0, s>>>(gs, per_batch, part);
  GNPDE_LAUNCH_CHECK();
  squareplus_gmax_kernel<<<(unsigned)B, kWave, 0, s>>>(part, (int)nb, reinterpret_cast<const long long*>(amax), gs);
  GNPDE_LAUNCH_CHECK();
  return GNPDE_OK;
}

}  // extern "C"
