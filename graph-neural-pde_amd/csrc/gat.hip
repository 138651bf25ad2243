// gat.hip — the GAT attention function's own entry points (function_GAT_attention.py):
// the fused-weight K1 (gnpde_attn_gat_rhs_f32: GatSoftmaxWeights, aggregate.hpp) and the
// LeakyReLU backward of the edge scores (gnpde_gat_score_backward_f32).  The node-score
// pass (gnpde_gat_scores_f32) is in node_scores.hip beside the kernel it shares; the
// statistics, weights and attention kernels take GAT as score mode GNPDE_SCORE_GAT.
#include "aggregate.hpp"
#include "rhs_host.hpp"

namespace gnpde {

// ge[e,h] = gs[e,h] * (sl[src,h] + sr[dst,h] > 0 ? 1 : slope): torch's LeakyReLU
// derivative (the slope at 0), edge-parallel; rowidx / col / perm: the aggregation CSR
// (row = source, col = destination, perm = COO id), gs and ge in COO order.
__global__ __launch_bounds__(256) void gat_score_backward_kernel(const int* __restrict__ rowidx,
                                                                  const int* __restrict__ col,
                                                                  const int* __restrict__ perm, int64_t nnz, int H,
                                                                  const double* __restrict__ sp, float slope,
                                                                  const float* __restrict__ gs,
                                                                  float* __restrict__ ge) {
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < nnz; p += (int64_t)gridDim.x * blockDim.x) {
    const int r = rowidx[p], c = col[p];
    const int64_t e = perm[p];
    for (int h = 0; h < H; ++h) {
      const double t = sp[(int64_t)r * 2 * H + h] + sp[(int64_t)c * 2 * H + H + h];
      ge[e * H + h] = gs[e * H + h] * (t > 0.0 ? 1.f : slope);
    }
  }
}

template <bool DST>
static int launch_gat_rhs(const int32_t* items, int64_t n_items, int32_t* heavy, int64_t n_heavy, const int32_t* col,
                          const double* sp, const double* m, const float* rl, int heads, float slope, int64_t C,
                          const Epi& ep, float* partials, hipStream_t s) {
  if (heads <= 2) {
    GatSoftmaxWeights<2, DST> wp{sp, m, rl, heads, slope};
    return launch_agg(items, n_items, heavy, n_heavy, col, wp, C, ep, partials, s);
  }
  GatSoftmaxWeights<0, DST> wp{sp, m, rl, heads, slope};
  return launch_agg(items, n_items, heavy, n_heavy, col, wp, C, ep, partials, s);
}

}  // namespace gnpde

using namespace gnpde;

extern "C" {

int gnpde_attn_gat_rhs_f32(const int32_t* items, int64_t n_items, int32_t* heavy, int64_t n_heavy,
                           const int32_t* col, const double* sp, const double* m, const float* rl, int norm_idx,
                           int64_t heads, float slope, int64_t C, const float* x, int64_t ldx, const float* x0,
                           int64_t ldx0, const float* alpha, const float* beta, int flags, float* f, int64_t ldf,
                           float* partials, int64_t n_slots, const gnpde_stage_epilogue_t* stage, void* stream) {
  const Epi ep = make_epi(x, ldx, x0, ldx0, alpha, beta, flags, f, ldf, stage);
  int rc = check_epi(ep, C, n_heavy, partials, n_slots);
  if (rc) return rc;
  GNPDE_REQUIRE(heads >= 1 && heads <= 8, GNPDE_EUNSUPPORTED, "attn_gat_rhs: heads=%lld not in [1,8]",
                (long long)heads);
  GNPDE_REQUIRE(norm_idx == 0 || norm_idx == 1, GNPDE_EINVAL, "attn_gat_rhs: norm_idx must be 0 or 1");
  GNPDE_REQUIRE(n_items >= 0 && n_items < INT32_MAX && n_heavy >= 0, GNPDE_EINVAL, "attn_gat_rhs: bad item counts");
  GNPDE_REQUIRE(n_items == 0 || (items && col && sp && m && rl), GNPDE_EINVAL,
                "attn_gat_rhs: NULL plan/col/node scores/statistics");
  if (norm_idx == 1)
    return launch_gat_rhs<true>(items, n_items, heavy, n_heavy, col, sp, m, rl, (int)heads, slope, C, ep, partials,
                                as_stream(stream));
  return launch_gat_rhs<false>(items, n_items, heavy, n_heavy, col, sp, m, rl, (int)heads, slope, C, ep, partials,
                               as_stream(stream));
}

int gnpde_gat_score_backward_f32(const int32_t* rowidx, const int32_t* col, const int32_t* perm, int64_t nnz,
                                 int64_t heads, const double* sp, float slope, const float* gs, float* ge,
                                 void* stream) {
  GNPDE_REQUIRE(heads >= 1 && heads <= 8 && nnz >= 0, GNPDE_EINVAL, "gat_score_backward: bad sizes");
  if (nnz == 0) return GNPDE_OK;
  GNPDE_REQUIRE(rowidx && col && perm && sp && gs && ge, GNPDE_EINVAL, "gat_score_backward: NULL pointer");
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(nnz, kBlock), 16384));
  gat_score_backward_kernel<<<grid, kBlock, 0, as_stream(stream)>>>(rowidx, col, perm, nnz, (int)heads, sp, slope, gs,
                                                                     ge);
  GNPDE_LAUNCH_CHECK();
  return GNPDE_OK;
}

}  // extern "C"
