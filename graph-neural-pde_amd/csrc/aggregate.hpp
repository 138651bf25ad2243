// aggregate.hpp — the gather-aggregate engine shared by the Laplacian RHS (K1)
// and the attention RHS (K3): one wavefront per work item (a whole CSR row or a
// chunk of a hub row), rows of x gathered with 16-byte loads, the RHS epilogue
// fused.  Hub rows are split into chunk items whose partial sums are combined
// inside the same launch by the chunk that finishes last (arrival ticket on the
// hub's plan entry; fixed summation order, so deterministic; no float atomics).
#pragma once
#include <algorithm>
#include <type_traits>

#include "common.hpp"
#include "scores.hpp"

namespace gnpde {

// ------------------------------------------------------------------ weight policies
// A policy splits the weight of CSR position p (row, destination c) into
// load() — the raw operands, issued with the column index — and finish() —
// the arithmetic, run once the first gathers of x are in flight, so the
// weight's memory latency overlaps the row gathers instead of preceding them.
//
// Plain per-edge weights (Laplacian RHS, function_laplacian_diffusion.py:54-57).
struct PlainWeights {
  const float* __restrict__ w;
  struct Raw {
    float w;
  };
  __device__ __forceinline__ Raw load(int /*row*/, int p, int /*c*/) const { return Raw{w[p]}; }
  __device__ __forceinline__ float finish(int /*row*/, const Raw& r) const { return r.w; }
};

// Reference-mode (fork scaled_dot) attention under destination-grouped softmax
// (attention_norm_idx 1), head-mean taken on the fly: the score of an edge is
// the node score cs[row, h] of its source (the aggregating row), the group
// statistics m, rl belong to its destination c.  Same arithmetic, in the same
// order, as attn_weights_kernel (rhs.hip), so fusing it into K1 changes no
// bit; it saves the separate weights pass and its [nnz] round trip.
// MAXH > 0: heads <= MAXH, the per-edge statistics are loaded up front;
// MAXH == 0: any heads <= 16, loaded in finish().  EXACT (heads == MAXH == 2,
// m 16-byte and rl 8-byte aligned): one 16-B load of m[c,:] and one 8-B load
// of rl[c,:] per edge instead of four scalar gathers.
// REC (with EXACT): m and rl come from the packed statistics records of the
// destinations (rec, stats_record_floats(2) = 4 floats: m[0..1], rl[0..1]):
// one 16-byte load per edge, a quarter of a cache line, instead of two lines of
// the separate arrays; the same values (the stored max is fp32-exact in both
// forms) and the same finish(), so the same bits.
template <int MAXH, bool EXACT = false, bool REC = false>
struct RefDstSoftmaxWeights {
  const double* __restrict__ cs;
  const double* __restrict__ m;
  const float* __restrict__ rl;
  int H;
  const float* __restrict__ rec;
  struct Raw {
    double mm[MAXH > 0 ? MAXH : 1];
    float rr[MAXH > 0 ? MAXH : 1];
    int c;
  };
  __device__ __forceinline__ Raw load(int /*row*/, int /*p*/, int c) const {
    Raw r;
    r.c = c;
    if constexpr (EXACT && REC) {
      static_assert(MAXH == 2 && stats_record_floats(2) == 4, "two-head records are 16 bytes");
      const float4 v = *reinterpret_cast<const float4*>(rec + (int64_t)c * 4);
      r.mm[0] = (double)v.x;
      r.mm[1] = (double)v.y;
      r.rr[0] = v.z;
      r.rr[1] = v.w;
    } else if constexpr (EXACT) {
      static_assert(MAXH == 2, "EXACT statistics loads are written for two heads");
      const double2 mv = *reinterpret_cast<const double2*>(m + (int64_t)c * 2);
      const float2 rv = *reinterpret_cast<const float2*>(rl + (int64_t)c * 2);
      r.mm[0] = mv.x;
      r.mm[1] = mv.y;
      r.rr[0] = rv.x;
      r.rr[1] = rv.y;
    } else if constexpr (MAXH > 0) {
#pragma unroll
      for (int h = 0; h < MAXH; ++h) {
        const int hh = h < H ? h : 0;
        r.mm[h] = m[(int64_t)c * H + hh];
        r.rr[h] = rl[(int64_t)c * H + hh];
      }
    }
    return r;
  }
  __device__ __forceinline__ float finish(int row, const Raw& r) const {
    float acc = 0.f;
    if constexpr (MAXH > 0) {
#pragma unroll
      for (int h = 0; h < MAXH; ++h)
        if (h < H) acc += expf((float)(cs[(int64_t)row * H + h] - r.mm[h])) * r.rr[h];
    } else {
      for (int h = 0; h < H; ++h)
        acc += expf((float)(cs[(int64_t)row * H + h] - m[(int64_t)r.c * H + h])) * rl[(int64_t)r.c * H + h];
    }
    return acc / (float)H;
  }
};

// GAT attention (function_GAT_attention.py:131-135), head mean taken on the fly:
// the score of edge (row, c) is LeakyReLU(sl[row,h] + sr[c,h]) from the node-score
// pairs sp [R, 2H] = [sl | sr] (gnpde_gat_scores_f32); the softmax group g is the
// row (DST false, attention_norm_idx 0) or the destination c (DST true, norm_idx 1).
// load() issues the sr[c,:] gather and, with DST, the destination's statistics;
// for source groups the row's own sl, m, rl are per-item values read in finish()
// (one address per row slot: served by the cache).  Same arithmetic, in the same
// order, as attn_weights_kernel in mode GAT (ScoreArgs::score -> gat_leaky), so the
// fused launch equals the weights pass + the plain K1 bit for bit.
// MAXH > 0: heads <= MAXH, operands loaded up front; MAXH == 0: any heads <= 8,
// loaded in finish().
template <int MAXH, bool DST>
struct GatSoftmaxWeights {
  const double* __restrict__ sp;
  const double* __restrict__ m;
  const float* __restrict__ rl;
  int H;
  float slope;
  struct Raw {
    double sr[MAXH > 0 ? MAXH : 1];
    double mm[(MAXH > 0 && DST) ? MAXH : 1];
    float rr[(MAXH > 0 && DST) ? MAXH : 1];
    int c;
  };
  __device__ __forceinline__ Raw load(int /*row*/, int /*p*/, int c) const {
    Raw r;
    r.c = c;
    if constexpr (MAXH > 0) {
#pragma unroll
      for (int h = 0; h < MAXH; ++h) {
        const int hh = h < H ? h : 0;
        r.sr[h] = sp[(int64_t)c * 2 * H + H + hh];
        if constexpr (DST) {
          r.mm[h] = m[(int64_t)c * H + hh];
          r.rr[h] = rl[(int64_t)c * H + hh];
        }
      }
    }
    return r;
  }
  __device__ __forceinline__ float finish(int row, const Raw& r) const {
    float acc = 0.f;
    const int64_t g = DST ? r.c : row;
    if constexpr (MAXH > 0) {
#pragma unroll
      for (int h = 0; h < MAXH; ++h)
        if (h < H) {
          const double s = gat_leaky(sp[(int64_t)row * 2 * H + h], r.sr[h], slope);
          const double mg = DST ? r.mm[h] : m[g * H + h];
          const float rg = DST ? r.rr[h] : rl[g * H + h];
          acc += expf((float)(s - mg)) * rg;
        }
    } else {
      for (int h = 0; h < H; ++h) {
        const double s = gat_leaky(sp[(int64_t)row * 2 * H + h], sp[(int64_t)r.c * 2 * H + H + h], slope);
        acc += expf((float)(s - m[g * H + h])) * rl[g * H + h];
      }
    }
    return acc / (float)H;
  }
};

// Reference-mode (fork scaled_dot) attention under destination-grouped SQUAREPLUS
// normalisation (square_plus, src/utils.py:129-140), head mean taken on the fly.  The
// squareplus value of an edge is a per-node quantity of its source, p[row, h] =
// squareplus_p(cs[row, h] - M_b) (gnpde_squareplus_stats_f32 forms the [R, H] array once per
// RHS), and the group statistics rl[c, h] = 1 / (sum p + 1e-16) belong to its destination c:
//   w = (1/H) sum_h p[row, h] * rl[c, h]
// — no transcendental per edge.  load() issues the rl[c, :] gather with the column index;
// p[row, :] is one address per row slot (loop-invariant: read once per item).  Same
// arithmetic, in the same order, as squareplus_edge_kernel (squareplus.hip), so the fused
// launch equals gnpde_squareplus_weights_f32 + gnpde_spmm_rhs_f32 bit for bit.
// MAXH > 0: heads <= MAXH, rl loaded up front; MAXH == 0: any heads <= 16, loaded in finish().
template <int MAXH>
struct RefDstSquareplusWeights {
  const float* __restrict__ pn;
  const float* __restrict__ rl;
  int H;
  struct Raw {
    float rr[MAXH > 0 ? MAXH : 1];
    int c;
  };
  __device__ __forceinline__ Raw load(int /*row*/, int /*p*/, int c) const {
    Raw r;
    r.c = c;
    if constexpr (MAXH > 0) {
#pragma unroll
      for (int h = 0; h < MAXH; ++h) r.rr[h] = rl[(int64_t)c * H + (h < H ? h : 0)];
    }
    return r;
  }
  __device__ __forceinline__ float finish(int row, const Raw& r) const {
    float acc = 0.f;
    if constexpr (MAXH > 0) {
#pragma unroll
      for (int h = 0; h < MAXH; ++h)
        if (h < H) acc = squareplus_mean_step(pn[(int64_t)row * H + h], r.rr[h], acc);
    } else {
      for (int h = 0; h < H; ++h) acc = squareplus_mean_step(pn[(int64_t)row * H + h], rl[(int64_t)r.c * H + h], acc);
    }
    return acc / (float)H;
  }
};

// Policies that take the narrow-row lane geometries of launch_agg_vec (several rows per
// wavefront below 17 lanes): the plain weights, and the GAT policy, which promises the
// bits of the weights pass + the plain K1 at every width, so it sums in the same order.
template <class WP>
struct takes_narrow_rows : std::is_same<WP, PlainWeights> {};
template <int MAXH, bool DST>
struct takes_narrow_rows<GatSoftmaxWeights<MAXH, DST>> : std::true_type {};
template <int MAXH>
struct takes_narrow_rows<RefDstSquareplusWeights<MAXH>> : std::true_type {};  // the same promise

template <class WP>
__host__ __device__ inline PlainWeights as_plain(const WP& wp) {
  if constexpr (std::is_same<WP, PlainWeights>::value) return wp;
  else return PlainWeights{nullptr};  // never launched (launch_agg_cfg)
}

// ------------------------------------------------------------------ hub rows
// Lane groups of the hub combine are powers of two (an xor tree joins them):
// a geometry with GL = 21 lanes per row (three bf16 rows of 168 columns per
// wavefront) combines its hub rows with 32-lane groups.
constexpr int pow2_ceil(int v) { return v <= 1 ? 1 : 2 * pow2_ceil((v + 1) / 2); }

// Sum the nch chunk partials of hub row `row` (slots first .. first+nch-1), then
// run the epilogue.  GL lanes cover the columns; the 64/GL lane groups take
// chunks g, g+G, ... and are combined by a fixed xor tree (deterministic).
template <int VEC, int GL, int STG, class T>
__device__ __forceinline__ void hub_combine(int row, int first, int nch, int C, const Epi& ep,
                                            const float* __restrict__ partials) {
  constexpr int G = kWave / GL;
  const int lane = threadIdx.x & 63;
  const int g = lane / GL, gl = lane % GL;
  const float a = (ep.flags & GNPDE_EPI_RHS) ? epi_alpha(ep) : 1.f;
  const float b = (ep.flags & GNPDE_ADD_SOURCE) ? *ep.beta : 0.f;
  double dpart[2] = {0.0, 0.0};
  for (int c0 = 0; c0 < C; c0 += GL * VEC) {
    const int cc = c0 + gl * VEC;
    const bool live = cc < C;
    float s[VEC];
#pragma unroll
    for (int t = 0; t < VEC; ++t) s[t] = 0.f;
#pragma unroll 4
    for (int c = g; c < nch; c += G) {
      float v[VEC];
      if (live) {
        load_vec<VEC>(partials + (int64_t)(first + c) * C + cc, v);
      } else {
#pragma unroll
        for (int t = 0; t < VEC; ++t) v[t] = 0.f;
      }
#pragma unroll
      for (int t = 0; t < VEC; ++t) s[t] += v[t];
    }
#pragma unroll
    for (int o = GL; o < kWave; o <<= 1)
#pragma unroll
      for (int t = 0; t < VEC; ++t) s[t] += __shfl_xor(s[t], o);
    if (g == 0 && live) epilogue_store<VEC, STG, T>(ep, row, cc, s, a, b, dpart);
  }
  epi_rowsums<GL, STG, T>(ep, row, dpart, 0, lane == 0);  // wave-uniform
}

// The sum of the nch chunk partials of a hub row (slots first .. first+nch-1),
// computed by all 64 lanes: lane groups of GLp = pow2_ceil(GL) lanes take chunks
// g, g+G, ... (4 loads in flight), joined by a fixed xor tree — the order of
// hub_combine, so the same bits.  Every lane ends with the sums of the columns
// (ch*GLp + lane % GLp)*VEC.
template <int VEC, int GL, int NCH>
__device__ __forceinline__ void hub_sum(int first, int nch, int C, const float* __restrict__ partials,
                                        float (&hs)[NCH][VEC]) {
  constexpr int GLp = pow2_ceil(GL);
  constexpr int G = kWave / GLp;
  static_assert(NCH == 1 || GLp == GL, "several column passes need power-of-two row lanes");
  const int lane = threadIdx.x & 63;
  const int g = lane / GLp, gl = lane % GLp;
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    const int cc = (ch * GLp + gl) * VEC;
    const bool live = cc < C;
#pragma unroll
    for (int t = 0; t < VEC; ++t) hs[ch][t] = 0.f;
#pragma unroll 4
    for (int c = g; c < nch; c += G) {
      float v[VEC];
      if (live) {
        load_vec<VEC>(partials + (int64_t)(first + c) * C + cc, v);
      } else {
#pragma unroll
        for (int t = 0; t < VEC; ++t) v[t] = 0.f;
      }
#pragma unroll
      for (int t = 0; t < VEC; ++t) hs[ch][t] += v[t];
    }
#pragma unroll
    for (int o = GLp; o < kWave; o <<= 1)
#pragma unroll
      for (int t = 0; t < VEC; ++t) hs[ch][t] += __shfl_xor(hs[ch][t], o);
  }
}

// Memory order of the arrival ticket.  The partials are stored write-through and
// drained (s_waitcnt vmcnt(0)) before the ticket, which is what an agent-scope
// release orders at the ISA level.  The ticket is not a formal C++ release as
// well: that adds buffer_wbl2 sc1, a write-back of every dirty line of the XCD's
// L2 before each chunk's ticket.
constexpr int kHubTicketOrder = __ATOMIC_RELAXED;

// Chunk waves whose write-through partial stores are issued: drain them; each
// row slot holding a hub chunk takes an arrival ticket on its hub's plan entry
// (heavy[h].w, an agent-scope atomic; hubs found by a binary search of the
// ascending first slots); every slot whose chunk arrived last then has its hub
// row summed by the whole wavefront (hub_sum, after an acquire; the ticket is
// reset to 0 for the next launch on this plan), and the slot's owner lanes take
// the row (erow) and its sums (acc) for the kernel's one epilogue.  Called by
// all 64 lanes; `chunk`, `slot` are per slot.  Returns whether this lane now
// owns a hub row.
template <int VEC, int GL, int SL, int RPW, int NCH>
__device__ __forceinline__ bool hub_claim(int4* heavy, int n_heavy, bool chunk, int slot, int C,
                                          const float* partials, int rs, int g, int gl, int& erow,
                                          float (&acc)[NCH][VEC]) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const int lane = threadIdx.x & 63;
  int lo = 0, won = 0;
  if (chunk) {
    int hi = n_heavy - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (heavy[mid].y <= slot)
        lo = mid;
      else
        hi = mid - 1;
    }
    if (lane % SL == 0) {
      const int t = __hip_atomic_fetch_add(&heavy[lo].w, 1, kHubTicketOrder, __HIP_MEMORY_SCOPE_AGENT);
      won = t == heavy[lo].z - 1;
    }
  }
  bool mine = false;
  for (int s = 0; s < RPW; ++s) {
    if (__shfl(won, s * SL)) {  // wave-uniform
      const int h = __shfl(lo, s * SL);
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      const int4 hv = heavy[h];
      float hs[NCH][VEC];
      hub_sum<VEC, GL, NCH>(uniform(hv.y), uniform(hv.z), C, partials, hs);
      // the slot's lane gl takes the sums of its columns from lane gl (group 0 holds every column)
      const bool take = rs == s && g == 0;
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
        for (int t = 0; t < VEC; ++t) {
          const float v = (GL == kWave) ? hs[ch][t] : __shfl(hs[ch][t], gl);
          acc[ch][t] = take ? v : acc[ch][t];
        }
      if (take) {
        erow = uniform(hv.x);
        mine = true;
      }
      if (lane == 0) __hip_atomic_store(&heavy[h].w, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  return mine;
}

// The hub combine of the flash kernels (flash.hip; agg_kernel uses hub_claim): each row slot of the wavefront that holds a
// hub chunk takes its own ticket (its first lane); every slot whose chunk
// arrived last is then combined by the WHOLE wavefront, one slot after the
// other (hub_combine over 64 lanes).  Called by all 64 lanes; `chunk` is per slot.
template <int VEC, int GL, int SL, int RPW, int STG, class T>
__device__ __forceinline__ void hub_arrive_slots(int4* heavy, int n_heavy, bool chunk, int slot, int C,
                                                 const Epi& ep, const float* partials) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const int lane = threadIdx.x & 63;
  int lo = 0, won = 0;
  if (chunk) {
    int hi = n_heavy - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (heavy[mid].y <= slot)
        lo = mid;
      else
        hi = mid - 1;
    }
    if (lane % SL == 0) {
      const int t = __hip_atomic_fetch_add(&heavy[lo].w, 1, kHubTicketOrder, __HIP_MEMORY_SCOPE_AGENT);
      won = t == heavy[lo].z - 1;
    }
  }
#pragma unroll
  for (int s = 0; s < RPW; ++s) {
    if (__shfl(won, s * SL)) {  // wave-uniform
      const int h = __shfl(lo, s * SL);
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      const int4 hv = heavy[h];
      hub_combine<VEC, pow2_ceil(GL), STG, T>(uniform(hv.x), uniform(hv.y), uniform(hv.z), C, ep, partials);
      if (lane == 0) __hip_atomic_store(&heavy[h].w, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// The folded dense output's crossing flag and coefficients (dense_coefs), formed ahead of
// the launch whose stage asks for them (ABI 8: dense_tab without dense_out) for the step's
// last launch.  A launch of its own: the same branch at the top of the aggregation kernel
// cost every instantiation (BLEND's fp32 rk4 step 0.556 -> 0.583 ms).
static __global__ __launch_bounds__(64) void dense_coef_kernel(gnpde_stage_epilogue_t st) {
  if (threadIdx.x == 0) dense_coefs(st, st.dense_tab);
}

// ------------------------------------------------------------------ frozen rows
// A row whose only edge is its own self loop of weight exactly 1.0f, and that no other row
// gathers, has f = a*(1*x - x) = 0: the first three rk4 stage inputs of such a row equal the
// row bit for bit, nothing reads them, and the step changes the row only by the rounding of
// its last combination, which depends on nothing but the row.  A solve
// that reads its state only at the end then leaves these rows out of every launch but its
// last, which streams them once: kFrozenPass row slices in flight per lane, each taken
// through `steps` whole rk4 steps in registers — the aggregation of its one edge
// (fmaf(1, v, 0)), f = a*(ax - x), and the SAME stage_combine / epi_finish as every other row
// with the own row, the base and every operand set to the slice: the operation sequence, and
// so the bits, of `steps` full steps (the last step's coefficients serve all: f is 0, or NaN
// for a non-finite entry, whatever the step size).  A lane reads its slice of fz_home before
// it stores (to the same row, or through out_rows).
constexpr int kStgFrozen = 6;
constexpr int kFrozenPass = 4;  // row slices in flight per lane
template <int RPW>
constexpr int frozen_rows_per_block() {
  return kWavesPerBlock * RPW * kFrozenPass;
}

template <int VEC, int GL, int RPW>
__device__ __forceinline__ void frozen_tail(const Epi& ep, int C, const float* __restrict__ home, int r0, int r1,
                                            int steps, int tb, int wave, int rs, int gl) {
  const int cc = gl * VEC;
  const int rb = r0 + tb * frozen_rows_per_block<RPW>() + wave * RPW + rs;
  Packed<VEC, float> v[kFrozenPass];
#pragma unroll
  for (int i = 0; i < kFrozenPass; ++i) {
    const int row = rb + i * kWavesPerBlock * RPW;
    if (row < r1 && rs < RPW && cc < C) {
      load_packed<VEC>(home + (int64_t)row * ep.ldx + cc, v[i]);
    } else {
#pragma unroll
      for (int t = 0; t < VEC; ++t) v[i].d[t] = 0u;
    }
  }
  const float a = (ep.flags & GNPDE_EPI_RHS) ? epi_alpha(ep) : 1.f;
  // the steps before the last: epi_finish's arithmetic (EPI_RHS, no source, f_lin 0: launch_agg_frozen)
  // without its stores, the slices of a lane side by side
  const float sc = out_scale(ep.st, 0, stage_scale(ep.st));
#pragma unroll 1
  for (int k = 1; k < steps; ++k) {
#pragma unroll
    for (int i = 0; i < kFrozenPass; ++i) {
      const Packed<VEC, float> x = v[i];
      float o[VEC], r[VEC];
#pragma unroll
      for (int t = 0; t < VEC; ++t) o[t] = a * (fmaf(1.0f, unpack(x, t), 0.f) - unpack(x, t));
      auto kval = [&](int /*j*/, int t) -> float { return unpack(x, t); };
      stage_combine<VEC, kStagePre, float>(ep, ep.st.o[0], 0, o, x, &x, kval, sc, r);
      pack_into<VEC, float>(r, v[i]);
    }
  }
#pragma unroll
  for (int i = 0; i < kFrozenPass; ++i) {
    const int row = rb + i * kWavesPerBlock * RPW;
    if (row < r1 && rs < RPW && cc < C) {
      EpiPre<VEC, float, 1> p;
      p.xr = v[i];
      p.x0r = v[i];
#pragma unroll
      for (int j = 0; j < stage_bpre<1>(); ++j) p.base[j] = v[i];
#pragma unroll
      for (int j = 0; j < stage_kpre<1>(); ++j) p.kv[j] = v[i];
      float ax[VEC];
#pragma unroll
      for (int t = 0; t < VEC; ++t) ax[t] = fmaf(1.0f, unpack(v[i], t), 0.f);
      epi_finish<VEC, 1, float>(ep, row, cc, ax, a, 0.f, p, nullptr);
    }
  }
}

// ------------------------------------------------------------------ column stripes
// The headline geometry (plain weights, fp32 rows of 65-128 columns in 16-byte slices, stage
// kinds 0 and 1) on a graph whose gathered rows do not fit one XCD's L2: the
// eight L2s are not shared and every XCD runs a random eighth of the items, so every XCD pulls
// nearly every gathered row once per launch.  With S column stripes a workgroup aggregates
// 128 / S columns of ALL its rows — 32 / S lanes per row slot, 2 S slots per wavefront — and
// workgroup b takes stripe (b % 8) * S / 8: the workgroups of 8 / S XCDs (b % 8 says which
// workgroups share an XCD: an observation, used for speed only) fetch a row's slice of that
// stripe, and no other XCD does.  Every (stripe, item block) pair is one workgroup by index
// arithmetic alone; no workgroup waits on another.
//
// Same bits as the unstriped kernel: per column the FMAs run in the row's CSR order (one edge
// group per slot, as there), the epilogue is epi_prefetch / epi_finish at the lane's columns,
// and a hub row is summed as the 32-lane geometry sums it (hub_sum<VEC, 32>: even chunks in
// order, odd chunks in order, the two added) — by the wavefront whose chunk slice arrives last
// of the hub's nch chunks x the stripes inside C (one ticket per hub, counted to their
// product), over the whole row.
//
// Which mapping a launch takes: k1_stripes_for (rhs.hip; GNPDE_K1_STRIPES).
int k1_stripes_for(int64_t n_items, int64_t C, int stage_kind, int flags);
void k1_striped_launched();

// A kernel of its own, not a launch-uniform branch of agg_kernel: the branch took the fused-stage
// instantiation from 60 to 69 VGPRs (8 -> 7 waves per SIMD) on the unstriped path as well.
//
// The launches of agg_kernel that agg_stripe_kernel can stand in for.
template <int VEC, int GL, int NCH, int U, int RPW, int STG, class WP, class T>
constexpr bool striped_geometry() {
  return std::is_same<WP, PlainWeights>::value && sizeof(T) == 4 && VEC == 4 && GL == 32 && RPW == 2 && NCH == 1 &&
         U == 4 && (STG == 0 || STG == 1);
}

template <int S>
constexpr int stripe_rpw() {
  return 2 * S;  // row slots per wavefront: 64 lanes / (32 / S lanes per slot)
}
// Workgroups of a striped launch: rounds of 8, each round 8 / S item blocks x S stripes.
template <int S>
inline unsigned stripe_grid(int64_t n_items) {
  const int64_t nib = ceil_div(n_items, (int64_t)kWavesPerBlock * stripe_rpw<S>());
  return (unsigned)(ceil_div(nib, (int64_t)(kNumXcd / S)) * kNumXcd);
}

template <int S, int STG>
__global__ __launch_bounds__(256) void agg_stripe_kernel(const int4* __restrict__ items, int n_items, int4* heavy,
                                                          int n_heavy, const int* __restrict__ col, PlainWeights wp,
                                                          int C, Epi ep, float* __restrict__ partials) {
  static_assert((S == 2 || S == 4) && (STG == 0 || STG == 1), "stripes of the forward epilogues");
  static_assert(!stage_rowsum<STG, float>(), "no per-row term to reduce across stripes");
  // U = 8 gathers per batch and the batches of a chunk unrolled (the compiler issues the next
  // batch's gathers ahead of the wait for this one's): 90-92 VGPRs, 5 waves per SIMD, and the
  // fastest of the forms measured (U = 4 in a rolled loop, 66 VGPRs and 7 waves,
  // ran S = 4 10 % behind the unstriped kernel; column ids of 32 edges per round trip, KR = 32 / SL,
  // came out behind KR = 1 at S = 2).
  constexpr int VEC = 4, U = 8;
  constexpr int SL = 32 / S;           // lanes per row slot: one edge group (G = 1)
  constexpr int KR = 1;                // registers of column ids per lane and chunk
  constexpr int RPW = stripe_rpw<S>();  // row slots per wavefront
  constexpr int XS = kNumXcd / S;      // item blocks per round of 8 workgroups
  const int b = blockIdx.x;
  const int stripe = (b % kNumXcd) / XS;  // = (b % 8) * S / 8
  const int ib = (b / kNumXcd) * XS + b % XS;
  const int c0 = stripe * SL * VEC;
  if (c0 >= C) return;  // workgroup-uniform: a stripe wholly outside C (S = 4, C <= 96)
  const int lane = threadIdx.x & 63;
  const int rs = lane / SL, gl = lane % SL;
  const int wid = uniform(ib * kWavesPerBlock + (threadIdx.x >> 6));
  if (wid * RPW >= n_items) return;  // wave-uniform
  const int item = wid * RPW + rs;
  const bool live = item < n_items;
  const int4 it = live ? items[item] : make_int4(0, 0, 0, -1);
  const int row = it.x, beg = it.y, end = it.z, slot = it.w;
  const int cc = c0 + gl * VEC;
  const bool inc = cc < C;  // a last stripe partly inside C
  const bool owner = live && slot < 0 && inc;

  EpiPre<VEC, float, STG> pre;
  if (owner) epi_prefetch<VEC, STG, float>(ep, row, cc, pre);  // ahead of the aggregation
  float acc[VEC];
#pragma unroll
  for (int t = 0; t < VEC; ++t) acc[t] = 0.f;
  const float* __restrict__ xb = ep.x + cc;
  // A slot takes the column ids and weights of CH = KR * SL edges in one round trip (KR
  // registers per lane), then gathers them U at a time, in CSR order.
  constexpr int CH = KR * SL;
  for (int e0 = beg; e0 < end; e0 += CH) {
    const int n = min(CH, end - e0);
    int mc[KR];
    float mw[KR];
#pragma unroll
    for (int k = 0; k < KR; ++k) {
      const int e = k * SL + gl;
      mc[k] = 0;
      mw[k] = 0.f;
      if (e < n) {
        mc[k] = col[e0 + e];
        mw[k] = wp.w[e0 + e];
      }
    }
#pragma unroll
    for (int k = 0; k < KR; ++k) {
      const int nk = min(SL, n - k * SL);  // the slot's edges in register k (the lanes of a slot agree)
#pragma unroll
      for (int j = 0; j < SL; j += U) {
        if (j >= nk) break;
        Packed<VEC, float> v[U];
        float ww[U];
        int srcl[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int jj = j + u;
          const int src = rs * SL + (jj < nk ? jj : 0);
          srcl[u] = src;
          const int c = __shfl(mc[k], src);
          if (jj < nk && inc) {
            load_packed<VEC>(xb + (int64_t)c * ep.ldx, v[u]);
          } else {
#pragma unroll
            for (int t = 0; t < VEC; ++t) v[u].d[t] = 0u;
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const float wsl = __shfl(mw[k], srcl[u]);
          ww[u] = j + u < nk ? wsl : 0.f;
        }
        // the edges of a row in CSR order (an edge that is not there adds 0 * 0: acc is never -0)
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int t = 0; t < VEC; ++t) acc[t] = fmaf(ww[u], unpack(v[u], t), acc[t]);
      }
    }
  }

  const bool chunk = live && slot >= 0;
  const bool anyc = n_heavy > 0 && __ballot(chunk) != 0;  // wave-uniform
  if (anyc && chunk) {  // this stripe's slice of the chunk's partial, write-through
    const __amdgpu_buffer_rsrc_t rp = buf_rsrc(partials);
    buf_store_wt<VEC>(rp, inc ? (uint32_t)(((int64_t)slot * C + cc) * 4) : kBufNone, acc);
  }
  const float a = (ep.flags & GNPDE_EPI_RHS) ? epi_alpha(ep) : 1.f;
  const float bt = (ep.flags & GNPDE_ADD_SOURCE) ? *ep.beta : 0.f;
  // The whole rows first: their operands and sums are dead before a hub's epilogue begins.
  if (owner) epi_finish<VEC, STG, float>(ep, row, cc, acc, a, bt, pre, nullptr);
  if (!anyc) return;

  // Hub chunks (hub_claim's protocol): the partial slices drained, one arrival per chunk slot
  // and stripe on the hub's ticket; the arrival that completes nch x (stripes inside C) has the
  // whole row summed and finished by this wavefront, 32 lanes over the columns as the unstriped
  // geometry's hub_sum, and resets the ticket for the next launch on this plan.
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const int nstr = (C + SL * VEC - 1) / (SL * VEC);
  int lo = 0, won = 0;
  if (chunk) {
    int hi = n_heavy - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (heavy[mid].y <= slot)
        lo = mid;
      else
        hi = mid - 1;
    }
    if (gl == 0) {
      const int t = __hip_atomic_fetch_add(&heavy[lo].w, 1, kHubTicketOrder, __HIP_MEMORY_SCOPE_AGENT);
      won = t == heavy[lo].z * nstr - 1;
    }
  }
#pragma unroll 1
  for (int s = 0; s < RPW; ++s) {
    if (__shfl(won, s * SL)) {  // wave-uniform
      const int h = __shfl(lo, s * SL);
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      const int4 hv = heavy[h];
      float hs[1][VEC];
      hub_sum<VEC, 32, 1>(uniform(hv.y), uniform(hv.z), C, partials, hs);
      // both 32-lane groups hold the row's sums; the first one stores
      if (lane < 32 && lane * VEC < C) epilogue_store<VEC, STG, float>(ep, uniform(hv.x), lane * VEC, hs[0], a, bt);
      if (lane == 0) __hip_atomic_store(&heavy[h].w, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// ------------------------------------------------------------------ aggregation kernel
// Lane layout: RPW row slots of SL = 64/RPW lanes per wavefront (one plan item
// each); inside a slot lane = g*GL + gl: G = SL/GL edges are gathered side by
// side, each by a group of GL lanes covering the C columns with VEC-wide loads
// (NCH column passes); U edges per group are in flight per iteration.  The
// epilogue operands (x_r, x0_r, stage inputs) are loaded beside the gathers
// when NCH <= 2 (PRE) so their latency overlaps the aggregation: ahead of the
// edge loop, or, in the headline geometry (SCHED below), behind the row's last
// gathers, with the row's loads issued in the order of its dependence chain
// and whole pairs of half batches pipelined.  Hub rows are combined in-launch
// by the chunk that arrives last (hub_claim), and run through the same
// epilogue as whole rows.
//
// STG_ = kStgFrozen (the last launch of an rk4 solve whose graph has frozen rows, DESIGN.md
// §6.23): the epilogue of STG 1, and the workgroups behind those of the items stream the
// frozen rows [fz_r0, fz_r1) — rows whose one edge is their own self loop of weight 1.0f,
// gathered by no other row — from fz_home through fz_steps steps' epilogues (frozen_tail).
template <int VEC, int GL, int NCH, int U, int RPW, int STG_, class WP, class T = float>
__global__ __launch_bounds__(256) void agg_kernel(const int4* __restrict__ items, int n_items, int4* heavy,
                                                   int n_heavy, const int* __restrict__ col, WP wp, int C, Epi ep,
                                                   float* __restrict__ partials, const float* fz_home = nullptr,
                                                   int fz_r0 = 0, int fz_r1 = 0, int fz_steps = 1) {
  constexpr int STG = STG_ == kStgFrozen ? 1 : STG_;
  constexpr int SL = kWave / RPW;
  constexpr int G = SL / GL;
  static_assert((SL & (SL - 1)) == 0 || G == 1, "non-power-of-two row slots hold one edge group");
  constexpr bool PRE = NCH <= 2;
  const int lane = threadIdx.x & 63;
  const int rs = lane / SL, sl = lane % SL;
  const int g = sl / GL, gl = sl % GL;
  if constexpr (STG_ == kStgFrozen) {
    static_assert(NCH == 1 && G == 1 && sizeof(T) == 4, "the frozen tail is written for the headline geometry");
    const int nb = (n_items + kWavesPerBlock * RPW - 1) / (kWavesPerBlock * RPW);  // the items' workgroups
    if ((int)blockIdx.x >= nb) {  // workgroup-uniform
      frozen_tail<VEC, GL, RPW>(ep, C, fz_home, fz_r0, fz_r1, fz_steps, (int)blockIdx.x - nb, threadIdx.x >> 6, rs,
                                gl);
      return;
    }
  }
  const int wid = uniform(xcd_block(ep.xcd_remap) * kWavesPerBlock + (threadIdx.x >> 6));
  const int item = wid * RPW + rs;
  if (wid * RPW >= n_items) return;
  // RPW = 3 (SL = 21): lane 63 is in no slot
  const bool live = item < n_items && rs < RPW;
  const int4 it = live ? items[item] : make_int4(0, 0, 0, -1);
  const int row = it.x, beg = it.y, end = it.z, slot = it.w;
  const bool owner = live && slot < 0 && g == 0;

  EpiPre<VEC, T, STG> pre[PRE ? NCH : 1];
  // The epilogue operands.  SCHED issues them BEHIND the gathers of the row's last batch:
  // the loads return in order, and ahead of the column ids they put one more round trip in
  // front of the gathers.
  auto prefetch = [&]() {
    if constexpr (PRE) {
      if (owner) {
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
          const int cc = (ch * GL + gl) * VEC;
          if (cc < C) epi_prefetch<VEC, STG, T>(ep, row, cc, pre[ch]);
        }
      }
    }
  };

  float acc[NCH][VEC];
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
    for (int t = 0; t < VEC; ++t) acc[ch][t] = 0.f;

  // The load schedule of DESIGN.md §6.13 (SCHED) is taken by the geometry it was measured
  // to win on — plain weights, two 32-lane row slots per wavefront, U = 4: fp32 rows of
  // 65-128 columns, the headline — and by nothing else: the 64-lane geometry lost 6 % to it
  // (BLEND C = 162 fp32 rk4 step 0.560 -> 0.595 ms) and the attention policies lose
  // occupancy.  Every other instantiation keeps the one-batch loop below it.
  constexpr bool SCHED = std::is_same<WP, PlainWeights>::value && sizeof(T) == 4 && VEC == 4 && GL == 32 &&
                         RPW == 2 && NCH == 1 && U == 4;
  if constexpr (SCHED) {
    // The first chunk's column ids go out first: everything else a row needs hangs on them.
    // The chunk loop below is wave-uniform (it runs to the longest row of the wavefront;
    // a slot whose row has ended holds n <= 0 edges), so its branches are scalar.
    const int len = end - beg;
    int lenmax = 0;
#pragma unroll
    for (int s = 0; s < RPW; ++s) lenmax = max(lenmax, __shfl(len, s * SL));
    lenmax = uniform(lenmax);
    int mc = 0;
    if (sl < len) mc = col[beg + sl];

    // Whole PAIRS of half batches (UP = U/2 edges per group, the registers of one batch of U)
    // are pipelined — batch b + 1 is issued before batch b is summed, so gathers stay in
    // flight across batches; the rest of a row (fewer than U edges per group) is one batch.
    // Whole batches of U with a second buffer measured 2.3 % slower (6 waves per SIMD).
    constexpr int UP = U / 2;
    constexpr int B = G * UP;
    using Slice = Packed<VEC, T>;  // gathered row slices in storage form (bf16: half the registers)
    const T* __restrict__ xb = as_t<T>(ep.x);

    // One chunk of SL edges per slot.  LAST: the wavefront's last chunk, behind whose last
    // gathers the epilogue operands go out — not behind the row's first ones, or a long row
    // would hold them in registers through its pipelined batches.
    auto chunk = [&](const int e0, auto last_chunk) {
      constexpr bool LAST = decltype(last_chunk)::value;
      const int n = min(SL, len - e0);              // this slot's edges in the chunk (<= 0: none)
      const int nmax = min(SL, lenmax - e0);        // the longest slot's (wave-uniform)
      const int npair = nmax / (2 * B) * (2 * B);  // its edges in whole pairs of half batches
      int mcn = 0;                                  // the next chunk's column ids, ahead of this chunk's gathers
      if (e0 + SL + sl < len) mcn = col[beg + e0 + SL + sl];
      typename WP::Raw raw{};
      if (sl < n) raw = wp.load(row, beg + e0 + sl, mc);
      float mw = 0.f;
      // the weights of the chunk's edges, finished while its first gathers are in flight
      auto finish = [&]() {
        if (sl < n) mw = wp.finish(row, raw);
      };
      // acc += w * x over a batch, the edges of a row in CSR order (an edge that is not there
      // leaves acc as it is: acc is never -0, so the same bits as adding 0 * 0)
      auto consume = [&](int j, const Slice(&v)[UP][NCH]) {
#pragma unroll
        for (int u = 0; u < UP; ++u) {
          const int jj = j + u * G + g;
          const float ww = __shfl(mw, rs * SL + (jj < n ? jj : 0));
#pragma unroll
          for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
            for (int t = 0; t < VEC; ++t)
              acc[ch][t] = jj < n ? fmaf(ww, unpack(v[u][ch], t), acc[ch][t]) : acc[ch][t];
        }
      };

      if (npair > 0) {
        // In a pipelined batch every lane issues every load — a lane whose slot has no edge
        // left, or that covers no column, re-reads a slice that is there and its sum skips it —
        // so no branch lies between the loads and the wait for a batch is counted (vmcnt(N)
        // with the next batch in flight; behind a branch around a load the compiler waits for
        // vmcnt(0)).
        auto issue = [&](int j, Slice(&v)[UP][NCH]) {
          int c[UP];
#pragma unroll
          for (int u = 0; u < UP; ++u) {
            const int jj = j + u * G + g;
            c[u] = __shfl(mc, rs * SL + (jj < n ? jj : 0));
          }
#pragma unroll
          for (int u = 0; u < UP; ++u) {
            const T* __restrict__ xr = xb + (int64_t)c[u] * ep.ldx;
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) {
              const int cc = (ch * GL + gl) * VEC;
              load_packed<VEC>(xr + (cc < C ? cc : 0), v[u][ch]);
            }
          }
        };
        Slice va[UP][NCH], vb[UP][NCH];
        issue(0, va);
        finish();
        int j = 0;
#pragma unroll 1  // a chunk holds at most SL / B batches: unrolled, all of them would be in flight
        for (; j + 2 * B < npair; j += 2 * B) {  // batch j is in flight in va
          issue(j + B, vb);
          consume(j, va);
          issue(j + 2 * B, va);
          consume(j + B, vb);
        }
        issue(j + B, vb);
        if constexpr (LAST)
          if (npair == nmax) prefetch();
        consume(j, va);
        consume(j + B, vb);
      }
      // The edges behind the whole pairs (at most one batch of U per group; of a short row,
      // all of them): only the gathers that are there are issued, all before the first is summed.  This loader and its FMA block repeat issue() and
      // consume() above on purpose: one buffer variable written by both a branch-free and a
      // predicated loader comes out of the register allocation with copies of single dwords
      // behind the loads, each a vmcnt(0).
      if (npair < nmax) {
        const int j = npair;
        Slice v[U][NCH];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int jj = j + u * G + g;
          const int c = __shfl(mc, rs * SL + (jj < n ? jj : 0));
          const T* __restrict__ xr = xb + (int64_t)c * ep.ldx;
#pragma unroll
          for (int ch = 0; ch < NCH; ++ch) {
            const int cc = (ch * GL + gl) * VEC;
            if (jj < n && cc < C) {
              load_packed<VEC>(xr + cc, v[u][ch]);
            } else {
#pragma unroll
              for (int t = 0; t < Slice::W; ++t) v[u][ch].d[t] = 0u;
            }
          }
        }
        if (j == 0) finish();
        if constexpr (LAST)
          prefetch();
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int jj = j + u * G + g;
          const float ww = __shfl(mw, rs * SL + (jj < n ? jj : 0));
#pragma unroll
          for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
            for (int t = 0; t < VEC; ++t)
              acc[ch][t] = jj < n ? fmaf(ww, unpack(v[u][ch], t), acc[ch][t]) : acc[ch][t];
        }
      }
      mc = mcn;
    };
    int e0 = 0;
    for (; e0 + SL < lenmax; e0 += SL) chunk(e0, std::false_type{});
    if (lenmax > 0)
      chunk(e0, std::true_type{});
    else
      prefetch();  // a wavefront of rows without edges
  } else {
    prefetch();  // ahead of the aggregation
    for (int e0 = beg; e0 < end; e0 += SL) {
      const int n = min(SL, end - e0);
      int mc = 0;
      typename WP::Raw raw{};
      if (sl < n) {
        mc = col[e0 + sl];
        raw = wp.load(row, e0 + sl, mc);
      }
      float mw = 0.f;
      for (int j = 0; j < n; j += G * U) {
        Packed<VEC, T> v[U][NCH];  // gathered row slices in storage form (bf16: half the registers)
        float ww[U];
        int srcl[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int jj = j + u * G + g;
          const int src = rs * SL + (jj < n ? jj : 0);
          srcl[u] = src;
          const int c = __shfl(mc, src);
          const T* __restrict__ xr = as_t<T>(ep.x) + (int64_t)c * ep.ldx;
#pragma unroll
          for (int ch = 0; ch < NCH; ++ch) {
            const int cc = (ch * GL + gl) * VEC;
            if (jj < n && cc < C) {
              load_packed<VEC>(xr + cc, v[u][ch]);
            } else {
#pragma unroll
              for (int t = 0; t < Packed<VEC, T>::W; ++t) v[u][ch].d[t] = 0u;
            }
          }
        }
        // the weights of this batch of edges, finished while its first gathers are in flight
        if (j == 0 && sl < n) mw = wp.finish(row, raw);
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int jj = j + u * G + g;
          const float wsl = __shfl(mw, srcl[u]);
          ww[u] = jj < n ? wsl : 0.f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
            for (int t = 0; t < VEC; ++t) acc[ch][t] = fmaf(ww[u], unpack(v[u][ch], t), acc[ch][t]);
      }
    }
  }
  // combine the G edge groups of each slot
#pragma unroll
  for (int o = GL; o < SL; o <<= 1)
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
      for (int t = 0; t < VEC; ++t) acc[ch][t] += __shfl_xor(acc[ch][t], o);

  // The row whose epilogue this lane runs: its own (an owner lane of a whole
  // row), or a hub row whose chunk arrived last in this wavefront (hub_claim);
  // ONE epilogue below serves both, so the hub combine adds no second copy of
  // the (wide) epilogue to the kernel's register allocation.
  int erow = row;
  bool fin = live && slot < 0 && g == 0;
  bool hub = false;
  if (n_heavy > 0) {  // hub chunks of any slot combined in-launch
    const bool chunk = live && slot >= 0;
    int anyc = 0;
#pragma unroll
    for (int s = 0; s < RPW; ++s) anyc |= __shfl((int)chunk, s * SL);
    if (anyc) {  // wave-uniform
      if (chunk && g == 0) {
        const __amdgpu_buffer_rsrc_t rp = buf_rsrc(partials);
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
          const int cc = (ch * GL + gl) * VEC;
          buf_store_wt<VEC>(rp, cc < C ? (uint32_t)(((int64_t)slot * C + cc) * 4) : kBufNone, acc[ch]);
        }
      }
      hub = hub_claim<VEC, GL, SL, RPW, NCH>(heavy, n_heavy, chunk, slot, C, partials, rs, g, gl, erow, acc);
      fin = fin || hub;
    }
  }  // (n_heavy == 0: no plan holds a chunk without its hub entry)
  if (!fin) return;
  if constexpr (PRE) {  // a hub row's epilogue operands were not prefetched
    if (hub) {
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        const int cc = (ch * GL + gl) * VEC;
        if (cc < C) epi_prefetch<VEC, STG, T>(ep, erow, cc, pre[ch]);
      }
    }
  }
  const float a = (ep.flags & GNPDE_EPI_RHS) ? epi_alpha(ep) : 1.f;
  const float b = (ep.flags & GNPDE_ADD_SOURCE) ? *ep.beta : 0.f;
  double dpart[2] = {0.0, 0.0};
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    const int cc = (ch * GL + gl) * VEC;
    if (cc < C) {
      if constexpr (PRE)
        epi_finish<VEC, STG, T>(ep, erow, cc, acc[ch], a, b, pre[ch], dpart);
      else
        epilogue_store<VEC, STG, T>(ep, erow, cc, acc[ch], a, b, dpart);
    }
  }
  // the row's owner lanes (g == 0: lanes [rs*SL, rs*SL + GL)) are all here
  if constexpr (stage_rowsum<STG, T>()) {
    const double* prev = nullptr;
    if constexpr (PRE && stage_dot<STG>()) prev = &pre[0].dprev;
    epi_rowsums<GL, STG, T>(ep, erow, dpart, rs * SL, gl == 0, prev);
  }
}

template <int VEC, int GL, int NCH, int U, int RPW, class WP, class T = float>
static int launch_agg_cfg(const int4* items, int64_t n_items, int4* heavy, int64_t n_heavy, const int* col,
                          const WP& wp, int C, const Epi& ep, float* partials, hipStream_t s) {
  const unsigned grid = (unsigned)ceil_div(n_items, (int64_t)kWavesPerBlock * RPW);
  const int nh = (int)n_heavy;  // hub rows are combined in the launch (hub_claim)
  // single-output stages without dot terms (every forward gnpde.integrator step) get the
  // leaner instantiation: 56-60 VGPRs, 8 waves per SIMD; the dot terms of the adjoint
  // stages alone cost the general one 40+ VGPRs (fused rk4 K1 92.9 -> 107 us at 4 waves)
  int stg = epi_stage_kind(ep);
  if (ep.has_stage && ep.st.dense_tab && !ep.st.dense_out) {  // the step's dense-output coefficients
    dense_coef_kernel<<<1, kWave, 0, s>>>(ep.st);
    GNPDE_LAUNCH_CHECK();
  }
  if (n_items > 0) {
    // the one-output adjoint stages: fp32 plain weights only (the transposed aggregation)
    if (stg == 3 && !(std::is_same<WP, PlainWeights>::value && sizeof(T) == 4)) stg = 2;
    if (stg == 4) {
      // the adaptive solvers' wide epilogue: plain weights only (the Laplacian RHS and
      // precomputed attention weights); the callers apply it after the other policies
      if constexpr (std::is_same<WP, PlainWeights>::value) {
        if (ep.st.dense_out)  // + the step's folded dense output (ABI 8)
          agg_kernel<VEC, GL, NCH, U, RPW, 5, PlainWeights, T><<<grid, kBlock, 0, s>>>(
              items, (int)n_items, heavy, nh, col, as_plain(wp), C, ep, partials);
        else
          agg_kernel<VEC, GL, NCH, U, RPW, 4, PlainWeights, T><<<grid, kBlock, 0, s>>>(
              items, (int)n_items, heavy, nh, col, as_plain(wp), C, ep, partials);
      } else {
        set_error("rhs: the wide (adaptive-solver) stage epilogue is fused with plain weights only; "
                  "apply it with gnpde_stage_apply_*");
        return GNPDE_EUNSUPPORTED;
      }
    } else if (stg == 3)
      agg_kernel<VEC, GL, NCH, U, RPW, 3, PlainWeights, float><<<grid, kBlock, 0, s>>>(
          items, (int)n_items, heavy, nh, col, as_plain(wp), C, ep, partials);
    else if (stg == 2)
      agg_kernel<VEC, GL, NCH, U, RPW, 2, WP, T><<<grid, kBlock, 0, s>>>(items, (int)n_items, heavy, nh, col, wp, C, ep,
                                                                          partials);
    else {
      // stage kinds 0 and 1; the headline geometry on a large graph in column stripes (agg_stripe_kernel)
      int stripes = 0;
      if constexpr (striped_geometry<VEC, GL, NCH, U, RPW, 0, WP, T>()) stripes = k1_stripes_for(n_items, C, stg, ep.flags);
      if (stripes) {
        if constexpr (striped_geometry<VEC, GL, NCH, U, RPW, 0, WP, T>()) {
#define GNPDE_STRIPED(S, STG)                                                                                       \
  agg_stripe_kernel<S, STG><<<stripe_grid<S>(n_items), kBlock, 0, s>>>(items, (int)n_items, heavy, nh, col, wp, C, ep, \
                                                                        partials)
          if (stripes == 4) {
            if (stg == 1) GNPDE_STRIPED(4, 1);
            else GNPDE_STRIPED(4, 0);
          } else {
            if (stg == 1) GNPDE_STRIPED(2, 1);
            else GNPDE_STRIPED(2, 0);
          }
#undef GNPDE_STRIPED
          k1_striped_launched();
        }
      } else if (stg == 1)
        agg_kernel<VEC, GL, NCH, U, RPW, 1, WP, T><<<grid, kBlock, 0, s>>>(items, (int)n_items, heavy, nh, col, wp, C,
                                                                            ep, partials);
      else
        agg_kernel<VEC, GL, NCH, U, RPW, 0, WP, T><<<grid, kBlock, 0, s>>>(items, (int)n_items, heavy, nh, col, wp, C,
                                                                            ep, partials);
    }
    GNPDE_LAUNCH_CHECK();
  }
  return GNPDE_OK;
}

// The lane geometry of a row width (lanes = ceil(C / VEC)), measured per width in
// round 1-2 (profiles/r02b_stripe_sweep.jsonl, r02b_layout_ab.jsonl).
template <int VEC, class WP, class T = float>
static int launch_agg_vec(const int4* items, int64_t n_items, int4* heavy, int64_t n_heavy, const int* col,
                          const WP& wp, int C, const Epi& ep, float* partials, hipStream_t s) {
  const int lanes = (int)ceil_div(C, VEC);
#define GNPDE_AGG(GL, NCH, U, RPW) \
  launch_agg_cfg<VEC, GL, NCH, U, RPW, WP, T>(items, n_items, heavy, n_heavy, col, wp, C, ep, partials, s)
  // Narrow rows (the column stripes of gnpde.dist at 2-8 GPUs: G-arxiv C = 128 / 8 = 16
  // floats = 4 lanes; G-rmat 256 / 8 = 32 floats = 8 lanes): several rows per
  // wavefront with 2-4 edges side by side per row slot, instead of one row per
  // wavefront idling 3/4 of a 16-lane group (G-arxiv rk4 step at 16 / 32 / 64 columns:
  // 0.133 / 0.152 / 0.243 ms against 0.266 / 0.270 / 0.296 with one row per wavefront).
  // A state far beyond the Infinity Cache (G-rmat stripes: 2M rows x 32-64 columns) is
  // gathered from HBM, where more independent rows per wavefront win (G-rmat rk4 step at
  // 32 / 64 columns 2.06 / 3.67 ms against 2.56 / 4.52); a cache-resident one (G-arxiv
  // stripes) prefers several edge groups per row (0.149 / 0.124 ms at 32 / 16 columns
  // against 0.283 / 0.318).
  // (plain weights and the GAT policy, takes_narrow_rows: the reference-score policy takes
  // the 16-lane geometry for narrow rows, which keeps the library's instantiation count down)
  if constexpr (takes_narrow_rows<WP>::value) {
    if (n_items * (int64_t)C * (int64_t)sizeof(T) > (int64_t)(96 << 20)) {
      if (lanes <= 4) return GNPDE_AGG(4, 1, 4, 16);
      if (lanes <= 8) return GNPDE_AGG(8, 1, 4, 8);
      if (lanes <= 16) return GNPDE_AGG(16, 1, 4, 4);
    }
    if (lanes <= 4) return GNPDE_AGG(4, 1, 4, 4);
    if (lanes <= 8) return GNPDE_AGG(8, 1, 8, 4);
    if (lanes <= 16) return GNPDE_AGG(16, 1, 4, 2);
  }
  if (lanes <= 16) return GNPDE_AGG(16, 1, 4, 1);
  if constexpr (sizeof(T) == 2 && VEC == 8) {
    // bf16 rows of 129-168 columns (BLEND: C = 162 padded to 168 = 21 lanes of 16 B):
    // three rows per wavefront, 63 of 64 lanes busy
    if (lanes > 16 && lanes <= 21) return GNPDE_AGG(21, 1, 4, 3);
  }
  // two rows per wavefront (fp32 C = 128 and bf16 rows of 17-32 lanes): with the
  // plan's items longest first, G-arxiv rk4 bench 9,301 against 8,643 RHS/s with
  // one row per wavefront
  if (lanes <= 32) return GNPDE_AGG(32, 1, 4, 2);
  if (lanes <= 64) return GNPDE_AGG(64, 1, 4, 1);
  if (lanes <= 128) return GNPDE_AGG(64, 2, 2, 1);
  if (lanes <= 256) return GNPDE_AGG(64, 4, 2, 1);
  if (lanes <= 512) return GNPDE_AGG(64, 8, 1, 1);
#undef GNPDE_AGG
  set_error("aggregate: C=%d too wide (max %d)", C, 512 * VEC);
  return GNPDE_EUNSUPPORTED;
}

// Widest vector (elements per lane: 4, 2 or 1 floats; 8, 4, 2 or 1 bf16) every
// operand of the aggregation and its epilogue allows: C, the leading dimensions
// and all pointers must agree.
// bf16 rows are sized to land in 17-32 lanes, the two-rows-per-wavefront
// geometry (launch_agg_vec): 8-byte gathers up to 128 columns, 16-byte gathers
// for 129-256 columns (G-arxiv, items longest first: C = 128 58 us against 77-96;
// BLEND C = 168 77 us against 93-122, 0.353-0.361 ms per rk4 step against 0.402).
template <class T = float>
inline int epi_vec_width(const Epi& ep, int64_t C, const void* partials) {
  const int kMax = sizeof(T) == 2 ? ((C > 128 && C <= 256) ? 8 : 4) : 16 / (int)sizeof(T);
  for (int v = kMax; v > 1; v >>= 1) {
    const size_t bytes = (size_t)v * sizeof(T);
    auto al = [&](const void* p) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) % bytes) == 0; };
    bool ok = C % v == 0 && ep.ldx % v == 0 && ep.ldf % v == 0 && al(ep.x);
    if (ep.flags & GNPDE_ADD_SOURCE) ok = ok && ep.ldx0 % v == 0 && al(ep.x0);
    if (ep.has_stage) {
      ok = ok && al(ep.st.f_out);
      for (int i = 0; i < ep.st.n_out; ++i) {
        ok = ok && al(ep.st.o[i].out) && al(ep.st.o[i].base);
      }
      for (int j = 0; j < ep.st.nk; ++j) ok = ok && al(ep.st.k[j]);
      if (ep.st.err_rows) ok = ok && al(ep.st.err.base) && al(ep.st.err_y0);
    } else {
      ok = ok && al(ep.f);
    }
    // fp32 partials are written with the same lane slices: v floats per lane (16-B pieces at most)
    ok = ok && (partials == nullptr || (reinterpret_cast<uintptr_t>(partials) % std::min<size_t>(16, 4 * v)) == 0);
    if (ok) return v;
  }
  return 1;
}

// The last launch of an rk4 solve with frozen rows (kStgFrozen): the plan's first n_items items
// (the rows that are not frozen) and, behind their workgroups, the frozen rows [r0, r1) of
// `home` taken through `steps` steps.  The headline geometry only — fp32 rows of 65-128
// columns, 16-byte slices, the fixed-grid epilogue (STG 1) — anything else is the caller's
// error: it keeps the full launch.
// (A template so that only the translation unit that calls it instantiates the kernel.)
template <class T = float>
static int launch_agg_frozen(const int32_t* items, int64_t n_items, int32_t* heavy, int64_t n_heavy,
                             const int32_t* col, const PlainWeights& wp, int64_t C, const Epi& ep, float* partials,
                             const float* home, int64_t r0, int64_t r1, int64_t steps, hipStream_t s) {
  constexpr int VEC = 4, GL = 32, RPW = 2;
  const int64_t lanes = ceil_div(C, VEC);
  GNPDE_REQUIRE(epi_vec_width<float>(ep, C, partials) == VEC && aligned16(home) && lanes > 16 && lanes <= GL,
                GNPDE_EUNSUPPORTED, "spmm_rhs_frozen: fp32 rows of 65-128 columns in 16-byte slices only (C=%lld)",
                (long long)C);
  GNPDE_REQUIRE(epi_stage_kind(ep) == 1 && ep.st.n_out == 1 && !ep.st.f_out && !ep.st.dense_tab && ep.st.f_lin == 0.f &&
                    !(ep.flags & GNPDE_ADD_SOURCE) && (ep.flags & GNPDE_EPI_RHS),
                GNPDE_EUNSUPPORTED, "spmm_rhs_frozen: the fixed-grid stage epilogue of the source-free RHS only");
  const unsigned grid = (unsigned)(ceil_div(n_items, (int64_t)kWavesPerBlock * RPW) +
                                   ceil_div(r1 - r0, (int64_t)frozen_rows_per_block<RPW>()));
  if (grid > 0) {
    agg_kernel<VEC, GL, 1, 4, RPW, kStgFrozen, PlainWeights, float><<<grid, kBlock, 0, s>>>(
        reinterpret_cast<const int4*>(items), (int)n_items, reinterpret_cast<int4*>(heavy), (int)n_heavy, col, wp,
        (int)C, ep, partials, home, (int)r0, (int)r1, (int)steps);
    GNPDE_LAUNCH_CHECK();
  }
  return GNPDE_OK;
}

template <class WP, class T = float>
static int launch_agg(const int32_t* items, int64_t n_items, int32_t* heavy, int64_t n_heavy,
                      const int32_t* col, const WP& wp, int64_t C, const Epi& ep, float* partials, hipStream_t s) {
  const int4* it = reinterpret_cast<const int4*>(items);
  int4* hv = reinterpret_cast<int4*>(heavy);
  const int c = (int)C;
  switch (epi_vec_width<T>(ep, C, partials)) {
    case 8:
      if constexpr (sizeof(T) == 2) return launch_agg_vec<8, WP, T>(it, n_items, hv, n_heavy, col, wp, c, ep, partials, s);
      [[fallthrough]];
    case 4: return launch_agg_vec<4, WP, T>(it, n_items, hv, n_heavy, col, wp, c, ep, partials, s);
    case 2: return launch_agg_vec<2, WP, T>(it, n_items, hv, n_heavy, col, wp, c, ep, partials, s);
    default: return launch_agg_vec<1, WP, T>(it, n_items, hv, n_heavy, col, wp, c, ep, partials, s);
  }
}

}  // namespace gnpde
