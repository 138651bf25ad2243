// adams.hip — the streaming passes of the Adams-Bashforth-Moulton multistep solvers
// (gnpde.integrator: explicit_adams / implicit_adams, torchdiffeq's fixed_adams).
//
// predict: one read of the state and of up to 11 history arrays gives the predictor
// increment dy, the next RHS input x = y0 + dy and (implicit) the corrector's constant
// part delta.  The order-11 coefficients alternate in sign with sum |b| ~ 591, so the
// sums are carried in fp64 per element and rounded once at the store; the pass is
// bandwidth-bound and the fp64 multiply-adds ride under the loads.
//
// correct: one corrector iteration dy = cf f + delta, x = y0 + dy, and the convergence
// ratio max_i |dy_old - dy| / (atol + rtol max(|dy_old|, |dy|)) reduced per workgroup and
// finished by the workgroup that arrives last.  The launch is gated on the status record:
// once an iteration has converged, later launches of the step return at once, so the host
// may enqueue several iterations and read the status once.
#include "common.hpp"

namespace gnpde {

constexpr int kAdamsMaxHist = GNPDE_ADAMS_MAX_HISTORY;
constexpr int kAdamsMaxBlocks = 2048;         // grid cap of the corrector: one partial per workgroup
constexpr int kAdamsPredictMaxBlocks = 8192;  // grid cap of the predictor: gnpde_rk_combine_f32's geometry

struct AdamsPredictArgs {
  const float* h[kAdamsMaxHist];
  double cdy[kAdamsMaxHist];
  double cdelta[kAdamsMaxHist];
  int nh;
};

template <int VEC>
struct alignas(4 * VEC) AdamsVec {
  float v[VEC];
};

// One group of VEC consecutive elements (group index i: elements i * VEC ...).  The loads of
// the group are issued together (a uniform j < nh guard per array), then the two fp64 chains
// run over them.
template <int VEC, bool DELTA>
__device__ __forceinline__ void adams_predict_group(int64_t i, const float* __restrict__ y0, const AdamsPredictArgs& a,
                                                    float* __restrict__ dy, float* __restrict__ x,
                                                    float* __restrict__ delta) {
  using Vec = AdamsVec<VEC>;
  const int nh = a.nh;
  Vec hv[kAdamsMaxHist];
#pragma unroll
  for (int j = 0; j < kAdamsMaxHist; ++j)
    if (j < nh) hv[j] = reinterpret_cast<const Vec*>(a.h[j])[i];
  const Vec yv = reinterpret_cast<const Vec*>(y0)[i];
  double sdy[VEC], sde[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) sdy[e] = sde[e] = 0.0;
#pragma unroll
  for (int j = 0; j < kAdamsMaxHist; ++j) {
    if (j < nh) {
      const double cy = a.cdy[j], cd = DELTA ? a.cdelta[j] : 0.0;
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const double v = (double)hv[j].v[e];
        sdy[e] = fma(cy, v, sdy[e]);
        if constexpr (DELTA) sde[e] = fma(cd, v, sde[e]);
      }
    }
  }
  Vec ody, ox, ode;
#pragma unroll
  for (int e = 0; e < VEC; ++e) {
    ody.v[e] = (float)sdy[e];
    ox.v[e] = (float)((double)yv.v[e] + sdy[e]);
    ode.v[e] = (float)sde[e];
  }
  reinterpret_cast<Vec*>(dy)[i] = ody;
  reinterpret_cast<Vec*>(x)[i] = ox;
  if constexpr (DELTA) reinterpret_cast<Vec*>(delta)[i] = ode;
}

// VEC = 4: 16-byte accesses over the n / 4 whole groups and a scalar tail for the n % 4
// elements behind them (the first lanes of workgroup 0); VEC = 1: bases that are not 16-byte
// aligned.
template <int VEC, bool DELTA>
__global__ __launch_bounds__(kBlock) void adams_predict_kernel(int64_t n, const float* __restrict__ y0,
                                                              AdamsPredictArgs a, float* __restrict__ dy,
                                                              float* __restrict__ x, float* __restrict__ delta) {
  const int64_t groups = n / VEC;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < groups; i += stride)
    adams_predict_group<VEC, DELTA>(i, y0, a, dy, x, delta);
  if constexpr (VEC > 1) {
    const int64_t e = groups * VEC + threadIdx.x;
    if (blockIdx.x == 0 && e < n) adams_predict_group<1, DELTA>(e, y0, a, dy, x, delta);
  }
}

// The ratio as an ordered unsigned word: ratios are >= 0 or NaN, non-negative floats order
// like their bit patterns, and the canonical NaN (0x7fc00000) lies above +inf — an unsigned
// maximum of these words is a maximum that keeps a NaN (fmax would drop it).
__device__ __forceinline__ unsigned ratio_word(double r) {
  if (r != r) return 0x7fc00000u;
  const float f = (float)r;  // (a ratio beyond fp32's range rounds to +inf: not converged either way)
  return __float_as_uint(f < 0.f ? 0.f : f);
}

struct AdamsWorkspace {
  gnpde_adams_status_t st;
  unsigned part[kAdamsMaxBlocks];  // one ratio word per workgroup of the running launch
};

// A lane's running maximum of the ratios num / den, kept as the pair itself: two candidates are
// compared by cross-multiplication (fp64 products of fp32-range values cannot overflow), so the
// pass takes one fp64 division per lane instead of one per element.  ``nan``: some ratio was NaN
// (a NaN operand, 0 / 0 with both tolerances zero, or inf / inf).
struct AdamsRatio {
  double num = 0.0, den = 1.0;
  bool nan = false;
  __device__ __forceinline__ void take(double n, double d) {
    if (n != n || !(d > 0.0) || d == __builtin_inf()) {
      nan = true;
    } else if (n * den > num * d) {
      num = n;
      den = d;
    }
  }
  __device__ __forceinline__ unsigned word() const { return nan ? 0x7fc00000u : ratio_word(num / den); }
};

// One group of VEC elements of a corrector iteration.
template <int VEC>
__device__ __forceinline__ void adams_correct_group(int64_t i, const float* __restrict__ f,
                                                    const float* __restrict__ delta, const float* __restrict__ y0,
                                                    double cf, double rtol, double atol, float* __restrict__ dy,
                                                    float* __restrict__ x, AdamsRatio& best) {
  using Vec = AdamsVec<VEC>;
  const Vec fv = reinterpret_cast<const Vec*>(f)[i];
  const Vec dv = reinterpret_cast<const Vec*>(delta)[i];
  const Vec yv = reinterpret_cast<const Vec*>(y0)[i];
  const Vec old = reinterpret_cast<const Vec*>(dy)[i];
  Vec ody, ox;
#pragma unroll
  for (int e = 0; e < VEC; ++e) {
    const double s = fma(cf, (double)fv.v[e], (double)dv.v[e]);
    const float nd = (float)s;
    ody.v[e] = nd;
    ox.v[e] = (float)((double)yv.v[e] + s);
    const double a0 = fabs((double)old.v[e]), a1 = fabs((double)nd);
    // (a NaN in either dy makes the numerator NaN, whichever side the comparison picks)
    best.take(fabs((double)old.v[e] - (double)nd), atol + rtol * (a0 > a1 ? a0 : a1));
  }
  reinterpret_cast<Vec*>(dy)[i] = ody;
  reinterpret_cast<Vec*>(x)[i] = ox;
}

template <int VEC>
__global__ __launch_bounds__(kBlock) void adams_correct_kernel(int64_t n, const float* __restrict__ f,
                                                              const float* __restrict__ delta,
                                                              const float* __restrict__ y0, double cf, double rtol,
                                                              double atol, float* __restrict__ dy,
                                                              float* __restrict__ x, AdamsWorkspace* ws) {
  __shared__ unsigned red[kWavesPerBlock];
  __shared__ int last_s;
  // The gate.  The record is written only by the last workgroup of an ungated launch, after
  // every workgroup of that launch has read it here and taken its arrival ticket below, so all
  // workgroups of one launch read the same value.
  if (__hip_atomic_load(&ws->st.converged, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return;
  const int64_t groups = n / VEC;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  AdamsRatio best;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < groups; i += stride)
    adams_correct_group<VEC>(i, f, delta, y0, cf, rtol, atol, dy, x, best);
  if constexpr (VEC > 1) {  // the n % VEC elements behind the whole groups
    const int64_t e = groups * VEC + threadIdx.x;
    if (blockIdx.x == 0 && e < n) adams_correct_group<1>(e, f, delta, y0, cf, rtol, atol, dy, x, best);
  }
  unsigned w = best.word();
  // workgroup maximum: wavefront shuffles, then the four wave words through LDS
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const unsigned other = (unsigned)__shfl_xor((int)w, o);
    w = other > w ? other : w;
  }
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  if (lane == 0) red[wave] = w;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned m = red[0];
    for (int k = 1; k < kWavesPerBlock; ++k) m = red[k] > m ? red[k] : m;
    // The partial goes out write-through (an agent-scope atomic store) and is drained before the
    // arrival ticket, which is what an agent-scope release orders at the ISA level; the ticket is
    // not a formal release as well (aggregate.hpp, kHubTicketOrder): that writes back every dirty
    // line of the XCD's L2 — this pass's own dy and x — once per workgroup, and ran the pass at
    // under half of the predictor's bytes/s.  The last arrival reads the partials with agent-scope
    // atomic loads, which no stale cache line can serve.
    __hip_atomic_store(&ws->part[blockIdx.x], m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned t = __hip_atomic_fetch_add(&ws->st.arrivals, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // (no instruction: the loads below stay behind it)
    last_s = (t == gridDim.x - 1) ? 1 : 0;
  }
  __syncthreads();
  if (!last_s) return;
  // the last workgroup: the maximum of the partials, then the record
  unsigned m = 0u;
  for (unsigned b = threadIdx.x; b < gridDim.x; b += blockDim.x) {
    const unsigned p = __hip_atomic_load(&ws->part[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    m = p > m ? p : m;
  }
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const unsigned other = (unsigned)__shfl_xor((int)m, o);
    m = other > m ? other : m;
  }
  __syncthreads();  // red[] was read by thread 0 above
  if (lane == 0) red[wave] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < kWavesPerBlock; ++k) m = red[k] > m ? red[k] : m;
    const float ratio = __uint_as_float(m);
    ws->st.ratio = ratio;
    ws->st.iterations = ws->st.iterations + 1;
    __hip_atomic_store(&ws->st.arrivals, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // last: the gate of the launches behind this one (a NaN ratio compares false)
    __hip_atomic_store(&ws->st.converged, ratio < 1.f ? 1 : 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

inline unsigned adams_grid(int64_t groups, int cap) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(groups, kBlock), cap));
}

}  // namespace gnpde

using namespace gnpde;

extern "C" {

int gnpde_adams_predict_f32(int64_t n, const float* y0, int nh, const float* const* hist, const double* cdy,
                            const double* cdelta, float* dy, float* x, float* delta, void* stream) {
  GNPDE_REQUIRE(n >= 0 && y0 && dy && x, GNPDE_EINVAL, "adams_predict: NULL y0 / dy / x or n < 0");
  GNPDE_REQUIRE(nh >= 1 && nh <= kAdamsMaxHist, GNPDE_EUNSUPPORTED, "adams_predict: nh=%d not in [1, %d]", nh,
                kAdamsMaxHist);
  GNPDE_REQUIRE(hist && cdy, GNPDE_EINVAL, "adams_predict: NULL hist / cdy");
  GNPDE_REQUIRE((delta == nullptr) == (cdelta == nullptr), GNPDE_EINVAL,
                "adams_predict: delta and cdelta go together");
  AdamsPredictArgs a;
  a.nh = nh;
  bool vec4 = n >= 4 && aligned16(y0) && aligned16(dy) && aligned16(x) && (!delta || aligned16(delta));
  for (int j = 0; j < kAdamsMaxHist; ++j) {
    a.h[j] = j < nh ? hist[j] : nullptr;
    a.cdy[j] = j < nh ? cdy[j] : 0.0;
    a.cdelta[j] = (j < nh && cdelta) ? cdelta[j] : 0.0;
    if (j < nh) {
      GNPDE_REQUIRE(hist[j] != nullptr, GNPDE_EINVAL, "adams_predict: hist[%d] is NULL", j);
      GNPDE_REQUIRE(hist[j] != dy && hist[j] != x && hist[j] != delta, GNPDE_EINVAL,
                    "adams_predict: hist[%d] aliases an output", j);
      vec4 = vec4 && aligned16(hist[j]);
    }
  }
  GNPDE_REQUIRE(dy != x && dy != delta && x != delta && y0 != dy && y0 != x && y0 != delta, GNPDE_EINVAL,
                "adams_predict: outputs alias each other or y0");
  if (n == 0) return GNPDE_OK;
  hipStream_t s = as_stream(stream);
  const unsigned grid = adams_grid(vec4 ? n / 4 : n, kAdamsPredictMaxBlocks);
  if (vec4) {
    if (delta)
      adams_predict_kernel<4, true><<<grid, kBlock, 0, s>>>(n, y0, a, dy, x, delta);
    else
      adams_predict_kernel<4, false><<<grid, kBlock, 0, s>>>(n, y0, a, dy, x, delta);
  } else {
    if (delta)
      adams_predict_kernel<1, true><<<grid, kBlock, 0, s>>>(n, y0, a, dy, x, delta);
    else
      adams_predict_kernel<1, false><<<grid, kBlock, 0, s>>>(n, y0, a, dy, x, delta);
  }
  GNPDE_LAUNCH_CHECK();
  return GNPDE_OK;
}

size_t gnpde_adams_workspace_bytes(void) { return sizeof(AdamsWorkspace); }

int gnpde_adams_status_reset(void* workspace, void* stream) {
  GNPDE_REQUIRE(workspace && aligned16(workspace), GNPDE_EINVAL, "adams_status_reset: workspace NULL or unaligned");
  GNPDE_HIP(hipMemsetAsync(workspace, 0, sizeof(gnpde_adams_status_t), as_stream(stream)));
  return GNPDE_OK;
}

int gnpde_adams_correct_f32(int64_t n, const float* f, const float* delta, const float* y0, double cf, double rtol,
                            double atol, float* dy, float* x, void* workspace, size_t workspace_bytes, void* stream) {
  GNPDE_REQUIRE(n >= 1 && f && delta && y0 && dy && x, GNPDE_EINVAL, "adams_correct: NULL operand or n < 1");
  GNPDE_REQUIRE(workspace && aligned16(workspace) && workspace_bytes >= sizeof(AdamsWorkspace), GNPDE_EINVAL,
                "adams_correct: workspace NULL, unaligned or smaller than %zu bytes", sizeof(AdamsWorkspace));
  GNPDE_REQUIRE(dy != x && dy != f && dy != delta && dy != y0 && x != f && x != delta && x != y0, GNPDE_EINVAL,
                "adams_correct: dy / x alias an operand");
  GNPDE_REQUIRE(rtol >= 0.0 && atol >= 0.0, GNPDE_EINVAL, "adams_correct: negative tolerance");
  const bool vec4 = n >= 4 && aligned16(f) && aligned16(delta) && aligned16(y0) && aligned16(dy) && aligned16(x);
  hipStream_t s = as_stream(stream);
  const unsigned grid = adams_grid(vec4 ? n / 4 : n, kAdamsMaxBlocks);
  AdamsWorkspace* ws = static_cast<AdamsWorkspace*>(workspace);
  if (vec4)
    adams_correct_kernel<4><<<grid, kBlock, 0, s>>>(n, f, delta, y0, cf, rtol, atol, dy, x, ws);
  else
    adams_correct_kernel<1><<<grid, kBlock, 0, s>>>(n, f, delta, y0, cf, rtol, atol, dy, x, ws);
  GNPDE_LAUNCH_CHECK();
  return GNPDE_OK;
}

}  // extern "C"
