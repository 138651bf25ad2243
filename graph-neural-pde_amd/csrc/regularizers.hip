// regularizers.hip — the row passes of the ODE regularisers (gnpde.regularized_ODE_function):
//
//   gnpde_row_energy_f32   acc[r] (+)= sum_{i<n} coef_i * sum_c k_i[r,c]^2     (kinetic energy of the
//                          stage derivatives f_i, directional penalty of v_i = J^T f_i: one read of
//                          every array, the per-row sum carried in fp64)
//   gnpde_row_axpy_f32     out[r,:] = base[r,:] + sum_{j<2} coef_j * g_j[r] * src_j[r,:]   (their
//                          backward: a row-scaled array, alone or added to a stage adjoint)
//
// Both give a row of C <= 256 columns to a team of L lanes of one wavefront, L the power of two
// that covers the row's 16-byte units (C % 4 == 0 and every base 16-byte aligned) or its columns
// (otherwise), at most 64: a wavefront carries 64 / L short rows at once, as K1 batches them, and a
// lane strides its row by L.  The team's fp64 partial sums meet in an xor butterfly over the team's
// lanes; lane 0 of the team stores.  One owner per row, every sum in an order that the row length
// alone fixes: no atomics, and the same bits whatever the grid.
#include "common.hpp"

namespace gnpde {

constexpr int kRegMaxArrays = 4;
constexpr int kRegMaxCols = 256;
constexpr int kRegMaxBlocks = 8192;  // grid cap: gnpde_rk_combine_f32's geometry

struct EnergyArgs {
  const float* k[kRegMaxArrays];
  double c[kRegMaxArrays];
};

// team geometry of a row of `units` elements per lane-stride (float4 units or columns)
struct RowTeams {
  int L;      // lanes per row (power of two <= 64)
  int shift;  // log2 L
  int iters;  // strides of L that cover the row
};

inline RowTeams row_teams(int64_t units) {
  RowTeams t{1, 0, 1};
  while (t.L < kWave && t.L < units) {
    t.L <<= 1;
    ++t.shift;
  }
  t.iters = (int)ceil_div(units, t.L);
  return t;
}

template <bool VEC4, int N>
__global__ __launch_bounds__(256) void row_energy_kernel(int64_t R, int C, int shift, int iters, EnergyArgs a,
                                                         double* __restrict__ acc, int accumulate,
                                                         float* __restrict__ out) {
  const int L = 1 << shift;
  const int lane = threadIdx.x & (L - 1);
  const int64_t teams_per_block = blockDim.x >> shift;
  const int team = threadIdx.x >> shift;
  const int units = VEC4 ? C >> 2 : C;
  // every lane of a wavefront runs the same number of trips (the butterfly below reads its
  // neighbours' registers): the loop bound is per wavefront's first row
  const int64_t stride = (int64_t)gridDim.x * teams_per_block;
  const int rows_per_wave = kWave >> shift;
  for (int64_t r0 = (int64_t)blockIdx.x * teams_per_block + (team & ~(rows_per_wave - 1)); r0 < R; r0 += stride) {
    const int64_t r = r0 + (team & (rows_per_wave - 1));
    double s = 0.0;
    if (r < R) {
      const int64_t base = r * (int64_t)C;
      for (int it = 0; it < iters; ++it) {
        const int u = lane + (it << shift);
        if (u < units) {
          if constexpr (VEC4) {
            float4 v[N];
#pragma unroll
            for (int i = 0; i < N; ++i) v[i] = reinterpret_cast<const float4*>(a.k[i] + base)[u];
#pragma unroll
            for (int i = 0; i < N; ++i) {
              double q = (double)v[i].x * (double)v[i].x;
              q = fma((double)v[i].y, (double)v[i].y, q);
              q = fma((double)v[i].z, (double)v[i].z, q);
              q = fma((double)v[i].w, (double)v[i].w, q);
              s = fma(a.c[i], q, s);
            }
          } else {
            float v[N];
#pragma unroll
            for (int i = 0; i < N; ++i) v[i] = a.k[i][base + u];
#pragma unroll
            for (int i = 0; i < N; ++i) s = fma(a.c[i], (double)v[i] * (double)v[i], s);
          }
        }
      }
    }
    for (int o = 1; o < L; o <<= 1) s += __shfl_xor(s, o);
    if (lane == 0 && r < R) {
      if (acc) acc[r] = accumulate ? acc[r] + s : s;
      if (out) out[r] = (float)s;
    }
  }
}

struct AxpyArgs {
  const float* src[2];
  const void* g[2];
  double c[2];
  int n;
  int g_f64;
};

template <bool VEC4>
__global__ __launch_bounds__(256) void row_axpy_kernel(int64_t R, int C, int shift, int iters, const float* base,
                                                       AxpyArgs a, float* out) {
  // base and out are not __restrict__: out may be base (each element read by the lane that writes it)
  const int L = 1 << shift;
  const int lane = threadIdx.x & (L - 1);
  const int64_t teams_per_block = blockDim.x >> shift;
  const int units = VEC4 ? C >> 2 : C;
  const int64_t stride = (int64_t)gridDim.x * teams_per_block;
  for (int64_t r = (int64_t)blockIdx.x * teams_per_block + (threadIdx.x >> shift); r < R; r += stride) {
    double sc[2] = {0.0, 0.0};
    for (int j = 0; j < a.n; ++j) {
      const double gv = a.g_f64 ? reinterpret_cast<const double*>(a.g[j])[r]
                                : (double)reinterpret_cast<const float*>(a.g[j])[r];
      sc[j] = a.c[j] * gv;
    }
    const int64_t off = r * (int64_t)C;
    for (int it = 0; it < iters; ++it) {
      const int u = lane + (it << shift);
      if (u >= units) break;
      if constexpr (VEC4) {
        const float4 b = base ? reinterpret_cast<const float4*>(base + off)[u] : make_float4(0.f, 0.f, 0.f, 0.f);
        double x = b.x, y = b.y, z = b.z, w = b.w;
        for (int j = 0; j < a.n; ++j) {
          const float4 v = reinterpret_cast<const float4*>(a.src[j] + off)[u];
          x = fma(sc[j], (double)v.x, x);
          y = fma(sc[j], (double)v.y, y);
          z = fma(sc[j], (double)v.z, z);
          w = fma(sc[j], (double)v.w, w);
        }
        reinterpret_cast<float4*>(out + off)[u] = make_float4((float)x, (float)y, (float)z, (float)w);
      } else {
        double x = base ? (double)base[off + u] : 0.0;
        for (int j = 0; j < a.n; ++j) x = fma(sc[j], (double)a.src[j][off + u], x);
        out[off + u] = (float)x;
      }
    }
  }
}

template <bool VEC4>
static void launch_energy(int n, unsigned grid, hipStream_t s, int64_t R, int C, const RowTeams& t,
                          const EnergyArgs& a, double* acc, int accumulate, float* out) {
  switch (n) {
    case 1: row_energy_kernel<VEC4, 1><<<grid, kBlock, 0, s>>>(R, C, t.shift, t.iters, a, acc, accumulate, out); break;
    case 2: row_energy_kernel<VEC4, 2><<<grid, kBlock, 0, s>>>(R, C, t.shift, t.iters, a, acc, accumulate, out); break;
    case 3: row_energy_kernel<VEC4, 3><<<grid, kBlock, 0, s>>>(R, C, t.shift, t.iters, a, acc, accumulate, out); break;
    default: row_energy_kernel<VEC4, 4><<<grid, kBlock, 0, s>>>(R, C, t.shift, t.iters, a, acc, accumulate, out);
  }
}

}  // namespace gnpde

using namespace gnpde;

extern "C" int gnpde_row_energy_f32(int64_t R, int64_t C, int n, const float* const* ks, const double* coef,
                                    double* acc, int accumulate, float* out, void* stream) {
  GNPDE_REQUIRE(R >= 0 && ks && coef && (acc || out), GNPDE_EINVAL, "row_energy: bad args");
  GNPDE_REQUIRE(n >= 1 && n <= kRegMaxArrays, GNPDE_EUNSUPPORTED, "row_energy: n=%d not in [1, %d]", n,
                kRegMaxArrays);
  GNPDE_REQUIRE(C >= 1 && C <= kRegMaxCols, GNPDE_EUNSUPPORTED, "row_energy: C=%lld not in [1, %d]", (long long)C,
                kRegMaxCols);
  if (R == 0) return GNPDE_OK;
  EnergyArgs a{};
  bool vec4 = C % 4 == 0;
  for (int i = 0; i < n; ++i) {
    GNPDE_REQUIRE(ks[i] != nullptr, GNPDE_EINVAL, "row_energy: ks[%d] is NULL", i);
    a.k[i] = ks[i];
    a.c[i] = coef[i];
    vec4 = vec4 && aligned16(ks[i]);
  }
  const RowTeams t = row_teams(vec4 ? C / 4 : C);
  const int64_t rows_per_block = kBlock >> t.shift;
  const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(R, rows_per_block), kRegMaxBlocks);
  hipStream_t s = as_stream(stream);
  if (vec4)
    launch_energy<true>(n, grid, s, R, (int)C, t, a, acc, accumulate, out);
  else
    launch_energy<false>(n, grid, s, R, (int)C, t, a, acc, accumulate, out);
  GNPDE_LAUNCH_CHECK();
  return GNPDE_OK;
}

extern "C" int gnpde_row_axpy_f32(int64_t R, int64_t C, const float* base, int n, const float* const* src,
                                  const void* const* g, int g_f64, const double* coef, float* out, void* stream) {
  GNPDE_REQUIRE(R >= 0 && out && (n == 0 || (src && g && coef)), GNPDE_EINVAL, "row_axpy: bad args");
  GNPDE_REQUIRE(n >= 0 && n <= 2, GNPDE_EUNSUPPORTED, "row_axpy: n=%d not in [0, 2]", n);
  GNPDE_REQUIRE(C >= 1 && C <= kRegMaxCols, GNPDE_EUNSUPPORTED, "row_axpy: C=%lld not in [1, %d]", (long long)C,
                kRegMaxCols);
  if (R == 0) return GNPDE_OK;
  AxpyArgs a{};
  a.n = n;
  a.g_f64 = g_f64 != 0;
  bool vec4 = C % 4 == 0 && aligned16(out) && (base == nullptr || aligned16(base));
  for (int j = 0; j < n; ++j) {
    GNPDE_REQUIRE(src[j] != nullptr && g[j] != nullptr, GNPDE_EINVAL, "row_axpy: term %d has a NULL array", j);
    GNPDE_REQUIRE(src[j] != out, GNPDE_EINVAL, "row_axpy: out aliases src[%d] (only base may be out)", j);
    a.src[j] = src[j];
    a.g[j] = g[j];
    a.c[j] = coef[j];
    vec4 = vec4 && aligned16(src[j]);
  }
  const RowTeams t = row_teams(vec4 ? C / 4 : C);
  const int64_t rows_per_block = kBlock >> t.shift;
  const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(R, rows_per_block), kRegMaxBlocks);
  hipStream_t s = as_stream(stream);
  if (vec4)
    row_axpy_kernel<true><<<grid, kBlock, 0, s>>>(R, (int)C, t.shift, t.iters, base, a, out);
  else
    row_axpy_kernel<false><<<grid, kBlock, 0, s>>>(R, (int)C, t.shift, t.iters, base, a, out);
  GNPDE_LAUNCH_CHECK();
  return GNPDE_OK;
}
