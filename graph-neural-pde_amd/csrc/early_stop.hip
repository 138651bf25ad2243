// early_stop.hip — the early-stop test integrator's score of one state
// (gnpde.early_stop_solver; src/early_stop_solver.py:108-128, :194-201): decode the state
// with the model's output layer, take the argmax and count the correct rows of the train /
// validation / test splits — one launch, no logits in memory, no host read
// (gnpde_decode_score_f32).
#include "common.hpp"

namespace gnpde {

constexpr int kScoreRows = 32;      // most state rows per tile (one lane of wave 0 each in the argmax phase)
constexpr int kScoreGroups = 8;     // most row groups G of a tile; a work item: one class x the rows q, q+G, q+2G, q+3G
constexpr int kScoreWFloats = 6656; // LDS floats of the weight chunk (ogbn-arxiv's 40 x 162 in one)
constexpr int kScoreMaxJC = 192;    // widest chunk of decoder columns

// Columns of one chunk: the whole decoder input when K * Cd fits, else as many as do.
inline int score_chunk_cols(int K, int Cd) { return std::min(Cd, std::min(kScoreMaxJC, kScoreWFloats / K)); }

// Row groups of a tile: as many as give every thread of the workgroup at most one work item
// (G * K <= 256: ogbn-arxiv's 40 classes take 6 groups, tiles of 24 rows, one pass of 240 threads).
inline int score_groups(int K) { return std::max(1, std::min(kScoreGroups, kBlock / K)); }

inline size_t score_lds_bytes(int K, int JC, int G) {
  const size_t TR = 4 * (size_t)G;
  return sizeof(float) * ((size_t)K * JC + K + TR * (JC + 1) + TR * K) + sizeof(int) * 2 * kScoreRows;
}

// A workgroup walks tiles of TR = 4 G state rows.  Per tile: the rows' split masks and labels
// (through `rows` when the state is renumbered); relu of the scored rows into LDS, a
// chunk of JC decoder columns at a time (an unscored row is never read); every work
// item adds its class's products over the chunk, j ascending, to four rows' logits
// (the weight chunk transposed in LDS: lanes of consecutive classes read consecutive
// words, lanes of one row quad the same state word); lane r of wave 0 takes row r's
// argmax (strict >: the lowest class wins a tie) and counts its hits per split.  The
// counts leave the workgroup as at most three integer atomics, after a wavefront sum.
__global__ __launch_bounds__(kBlock) void decode_score_kernel(const float* __restrict__ y, int R, int64_t ld, int Cd,
                                                              const float* __restrict__ W,
                                                              const float* __restrict__ b, int K,
                                                              const uint8_t* __restrict__ split,
                                                              const int* __restrict__ label,
                                                              const int* __restrict__ rows, int* counts,
                                                              int* __restrict__ pred_out, int JC, int G, int n_tiles) {
  extern __shared__ __align__(16) float smem[];
  float* Wt = smem;                                  // [JC][K]
  float* bs = Wt + (size_t)K * JC;                   // [K]
  const int TR = 4 * G;
  float* z = bs + K;                                 // [TR][JC + 1]
  float* lg = z + (size_t)TR * (JC + 1);             // [TR][K]
  int* sp = reinterpret_cast<int*>(lg + (size_t)TR * K);  // [32] split masks (0: unscored)
  int* lb = sp + kScoreRows;                         // [32] labels
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int ldz = JC + 1;
  const int n_chunks = (Cd + JC - 1) / JC;
  for (int c = tid; c < K; c += kBlock) bs[c] = b ? b[c] : 0.f;
  int hit0 = 0, hit1 = 0, hit2 = 0;
  bool w_loaded = false;
  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int r0 = tile * TR;
    if (tid < TR) {
      const int r = r0 + tid;
      int s = 0, l = -1;
      if (r < R) {
        const int src = rows ? rows[r] : r;
        if (src >= 0 && src < R) {
          s = split[src] & 7;
          if (s) l = label[src];
        }
      }
      sp[tid] = s;
      lb[tid] = l;
    }
    for (int i = tid; i < TR * K; i += kBlock) lg[i] = 0.f;
    __syncthreads();
    for (int ch = 0; ch < n_chunks; ++ch) {
      const int j0 = ch * JC;
      const int jc = min(JC, Cd - j0);
      if (!w_loaded || n_chunks > 1) {
        for (int i = tid; i < K * jc; i += kBlock) {
          const int c = i / jc, jj = i - c * jc;
          Wt[jj * K + c] = W[(int64_t)c * Cd + j0 + jj];
        }
        w_loaded = true;
      }
      for (int row = wave; row < TR; row += kWavesPerBlock) {
        float* zr = z + row * ldz;
        if (sp[row]) {
          const float* yr = y + (int64_t)(r0 + row) * ld + j0;
          for (int jj = lane; jj < jc; jj += kWave) {
            const float v = yr[jj];
            zr[jj] = v < 0.f ? 0.f : v;
          }
        } else {
          for (int jj = lane; jj < jc; jj += kWave) zr[jj] = 0.f;
        }
      }
      __syncthreads();
      for (int item = tid; item < G * K; item += kBlock) {
        const int q = item / K, c = item - q * K;
        if (!(sp[q] | sp[q + G] | sp[q + 2 * G] | sp[q + 3 * G])) continue;
        const float* z0 = z + q * ldz;
        const float* z1 = z0 + G * ldz;
        const float* z2 = z1 + G * ldz;
        const float* z3 = z2 + G * ldz;
        float* l0 = lg + q * K + c;
        float* l1 = l0 + G * K;
        float* l2 = l1 + G * K;
        float* l3 = l2 + G * K;
        float a0 = *l0, a1 = *l1, a2 = *l2, a3 = *l3;
        for (int jj = 0; jj < jc; ++jj) {
          const float w = Wt[jj * K + c];
          a0 = fmaf(w, z0[jj], a0);
          a1 = fmaf(w, z1[jj], a1);
          a2 = fmaf(w, z2[jj], a2);
          a3 = fmaf(w, z3[jj], a3);
        }
        *l0 = a0;
        *l1 = a1;
        *l2 = a2;
        *l3 = a3;
      }
      __syncthreads();
    }
    if (tid < TR) {
      const int s = sp[tid];
      int p = -1;
      if (s) {
        const float* l = lg + tid * K;
        float best = l[0] + bs[0];
        p = 0;
        for (int c = 1; c < K; ++c) {
          const float v = l[c] + bs[c];
          if (v > best) {
            best = v;
            p = c;
          }
        }
        if (p == lb[tid]) {
          hit0 += s & 1;
          hit1 += (s >> 1) & 1;
          hit2 += (s >> 2) & 1;
        }
      }
      if (pred_out && r0 + tid < R) pred_out[r0 + tid] = p;
    }
    __syncthreads();
  }
  if (wave == 0) {  // lanes >= 32 hold zeros
    for (int o = 32; o > 0; o >>= 1) {
      hit0 += __shfl_xor(hit0, o);
      hit1 += __shfl_xor(hit1, o);
      hit2 += __shfl_xor(hit2, o);
    }
    if (lane == 0) {
      if (hit0) atomicAdd(counts + 0, hit0);
      if (hit1) atomicAdd(counts + 1, hit1);
      if (hit2) atomicAdd(counts + 2, hit2);
    }
  }
}

}  // namespace gnpde

using namespace gnpde;

extern "C" {

int gnpde_decode_score_f32(const float* y, int64_t R, int64_t ld, int64_t Cd, const float* W, const float* b,
                           int64_t K, const uint8_t* split, const int32_t* label, const int32_t* rows,
                           int32_t* counts, int32_t* pred_out, void* stream) {
  GNPDE_REQUIRE(R >= 0 && R < INT32_MAX - kScoreRows, GNPDE_EINVAL, "decode_score: R=%lld out of range", (long long)R);
  GNPDE_REQUIRE(K >= 1, GNPDE_EINVAL, "decode_score: K=%lld must be >= 1", (long long)K);
  GNPDE_REQUIRE(Cd >= 1 && Cd <= ld, GNPDE_EINVAL, "decode_score: Cd=%lld must be in [1, ld=%lld]", (long long)Cd,
                (long long)ld);
  GNPDE_REQUIRE(counts && W && (R == 0 || (y && split && label)), GNPDE_EINVAL,
                "decode_score: NULL y / W / split / label / counts");
  GNPDE_REQUIRE(K <= 128 && Cd <= 512, GNPDE_EUNSUPPORTED,
                "decode_score: K=%lld, Cd=%lld outside the kernel's range (K <= 128, Cd <= 512)", (long long)K,
                (long long)Cd);
  if (R == 0) return GNPDE_OK;
  const int JC = score_chunk_cols((int)K, (int)Cd);
  const int G = score_groups((int)K);
  const size_t lds = score_lds_bytes((int)K, JC, G);  // < 64 KiB for every supported K, Cd
  const int n_tiles = (int)ceil_div(R, 4 * G);
  const unsigned grid = (unsigned)std::min<int64_t>(n_tiles, 768);
  decode_score_kernel<<<grid, kBlock, lds, as_stream(stream)>>>(y, (int)R, ld, (int)Cd, W, b, (int)K, split, label,
                                                                 rows, counts, pred_out, JC, G, n_tiles);
  GNPDE_LAUNCH_CHECK();
  return GNPDE_OK;
}

}  // extern "C"
