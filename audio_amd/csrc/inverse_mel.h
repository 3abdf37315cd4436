// InverseMelScale (F.inverse_mel_scale / T.InverseMelScale): out[v][f] = relu(sum_m P[f][m] y[v][m]) over all frames v of all
// rows, P the (n_stft, n_mels) pseudo-inverse of the mel filterbank that the host builds (_host.inverse_mel_matrix).  A dense
// (frames x n_mels) . (n_mels x n_stft) product with n_stft in the hundreds; one launch.
//
// Arithmetic.  v_mfma_f32_16x16x4_f32: exact float32 FMA chains.  A = a tile of P (16 bins x 4 mels), B = a tile of y^T
// (4 mels x 16 frames), so D holds 16 bins x 16 frames and a lane ends with 4 consecutive bins of one frame.  Every output
// has ONE accumulator that starts at zero and takes its products in ascending m (the instruction adds its 4 products in
// ascending k, the steps follow in ascending m): the result does not depend on the tile a frame falls in, on the number of
// rows, on the input's layout or on its alignment.  mels beyond n_mels up to the next multiple of 4 are zeros on both sides.
//
// Tile plan.  A workgroup of 4 waves owns kFrames = 64 consecutive frames of ONE row (wave w: frames 16 w .. 16 w + 15):
//   stage_y   the frames' mel values, read in place through the strides, widened (float16 / bfloat16), optionally exp'ed
//             (log_input: the accurate expf), written to LDS once, in the order the B operand is read;
//   per tile of kBins = 64 bins of n_stft (n_stft is tiled through LDS, 513 and 1025 take 9 and 17 tiles):
//     stage_p   the tile's 64 rows of P from global memory (L2-resident: P is at most 1 MiB) to LDS: the host lays P out tile
//               by tile in the A operand's order, so this is a straight copy in 16-byte accesses;
//     mma       n_mels / 4 steps; per step one B read and, per 16 bins of the tile that exist, one A read and one MFMA
//               (up to 4 independent accumulators per wave: the dependent latency of 40 cycles is covered);
//               the accumulators go to the output tile in LDS, [frame][bin];
//     store     relu, the one rounding to the output type, rows of 64 consecutive bins per wave: coalesced whatever
//               n_stft is (a frame's row of 201 or 513 elements starts on no 16-byte boundary).
// Operand order in LDS ("fragment order"): element (m, j) -- j the frame or the bin within the tile -- sits at
//   ((m / 4) * 4 + j / 16) * 64 + (m % 4) * 16 + j % 16,
// so that the 64 lanes of an operand read are 64 consecutive floats: no bank conflict, no padding.
// LDS: (2 * 64 * K4 + 64 * 68) * 4 bytes with K4 = n_mels rounded up to 4: 57 KB at 80 mels, 145 KB at the limit of 256.
//
// Input layouts (Args::time_major).  0: unit stride along mel, `st` elements between frames (the frame-major view every
// MelSpectrogram here returns); a lane loads 16 bytes along mel.  1: unit stride along time, `sm` elements between mels
// (a contiguous (B, n_mels, T)); a lane loads 16 bytes along time.  A group of 16 bytes that does not start on a 16-byte
// boundary, or that crosses the end of its row, is loaded element by element: the same values, so the same bits.
//
// The phase functions are AAMD_HD: tests/cpu_sim/sim_inverse_mel.cpp replays them with g++ (fmaf for the MFMA chain).
#pragma once
#include <math.h>

#include "wave_augment.h"

namespace aamd {
namespace iml {

using wa::Elem;
using wa::Vec;
using wa::aligned16;
using wa::load_group;

constexpr int kThreads = 256;
constexpr int kFrames = 64;               // frames of one row per workgroup
constexpr int kBins = 64;                 // bins of n_stft per LDS tile
constexpr int kSub = 16;                  // the MFMA's tile edge
constexpr int kOutPitch = kBins + 4;      // floats between two frames of the output tile (rows stay 16-byte aligned)
constexpr int kMaxMels = 256;
constexpr int kBatch = 8;                 // 16-byte loads per thread that a staging phase issues together

struct Args {
  const void* x;                // (rows, n_mels, T) through sr / sm / st
  const float* P;               // ceil(F / kBins) tiles of kBins * K4 floats in fragment order, 16-byte aligned
  void* out;                    // dense (rows, T, F)
  int64_t rows, T, sr, sm, st;
  int32_t F, K;                 // n_stft, n_mels
  int32_t time_major;           // 0: sm == 1; 1: st == 1
  int32_t log_input;            // y = expf(x)
};

AAMD_HD int k_pad(int K) { return (K + 3) & ~3; }
AAMD_HD int64_t tiles_per_row(int64_t T) { return (T + kFrames - 1) / kFrames; }
AAMD_HD int64_t lds_floats(int K) { return 2 * (int64_t)kFrames * k_pad(K) + (int64_t)kFrames * kOutPitch; }
AAMD_HD int frag_index(int m, int j) { return (((m >> 2) * 4 + (j >> 4)) << 6) + ((m & 3) << 4) + (j & 15); }
AAMD_HD float prologue(float v, int log_input) { return log_input ? expf(v) : v; }

// The two staging phases issue the loads of kBatch items per thread together and write them to LDS afterwards, so that a
// workgroup waits for one round trip to memory per kBatch * kThreads items, not for one per item.
//
// The workgroup's frames [t0, t0 + kFrames) of `row` into LDS in fragment order; frames beyond T and mels beyond K are zeros.
template <int DT>
AAMD_HD void stage_y(int tid, const Args& a, int64_t row, int64_t t0, float* yfrag) {
  using E = Elem<DT>;
  using S = typename E::S;
  constexpr int V = 16 / sizeof(S);
  const S* base = static_cast<const S*>(a.x) + row * a.sr;
  const int KP = k_pad(a.K);
  if (!a.time_major) {
    // 16 frames x 4 groups of V mels per wave instruction: 4 V consecutive elements of every frame's row
    const int n = (((KP + V - 1) / V + 3) & ~3) * kFrames;
    for (int q0 = tid; q0 < n; q0 += kBatch * kThreads) {
      Vec<S> g[kBatch];
#pragma unroll
      for (int j = 0; j < kBatch; ++j) {
        const int q = q0 + j * kThreads, rest = q >> 6;
        const int fr = (rest & 3) * kSub + (q & 15), m0 = ((rest >> 2) * 4 + ((q >> 4) & 3)) * V;
        const int64_t t = t0 + fr;
        g[j] = Vec<S>{};
        if (q < n && m0 < a.K && t < a.T) {
          const S* p = base + t * a.st;
          load_group(p, aligned16(p + m0), (int64_t)m0, (int64_t)a.K, g[j]);
        }
      }
#pragma unroll
      for (int j = 0; j < kBatch; ++j) {
        const int q = q0 + j * kThreads, rest = q >> 6;
        const int fr = (rest & 3) * kSub + (q & 15), m0 = ((rest >> 2) * 4 + ((q >> 4) & 3)) * V;
        if (q >= n || m0 >= KP) continue;
        const bool live = t0 + fr < a.T;
#pragma unroll
        for (int k = 0; k < V; ++k)
          if (m0 + k < KP)
            yfrag[frag_index(m0 + k, fr)] = live && m0 + k < a.K ? prologue(E::load(g[j].e[k]), a.log_input) : 0.0f;
      }
    }
  } else {
    // kFrames / V groups of V frames per mel: a wave instruction reads whole rows of 64 frames
    constexpr int TG = kFrames / V;
    const int n = KP * TG;
    for (int q0 = tid; q0 < n; q0 += kBatch * kThreads) {
      Vec<S> g[kBatch];
#pragma unroll
      for (int j = 0; j < kBatch; ++j) {
        const int q = q0 + j * kThreads, m = q / TG;
        const int64_t t = t0 + (q - m * TG) * V;
        g[j] = Vec<S>{};
        if (q < n && m < a.K && t < a.T) {
          const S* p = base + (int64_t)m * a.sm;
          load_group(p, aligned16(p + t), t, a.T, g[j]);
        }
      }
#pragma unroll
      for (int j = 0; j < kBatch; ++j) {
        const int q = q0 + j * kThreads, m = q / TG, fr0 = (q - m * TG) * V;
        if (q >= n) continue;
#pragma unroll
        for (int k = 0; k < V; ++k)
          yfrag[frag_index(m, fr0 + k)] = m < a.K && t0 + fr0 + k < a.T ? prologue(E::load(g[j].e[k]), a.log_input) : 0.0f;
      }
    }
  }
}

// Tile f0 / kBins of P into LDS: the host stores P tile by tile in fragment order (_host.inverse_mel_fragments: rows beyond F
// and mels beyond K are zeros there), so a tile is kBins * K4 consecutive floats: coalesced 16-byte loads, 16-byte LDS writes.
AAMD_HD void stage_p(int tid, const Args& a, int f0, float* pfrag) {
  const int n = k_pad(a.K) * (kBins / 4);
  const F4* src = reinterpret_cast<const F4*>(a.P) + (int64_t)(f0 / kBins) * n;
  F4* dst = reinterpret_cast<F4*>(pfrag);
  for (int q0 = tid; q0 < n; q0 += kBatch * kThreads) {
    F4 v[kBatch];
#pragma unroll
    for (int j = 0; j < kBatch; ++j) {
      const int q = q0 + j * kThreads;
      v[j] = F4{0.0f, 0.0f, 0.0f, 0.0f};
      if (q < n) v[j] = src[q];
    }
#pragma unroll
    for (int j = 0; j < kBatch; ++j) {
      const int q = q0 + j * kThreads;
      if (q < n) dst[q] = v[j];
    }
  }
}

// One lane's share of its wave's 16 frames x (NFT * 16) bins: bins 4 (lane / 16) .. + 3 of every 16, frame lane % 16.
template <int NFT>
AAMD_HD void mma_lane(int wave, int lane, int KP, const float* yfrag, const float* pfrag, float* otile) {
  float* o = otile + (wave * kSub + (lane & 15)) * kOutPitch + 4 * (lane >> 4);
#if defined(__HIP_DEVICE_COMPILE__)
  using f32x4 = __attribute__((ext_vector_type(4))) float;
  f32x4 acc[NFT];
#pragma unroll
  for (int ft = 0; ft < NFT; ++ft) acc[ft] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  const float* yb = yfrag + wave * 64 + lane;
  const float* pb = pfrag + lane;
  // the operands of step ks + 1 are read from LDS before the products of step ks are issued
  float b = yb[0], av[NFT];
#pragma unroll
  for (int ft = 0; ft < NFT; ++ft) av[ft] = pb[ft * 64];
  for (int ks = 1; ks < (KP >> 2); ++ks) {
    const float bn = yb[ks * 256];
    float an[NFT];
#pragma unroll
    for (int ft = 0; ft < NFT; ++ft) an[ft] = pb[ks * 256 + ft * 64];
#pragma unroll
    for (int ft = 0; ft < NFT; ++ft) {
      acc[ft] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ft], b, acc[ft], 0, 0, 0);
      av[ft] = an[ft];
    }
    b = bn;
  }
#pragma unroll
  for (int ft = 0; ft < NFT; ++ft) acc[ft] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ft], b, acc[ft], 0, 0, 0);
#pragma unroll
  for (int ft = 0; ft < NFT; ++ft)
    *reinterpret_cast<F4*>(o + ft * kSub) = F4{acc[ft][0], acc[ft][1], acc[ft][2], acc[ft][3]};
#else
  // the instruction's arithmetic, lane by lane: D[i][j] takes A[i][k] B[k][j] in ascending k as fused multiply-adds
  for (int ft = 0; ft < NFT; ++ft)
    for (int r = 0; r < 4; ++r) {
      float acc = 0.0f;
      for (int m = 0; m < KP; ++m) acc = fmaf(pfrag[frag_index(m, ft * kSub + 4 * (lane >> 4) + r)],
                                              yfrag[frag_index(m, wave * kSub + (lane & 15))], acc);
      o[ft * kSub + r] = acc;
    }
#endif
}

AAMD_HD void mma_thread(int tid, const Args& a, int f0, const float* yfrag, const float* pfrag, float* otile) {
  const int wave = tid >> 6, lane = tid & 63, KP = k_pad(a.K);
  const int left = a.F - f0;
  if (left > 3 * kSub) mma_lane<4>(wave, lane, KP, yfrag, pfrag, otile);
  else if (left > 2 * kSub) mma_lane<3>(wave, lane, KP, yfrag, pfrag, otile);
  else if (left > kSub) mma_lane<2>(wave, lane, KP, yfrag, pfrag, otile);
  else mma_lane<1>(wave, lane, KP, yfrag, pfrag, otile);
}

AAMD_HD float relu(float v) { return v < 0.0f ? 0.0f : v; }   // a NaN stays a NaN

// The output tile to memory: a wave instruction writes up to 64 consecutive bins of one frame.
template <int DT>
AAMD_HD void store_tile(int tid, const Args& a, int64_t row, int64_t t0, int f0, const float* otile) {
  using E = Elem<DT>;
  using S = typename E::S;
  const int j = tid & (kBins - 1), f = f0 + j;
  if (f >= a.F) return;
  for (int fr = tid >> 6; fr < kFrames; fr += kThreads / kBins) {
    const int64_t t = t0 + fr;
    if (t >= a.T) break;
    static_cast<S*>(a.out)[(row * a.T + t) * a.F + f] = E::store(relu(otile[fr * kOutPitch + j]));
  }
}

#if defined(__HIPCC__)
template <int DT>
__global__ void __launch_bounds__(kThreads) inverse_mel_kernel(Args a, int64_t tiles) {
  extern __shared__ __attribute__((aligned(16))) float iml_smem[];
  const int KP = k_pad(a.K);
  float* yfrag = iml_smem;
  float* pfrag = yfrag + kFrames * KP;
  float* otile = pfrag + kBins * KP;
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x / tiles, t0 = (blockIdx.x - row * tiles) * kFrames;
  stage_y<DT>(tid, a, row, t0, yfrag);
  for (int f0 = 0; f0 < a.F; f0 += kBins) {
    // (the tile before this one: its operand reads ended at the barrier behind its products, and no wave passes the next
    // barrier before every wave has stored its share of the output tile)
    stage_p(tid, a, f0, pfrag);
    __syncthreads();
    mma_thread(tid, a, f0, yfrag, pfrag, otile);
    __syncthreads();
    store_tile<DT>(tid, a, row, t0, f0, otile);
  }
}
#endif  // __HIPCC__

}  // namespace iml
}  // namespace aamd
