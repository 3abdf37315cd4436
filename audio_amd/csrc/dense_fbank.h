// Dense filterbank projection (F.dense_fbank_scale / T.ChromaScale): out[v][n] = sum_k x[v][k] W[k][n] over all frames v of all
// rows, W an (n_freqs, n_out) filterbank with few outputs (a chromagram has 12) and a long contraction axis (n_freqs = 201 ..
// 4097) in which almost every entry is non-zero: the banded mel kernels have no band to walk here.  One launch.
//
// Arithmetic.  v_mfma_f32_16x16x4_f32: exact float32 FMA chains.  A = a tile of W^T (16 outputs x 4 bins), B = a tile of x^T
// (4 bins x 16 frames), so D holds 16 outputs x 16 frames and a lane ends with 4 consecutive outputs of one frame: what the
// frame-major store wants.  Every output has ONE accumulator that starts at zero, stays in registers across all K tiles and
// takes its products in ascending k (the instruction adds its 4 products in ascending k, the steps follow in ascending k): the
// result does not depend on the tile a frame falls in, on the number of rows, on the input's layout or alignment, or on kTileK.
// Bins beyond n_freqs up to the next multiple of 4 are zeros on both sides; outputs beyond n_out are zero columns of W whose
// results are not stored.
//
// Tile plan.  A workgroup of 4 waves owns kFrames = 64 consecutive frames of ONE row (wave w: frames 16 w .. 16 w + 15) and
// walks n_freqs in tiles of kTileK = 64 bins:
//   fetch     the NEXT tile's global loads into registers: the frames' bins, read in place through the strides (4 or 2
//             16-byte groups per thread), and the tile of W (the host lays W out in the A operand's order, so a tile is a
//             run of consecutive floats; up to 8 16-byte groups per thread at 128 outputs, 1 at 12);
//   mma       the CURRENT tile from LDS: per step of 4 bins one B read and, per 16 outputs, one A read and one MFMA (up to
//             8 independent accumulators per wave); the loads of `fetch` are in flight meanwhile;
//   commit    after a barrier, the fetched registers to LDS (widened: float16 / bfloat16), in the order the operands are read.
// One LDS buffer, two barriers a tile; the memory round trip hides behind the products.  The kernel is bound by the one read
// of x (24 flops per 4 bytes at 12 outputs).
// Operand order in LDS ("fragment order", inverse_mel.h's): element (k, j) of the x tile -- j the frame -- sits at
//   ((k / 4) * 4 + j / 16) * 64 + (k % 4) * 16 + j % 16,
// element (k, n) of W at ((k / 4) * NT + n / 16) * 64 + (k % 4) * 16 + n % 16 with NT = ceil(n_out / 16): the 64 lanes of
// an operand read are 64 consecutive floats.
// LDS: (64 * 64 + 64 * 16 * NT) * 4 bytes: 20 KB up to 16 outputs, 48 KB at the limit of 128; the registers, not the LDS, set
// the workgroups a CU (5 up to 32 outputs, 3 beyond: DESIGN 4.25).
//
// Input layouts (Args::time_major).  0: unit stride along freq, `st` elements between frames (the frame-major view every
// Spectrogram here returns); a lane loads 16 bytes along freq.  1: unit stride along time, `sk` elements between bins (a
// contiguous (B, n_freqs, T)); a lane loads 16 bytes along time.  A float32 group is one access at any element offset; a
// half-type group that does not start on a 16-byte boundary, and any group that crosses the end of its row, is loaded element
// by element: the same values, so the same bits (load_x).
//
// The phase functions are AAMD_HD: tests/cpu_sim/sim_dense_fbank.cpp replays them with g++ (fmaf for the MFMA chain).
#pragma once
#include <math.h>

#include "wave_augment.h"

namespace aamd {
namespace dfb {

using wa::Elem;
using wa::Vec;
using wa::aligned16;
using wa::load_group;

constexpr int kThreads = 256;
constexpr int kFrames = 64;               // frames of one row per workgroup
constexpr int kTileK = 64;                // bins of n_freqs per LDS tile
constexpr int kSub = 16;                  // the MFMA's tile edge
constexpr int kMaxN = 128;                // outputs
constexpr int kMaxK = 4097;               // bins: n_fft = 8192, the package's limit
constexpr int kMaxNT = kMaxN / kSub;      // accumulators per wave
constexpr int kSmallNT = 2;               // up to 32 outputs: the kernel that keeps fewer registers (more workgroups a CU)

struct Args {
  const void* x;                // (rows, n_freqs, T) through sr / sk / st
  const float* W;               // K4 / 4 * NT * 64 floats in fragment order, 16-byte aligned
  void* out;                    // dense (rows, T, N)
  int64_t rows, T, sr, sk, st;
  int32_t K, N;                 // n_freqs, n_out
  int32_t time_major;           // 0: sk == 1; 1: st == 1
};

AAMD_HD int k_pad(int K) { return (K + 3) & ~3; }
AAMD_HD int n_tiles(int N) { return (N + kSub - 1) / kSub; }
AAMD_HD int64_t tiles_per_row(int64_t T) { return (T + kFrames - 1) / kFrames; }
AAMD_HD int64_t lds_floats(int N) { return (int64_t)kFrames * kTileK + (int64_t)kTileK * kSub * n_tiles(N); }
AAMD_HD int x_index(int k, int j) { return (((k >> 2) * 4 + (j >> 4)) << 6) + ((k & 3) << 4) + (j & 15); }
AAMD_HD int64_t w_index(int k, int n, int NT) { return (((int64_t)(k >> 2) * NT + (n >> 4)) << 6) + ((k & 3) << 4) + (n & 15); }
// steps of 4 bins in the tile that starts at bin k0
AAMD_HD int tile_steps(int K, int k0) { return (k_pad(K) - k0 < kTileK ? k_pad(K) - k0 : kTileK) >> 2; }

// What a thread holds between `fetch` and `commit`: its share of the next tile, as loaded.
template <typename S, int NT>
struct Fetched {
  static constexpr int kX = kFrames * kTileK * (int)sizeof(S) / (16 * kThreads);   // 4 (float32) or 2
  static constexpr int kW = kTileK / 4 * NT * kSub / kThreads;                     // 16-byte groups of a W tile: NT
  Vec<S> x[kX];
  F4 w[kW];
};

// Elements [i0, i0 + V) of a row of x; those at or beyond `end` come back as zero bits.  float32: one 16-byte access wherever
// the group lies inside the row -- the access needs the element's alignment only, which matters here: rows of 201 or 1025
// float32 start on a 16-byte boundary once in four.  The half types: wa::load_group's rule (16-byte aligned groups in one
// access, the others element by element).  The same values either way, so the same bits.
struct __attribute__((packed, aligned(4))) U4 {
  float e[4];
};
AAMD_HD void load_x(const float* row, int64_t i0, int64_t end, Vec<float>& v) {
  if (i0 + 4 <= end) {
    const U4 u = *reinterpret_cast<const U4*>(row + i0);
#pragma unroll
    for (int k = 0; k < 4; ++k) v.e[k] = u.e[k];
    return;
  }
  for (int k = 0; k < 4; ++k) v.e[k] = i0 + k < end ? row[i0 + k] : 0.0f;
}
AAMD_HD void load_x(const uint16_t* row, int64_t i0, int64_t end, Vec<uint16_t>& v) {
  load_group(row, aligned16(row + i0), i0, end, v);
}

// group q (< kX * kThreads) of the x tile, frame-major input: 16 frames x 4 groups of V bins per wave instruction
template <int V>
AAMD_HD void fm_group(int q, int& fr, int& kk) {
  const int rest = q >> 6;
  fr = (rest & 3) * kSub + (q & 15);
  kk = ((rest >> 2) * 4 + ((q >> 4) & 3)) * V;
}

// The global loads of the tile at bin k0: frames [t0, t0 + kFrames) of `row`, and the tile's share of W.
template <int DT, int NT>
AAMD_HD void fetch(int tid, const Args& a, int64_t row, int64_t t0, int k0, Fetched<typename Elem<DT>::S, NT>& f) {
  using S = typename Elem<DT>::S;
  constexpr int V = 16 / sizeof(S), KX = Fetched<S, NT>::kX, KW = Fetched<S, NT>::kW;
  const S* base = static_cast<const S*>(a.x) + row * a.sr;
  if (!a.time_major) {
#pragma unroll
    for (int j = 0; j < KX; ++j) {
      int fr, kk;
      fm_group<V>(tid + j * kThreads, fr, kk);
      const int64_t t = t0 + fr;
      f.x[j] = Vec<S>{};
      if (k0 + kk < a.K && t < a.T) {
        const S* p = base + t * a.st;
        load_x(p, (int64_t)(k0 + kk), (int64_t)a.K, f.x[j]);
      }
    }
  } else {
    // kFrames / V groups of V frames per bin: a wave instruction reads whole rows of 64 frames
    constexpr int TG = kFrames / V;
#pragma unroll
    for (int j = 0; j < KX; ++j) {
      const int q = tid + j * kThreads, kk = q / TG;
      const int64_t t = t0 + (q - kk * TG) * V;
      f.x[j] = Vec<S>{};
      if (k0 + kk < a.K && t < a.T) {
        const S* p = base + (int64_t)(k0 + kk) * a.sk;
        load_x(p, t, a.T, f.x[j]);
      }
    }
  }
  // W (NT = n_tiles(N)): the host's image is padded to 4 bins and 16 outputs, so a tile is tile_steps * NT * 16 whole groups
  const int n = tile_steps(a.K, k0) * NT * kSub;
  const F4* src = reinterpret_cast<const F4*>(a.W) + (int64_t)(k0 >> 2) * NT * kSub;
#pragma unroll
  for (int j = 0; j < KW; ++j) {
    const int q = tid + j * kThreads;
    f.w[j] = F4{0.0f, 0.0f, 0.0f, 0.0f};
    if (q < n) f.w[j] = src[q];
  }
}

// The fetched tile into LDS in fragment order; frames beyond T and bins beyond K are zeros.
template <int DT, int NT>
AAMD_HD void commit(int tid, const Args& a, int64_t t0, int k0, const Fetched<typename Elem<DT>::S, NT>& f, float* xfrag,
                    float* wfrag) {
  using E = Elem<DT>;
  using S = typename E::S;
  constexpr int V = 16 / sizeof(S), KX = Fetched<S, NT>::kX, KW = Fetched<S, NT>::kW;
  if (!a.time_major) {
#pragma unroll
    for (int j = 0; j < KX; ++j) {
      int fr, kk;
      fm_group<V>(tid + j * kThreads, fr, kk);
      const bool live = t0 + fr < a.T;
#pragma unroll
      for (int e = 0; e < V; ++e)
        xfrag[x_index(kk + e, fr)] = live && k0 + kk + e < a.K ? E::load(f.x[j].e[e]) : 0.0f;
    }
  } else {
    constexpr int TG = kFrames / V;
#pragma unroll
    for (int j = 0; j < KX; ++j) {
      const int q = tid + j * kThreads, kk = q / TG, fr0 = (q - kk * TG) * V;
#pragma unroll
      for (int e = 0; e < V; ++e)
        xfrag[x_index(kk, fr0 + e)] = k0 + kk < a.K && t0 + fr0 + e < a.T ? E::load(f.x[j].e[e]) : 0.0f;
    }
  }
  const int n = tile_steps(a.K, k0) * NT * kSub;
  F4* dst = reinterpret_cast<F4*>(wfrag);
#pragma unroll
  for (int j = 0; j < KW; ++j) {
    const int q = tid + j * kThreads;
    if (q < n) dst[q] = f.w[j];
  }
}

// A lane's accumulators: acc.v[nt][r] is output 16 nt + 4 (lane / 16) + r of frame lane % 16 of its wave.
struct Acc {
  float v[kMaxNT][4];
};

template <int NT>
AAMD_HD void clear(Acc& acc) {
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc.v[nt][r] = 0.0f;
}

// `steps` steps of 4 bins of the tile in LDS onto the lane's accumulators.
template <int NT>
AAMD_HD void mma_lane(int wave, int lane, int steps, const float* xfrag, const float* wfrag, Acc& acc) {
#if defined(__HIP_DEVICE_COMPILE__)
  using f32x4 = __attribute__((ext_vector_type(4))) float;
  f32x4 c[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) c[nt] = f32x4{acc.v[nt][0], acc.v[nt][1], acc.v[nt][2], acc.v[nt][3]};
  const float* xb = xfrag + wave * 64 + lane;
  const float* wb = wfrag + lane;
  // the operands of step ks + 1 are read from LDS before the products of step ks are issued
  float b = xb[0], av[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) av[nt] = wb[nt * 64];
  for (int ks = 1; ks < steps; ++ks) {
    const float bn = xb[ks * 256];
    float an[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) an[nt] = wb[(ks * NT + nt) * 64];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      c[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[nt], b, c[nt], 0, 0, 0);
      av[nt] = an[nt];
    }
    b = bn;
  }
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) c[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[nt], b, c[nt], 0, 0, 0);
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc.v[nt][r] = c[nt][r];
#else
  // the instruction's arithmetic, lane by lane: D[i][j] takes A[i][k] B[k][j] in ascending k as fused multiply-adds
  for (int nt = 0; nt < NT; ++nt)
    for (int r = 0; r < 4; ++r) {
      float c = acc.v[nt][r];
      for (int k = 0; k < 4 * steps; ++k)
        c = fmaf(wfrag[w_index(k, nt * kSub + 4 * (lane >> 4) + r, NT)], xfrag[x_index(k, wave * kSub + (lane & 15))], c);
      acc.v[nt][r] = c;
    }
#endif
}

template <typename S>
struct alignas(4 * sizeof(S)) Quad {
  S e[4];
};

// The lane's outputs to memory, rounded once: 4 consecutive outputs of a frame in one access where the rows of N elements
// keep them aligned (N % 4 == 0: a wave instruction then writes 16 whole frames), one by one otherwise.
template <int DT, int NT>
AAMD_HD void store_lane(int wave, int lane, const Args& a, int64_t row, int64_t t0, const Acc& acc) {
  using E = Elem<DT>;
  using S = typename E::S;
  const int64_t t = t0 + wave * kSub + (lane & 15);
  if (t >= a.T) return;
  S* o = static_cast<S*>(a.out) + (row * a.T + t) * a.N;
  const bool quads = (a.N & 3) == 0;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int n0 = nt * kSub + 4 * (lane >> 4);
    if (quads) {
      if (n0 < a.N)
        *reinterpret_cast<Quad<S>*>(o + n0) =
            Quad<S>{{E::store(acc.v[nt][0]), E::store(acc.v[nt][1]), E::store(acc.v[nt][2]), E::store(acc.v[nt][3])}};
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (n0 + r < a.N) o[n0 + r] = E::store(acc.v[nt][r]);
    }
  }
}

#if defined(__HIPCC__)
template <int DT, int NT>
__device__ __forceinline__ void run_block(const Args& a, int64_t row, int64_t t0, float* xfrag, float* wfrag) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  Fetched<typename Elem<DT>::S, NT> f;
  Acc acc;
  clear<NT>(acc);
  fetch<DT, NT>(tid, a, row, t0, 0, f);
  for (int k0 = 0; k0 < a.K; k0 += kTileK) {
    commit<DT, NT>(tid, a, t0, k0, f, xfrag, wfrag);
    __syncthreads();
    if (k0 + kTileK < a.K) fetch<DT, NT>(tid, a, row, t0, k0 + kTileK, f);
    mma_lane<NT>(wave, lane, tile_steps(a.K, k0), xfrag, wfrag, acc);
    __syncthreads();      // (no wave overwrites the tile before every wave has read it)
  }
  store_lane<DT, NT>(wave, lane, a, row, t0, acc);
}

// SMALL: n_out <= 16 kSmallNT, else the rest up to kMaxN (two kernels, so that few outputs do not pay for the registers of many)
template <int DT, bool SMALL>
__global__ void __launch_bounds__(kThreads) dense_fbank_kernel(Args a, int64_t tiles) {
  extern __shared__ __attribute__((aligned(16))) float dfb_smem[];
  float* xfrag = dfb_smem;
  float* wfrag = xfrag + kFrames * kTileK;
  const int64_t row = blockIdx.x / tiles, t0 = (blockIdx.x - row * tiles) * kFrames;
  if (SMALL) {
    if (n_tiles(a.N) == 1) run_block<DT, 1>(a, row, t0, xfrag, wfrag);
    else run_block<DT, 2>(a, row, t0, xfrag, wfrag);
    return;
  }
  switch (n_tiles(a.N)) {
    case 3: run_block<DT, 3>(a, row, t0, xfrag, wfrag); break;
    case 4: run_block<DT, 4>(a, row, t0, xfrag, wfrag); break;
    case 5: run_block<DT, 5>(a, row, t0, xfrag, wfrag); break;
    case 6: run_block<DT, 6>(a, row, t0, xfrag, wfrag); break;
    case 7: run_block<DT, 7>(a, row, t0, xfrag, wfrag); break;
    default: run_block<DT, 8>(a, row, t0, xfrag, wfrag); break;
  }
}
#endif  // __HIPCC__

}  // namespace dfb
}  // namespace aamd
