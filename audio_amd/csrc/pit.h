// Permutation-invariant training (F.permutation_invariant_training, F.pit_metric_matrix, F.pit_assignment, F.pit_permutate):
// the S x S scores of every estimate against every reference of an example for SI-SDR / SI-SNR / SNR, the best assignment
// and its gradient, all on the device, without atomics and without a host read-back.  The row arithmetic is csrc/sdr.h's
// (stats_of, alpha_of, grad_coef, store_once); all sums are float64 for every input dtype; samples are read as stored
// through the strides and widened on load; nothing at or beyond an example's length is read.
//   gram_kernel           one workgroup per (example, 4096 samples).  The 16 rows of an example -- preds in rows 0 .. S-1, targets
//                         in rows 8 .. 8+S-1, absent rows zero -- are staged 256 samples at a time as float64, sample-major:
//                         K-step s (4 samples) is the 64 doubles x[66 s + 16 (n & 3) + row], so lane l of a wave reads
//                         row l % 16 of sample l / 16 with one contiguous read and the SAME register is the A and the B operand
//                         of v_mfma_f64_16x16x4_f64: G += X X^T.  The 2 doubles of padding per K-step spread the staging
//                         writes (one lane per 16-byte group of a row) over the banks.  The next piece's 16-byte loads are
//                         in flight while the waves multiply: wave w owns K-steps 16 w .. 16 w + 15 of a piece on four
//                         independent accumulator tiles, summed (0 + 1) + (2 + 3), then ((w0 + w1) + w2) + w3 through LDS.
//                         With zero_mean the rows are shifted by the mean of their first 256 samples; the plain row sums and
//                         the per-row non-finite flags are taken on the vector unit while staging, in a fixed tree.  The
//                         partial is the S x S preds-targets block, the diagonal, 16 row sums, 16 flags, 16 shifts: 128 doubles.
//   pair_stats_kernel     one wave per example, one lane per pair: folds the partials in ascending span order and forms what
//                         sdr::stats_of / alpha_of form, into (B, S, S, 8) of sdr::kStat's layout.
//   pair_residual_kernel  one workgroup per (example, 4096 samples): sum of (alpha_ij (t_j - ct_j) - (p_i - cp_i))^2 for all S^2
//                         pairs, summed directly (sdr.h says why).  A wave owns S / 4 pred rows (at least one) and all S target
//                         rows: at most 16 accumulators a lane, reduced by a butterfly over the wave, no LDS and no barrier.
//                         For S <= 2 the spare waves take the other halves / quarters of the chunk, so a partial covers
//                         res_sub(S) samples.  Each of the 2 S rows comes from HBM once; the target rows are re-read by the
//                         workgroup's other waves from the caches.
//   assign_kernel         one workgroup of 256 lanes per example: folds the residual partials in ascending order, forms the
//                         scores (rounded to the output type, so the search sees what the caller sees) in LDS, then a subset
//                         DP with one lane per subset of targets, F[mask] = best over j in mask, ascending, of
//                         M[k][j] + F[mask ^ (1 << j)] with k = S - |mask|: S steps, a barrier each.  The reconstruction walks
//                         forward from estimate 0 and takes the smallest j whose M[k][j] + F[rest] equals F[mask]: the same
//                         expression, compared exactly.  A NaN in the matrix gives a NaN metric and the identity.
//   pit_grad_kernel       one launch: workgroup (example, i, 4096 samples) writes grad_preds[b, i] and grad_target[b, pi(i)]
//                         from p_i and t_pi(i) with sdr::grad_coef's coefficients of the chosen pair and cotangent / S.
//   gather_kernel         F.pit_permutate: out[b, i] = src[b, perm[b, i]], 16-byte accesses, perm read here; an index outside
//                         [0, S) is not used as one: the row is filled with the caller's pattern (NaN for floating types).
// Spans, chunks and pieces are anchored at a row's first sample and depend on nothing but the index and S, so example b of a
// batch equals the call on example b and an example with lengths[b] equals the call on [..., :lengths[b]], bit for bit.
#pragma once
#include "sdr.h"

namespace aamd {
namespace pit {

using wa::Elem;
using wa::Vec;

constexpr int kThreads = 256;
constexpr int kMaxS = 8;                  // PIT_MAX_SOURCES: 2^8 subsets = one lane each
constexpr int kRows = 16;                 // rows of the Gram tile: preds 0 .. 7, targets 8 .. 15
constexpr int kPiece = 256;               // samples staged at a time: 64 K-steps, 16 a wave
constexpr int kGramSpan = 16 * kPiece;    // samples per workgroup of gram_kernel
constexpr int kStepPitch = 64 + 2;        // doubles from one K-step's operand to the next in LDS
constexpr int kAcc = 4;                   // independent accumulator tiles of a wave
constexpr int kTilePitch = 17;
constexpr int kPart = 128;                // doubles of a Gram partial: [64] p_i . t_j at 8 i + j, [16] diagonal, [16] sums, [16] flags, [16] shifts
constexpr int kResChunk = 4096;           // samples per workgroup of pair_residual_kernel
constexpr int kGatherVecs = 4;            // 16-byte groups a thread of gather_kernel moves

struct Args {
  const void *p, *t;            // preds, target: (B, S, T), unit sample stride, strides in elements
  const void* lengths;          // [B] int32 / int64, or null
  int64_t B, T, pb, ps, tb, ts;
  int64_t gspans, rparts, chunks, gchunks;   // Gram partials, residual partials, residual workgroups, gradient workgroups per row
  int32_t S, len64, zero_mean, mode, minimize;
  double eps;
  double* gram;                 // (B, gspans, kPart)
  double* pstat;                // (B, S, S, sdr::kStat)
  double* res;                  // (B, rparts, 64): pair (i, j) at 8 i + j
  const void* min;              // (B, S, S) ready matrix of the output type, or null: the fused route
  void *mout, *best;            // (B, S, S) and (B) of the output type; either may be null
  int64_t* perm;                // (B, S), or null
  double* stat;                 // (B, S, sdr::kStat) of the chosen pairs, or null
  const int64_t* perm_in;       // backward
  const double* cot;            // (B)
  void *gp, *gt;                // dense (B, S, T); either may be null
};

struct GatherArgs {
  const void* src;              // (B, S, R) through sb / ss, unit stride along R
  const int64_t* perm;          // (B, S)
  void* out;                    // dense (B, S, R)
  int64_t B, S, R, sb, ss, chunks;
  uint64_t fill;                // the element written for an index outside [0, S)
};

// what sdr.h's row helpers read of their Args
AAMD_HD sdr::Args metric_of(const Args& a) {
  sdr::Args m{};
  m.lengths = a.lengths; m.len64 = a.len64; m.T = a.T;
  m.zero_mean = a.zero_mean; m.mode = a.mode; m.eps = a.eps;
  return m;
}

// instantiation of pair_residual_kernel that serves S sources, and the samples one of its partials covers
AAMD_HD int res_bucket(int S) { return S <= 2 ? S : (S <= 4 ? 4 : 8); }
AAMD_HD int res_sub(int S) { return S <= 1 ? kResChunk / 4 : (S == 2 ? kResChunk / 2 : kResChunk); }

#if defined(__HIPCC__)
using sdr::d4;

template <int DT>
__device__ __forceinline__ const typename Elem<DT>::S* row_of(const Args& a, int64_t b, int tr) {      // tile row tr
  using S = typename Elem<DT>::S;
  return tr < 8 ? static_cast<const S*>(a.p) + b * a.pb + (int64_t)tr * a.ps
                : static_cast<const S*>(a.t) + b * a.tb + (int64_t)(tr - 8) * a.ts;
}

template <int DT>
__global__ __launch_bounds__(kThreads) void gram_kernel(Args a) {
  using E = Elem<DT>;
  using S = typename E::S;
  constexpr int V = 16 / sizeof(S);
  constexpr int kLpr = kThreads / kRows;       // lanes that stage one row
  constexpr int kIt = kPiece / (kLpr * V);     // 16-byte groups of a piece a lane stages
  constexpr int kStage = (kPiece / 4) * kStepPitch;
  static_assert(4 * 16 * kTilePitch + kThreads <= kStage, "the epilogue reuses the staging area");
  __shared__ __align__(16) double x[kStage];
  __shared__ int bad[kRows];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t b = (int64_t)blockIdx.x / a.gspans, span = (int64_t)blockIdx.x - b * a.gspans;
  const sdr::Args m = metric_of(a);
  const int64_t L = sdr::row_length(m, b);
  const int64_t n_begin = span * kGramSpan;
  if (L <= 0 || n_begin >= L) return;                                   // uniform; such a partial is never folded
  const int64_t n_end = n_begin + kGramSpan < L ? n_begin + kGramSpan : L;
  const int npieces = (int)((n_end - n_begin + kPiece - 1) / kPiece);
  const int tr = tid / kLpr, g0 = tid % kLpr;                           // this lane's tile row, and its place among the row's lanes
  const bool present = (tr & 7) < a.S;
  const S* row = present ? row_of<DT>(a, b, tr) : nullptr;
  const bool vec = wa::aligned16(row);

  for (int j = tid; j < kStage; j += kThreads) x[j] = 0.0;              // absent rows stay zero
  if (tid < kRows) bad[tid] = 0;
  __syncthreads();

  Vec<S> buf[kIt];
  // what zero_mean's sums are taken about: the mean of the row's first piece, the same bits in every workgroup of the example.
  // (The first sample alone, sdr::shift_of's choice, leaves N d_p d_t in the co-moment of two uncorrelated rows, hundreds of
  // times what remains of it: every wrong pair of a mixture is such a pair.)
  double sh = 0.0;
  if (a.zero_mean && present) {
    const int64_t head = L < kPiece ? L : kPiece;
#pragma unroll
    for (int it = 0; it < kIt; ++it) {
      wa::load_group(row, vec, (int64_t)(it * kLpr + g0) * V, head, buf[it]);
#pragma unroll
      for (int k = 0; k < V; ++k) sh += (double)E::load(buf[it].e[k]);          // zero bits at or beyond head
    }
#pragma unroll
    for (int msk = kLpr >> 1; msk > 0; msk >>= 1) sh += __shfl_xor(sh, msk, 64); // the row's 16 lanes: every lane gets the same bits
    sh /= (double)head;
  }
  double rs = 0.0;
  int badl = 0;
  d4 acc[kAcc];
#pragma unroll
  for (int k = 0; k < kAcc; ++k) acc[k] = d4{0.0, 0.0, 0.0, 0.0};

  auto fetch = [&](int w) {
    if (!present) return;
#pragma unroll
    for (int it = 0; it < kIt; ++it)                                    // nothing at or beyond L is read
      wa::load_group(row, vec, n_begin + (int64_t)w * kPiece + (it * kLpr + g0) * V, L, buf[it]);
  };

  fetch(0);
  for (int w = 0; w < npieces; ++w) {
    const int64_t n0 = n_begin + (int64_t)w * kPiece;
    if (w > 0) __syncthreads();                                         // the last piece's operands have been read
    if (present) {
#pragma unroll
      for (int it = 0; it < kIt; ++it) {
#pragma unroll
        for (int k = 0; k < V; ++k) {
          const int kk = (it * kLpr + g0) * V + k;
          const bool in = n0 + kk < L;
          double v = (double)E::load(buf[it].e[k]);
          badl |= in && !sdr::finite(v);
          v = in ? v - sh : 0.0;
          rs += v;
          x[(kk >> 2) * kStepPitch + (kk & 3) * 16 + tr] = v;
        }
      }
    }
    __syncthreads();
    if (w + 1 < npieces) fetch(w + 1);
    const int64_t live = L - n0 < kPiece ? L - n0 : kPiece;             // K-steps past it multiply zeros
    const int steps = (int)((live + 3) >> 2);
#pragma unroll
    for (int i = 0; i < 16 / kAcc; ++i) {
#pragma unroll
      for (int k = 0; k < kAcc; ++k) {
        const int st = wave * 16 + i * kAcc + k;
        if (st < steps) {                                               // uniform over the wave
          const double xv = x[st * kStepPitch + lane];
          acc[k] = __builtin_amdgcn_mfma_f64_16x16x4f64(xv, xv, acc[k], 0, 0, 0);
        }
      }
    }
  }

  // epilogue: D[i][j] of a tile sits in lane 16 (i & 3) + j, register i >> 2
  __syncthreads();
  const d4 sum = (acc[0] + acc[1]) + (acc[2] + acc[3]);
  double* tile = x + wave * 16 * kTilePitch;
  double* red = x + 4 * 16 * kTilePitch;
#pragma unroll
  for (int v = 0; v < 4; ++v) tile[(4 * v + (lane >> 4)) * kTilePitch + (lane & 15)] = sum[v];
  red[tid] = rs;
  if (badl) bad[tr] = 1;                                                // every writer stores the same value
  if (g0 == 0) a.gram[(b * a.gspans + span) * kPart + 112 + tr] = sh;
  __syncthreads();
  for (int stride = kLpr >> 1; stride > 0; stride >>= 1) {              // a row's lanes, fixed order
    if (g0 < stride) red[tid] += red[tid + stride];
    __syncthreads();
  }
  double* out = a.gram + (b * a.gspans + span) * kPart;
  const int i = tid >> 4, j = tid & 15, e = i * kTilePitch + j;
  const double gij = ((x[e] + x[16 * kTilePitch + e]) + x[2 * 16 * kTilePitch + e]) + x[3 * 16 * kTilePitch + e];
  if (i < 8 && j >= 8) out[i * 8 + (j - 8)] = gij;
  if (i == j) out[64 + i] = gij;
  if (tid < kRows) {
    out[80 + tid] = red[tid * kLpr];
    out[96 + tid] = bad[tid] ? 1.0 : 0.0;
  }
}

template <int DT>
__global__ __launch_bounds__(sdr::kSolveThreads) void pair_stats_kernel(Args a) {
  const int lane = threadIdx.x, S = a.S;
  const int64_t b = blockIdx.x;
  if (lane >= S * S) return;
  const int i = lane / S, j = lane - i * S;
  const sdr::Args m = metric_of(a);
  const int64_t L = sdr::row_length(m, b);
  double shp = 0.0, sht = 0.0;
  if (a.zero_mean && L > 0) {                                           // what gram_kernel shifted the rows by
    shp = a.gram[b * a.gspans * kPart + 112 + i];
    sht = a.gram[b * a.gspans * kPart + 120 + j];
  }
  const int64_t nsp = L > 0 ? sdr::ceil_div(L, kGramSpan) : 0;
  double sh[sdr::kMom] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t sp = 0; sp < nsp && sp < a.gspans; ++sp) {
    const double* gp = a.gram + (b * a.gspans + sp) * kPart;
    sh[0] += gp[80 + i]; sh[1] += gp[88 + j];
    sh[2] += gp[64 + i]; sh[3] += gp[72 + j];
    sh[4] += gp[8 * i + j];
    sh[5] += gp[96 + i] + gp[104 + j];
  }
  const sdr::Stats s = sdr::stats_of(m, L, sh, shp, sht);
  double* st = a.pstat + ((b * S + i) * S + j) * sdr::kStat;
  st[0] = s.N; st[1] = s.cp; st[2] = s.ct; st[3] = s.Stt; st[4] = s.Spt; st[5] = sdr::alpha_of(m, s); st[6] = 0.0;
  st[7] = s.bad ? 1.0 : 0.0;
}

template <int DT, int NS>
__global__ __launch_bounds__(kThreads) void pair_residual_kernel(Args a) {
  using E = Elem<DT>;
  using S = typename E::S;
  constexpr int V = 16 / sizeof(S);
  constexpr int kPw = NS >= 4 ? NS / 4 : 1;          // pred rows of a wave
  constexpr int kWps = NS / kPw;                     // waves that share a run of samples
  constexpr int kSubs = 4 / kWps;                    // runs of a chunk
  constexpr int kSub = kResChunk / kSubs;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, ns = a.S;
  const int64_t b = (int64_t)blockIdx.x / a.chunks, chunk = (int64_t)blockIdx.x - b * a.chunks;
  const sdr::Args m = metric_of(a);
  const int64_t L = sdr::row_length(m, b);
  const int ip = (wave % kWps) * kPw;
  const int64_t part = chunk * kSubs + wave / kWps, begin = part * kSub;
  if (L <= 0 || begin >= L || ip >= ns) return;                         // uniform over the wave; such a partial is never folded
  const int64_t end = begin + kSub < L ? begin + kSub : L;

  double al[kPw][NS], cp[kPw], ct[NS], acc[kPw][NS];
  const S *pr[kPw], *tr[NS];
  bool vp[kPw], vt[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) { ct[j] = 0.0; tr[j] = nullptr; vt[j] = false; }
#pragma unroll
  for (int ii = 0; ii < kPw; ++ii) {
    cp[ii] = 0.0; pr[ii] = nullptr; vp[ii] = false;
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      al[ii][j] = acc[ii][j] = 0.0;
      if (ip + ii < ns && j < ns) {
        const double* st = a.pstat + ((b * ns + ip + ii) * ns + j) * sdr::kStat;
        cp[ii] = st[1]; ct[j] = st[2]; al[ii][j] = st[5];
        pr[ii] = row_of<DT>(a, b, ip + ii); vp[ii] = wa::aligned16(pr[ii]);
        tr[j] = row_of<DT>(a, b, 8 + j); vt[j] = wa::aligned16(tr[j]);
      }
    }
  }
#pragma unroll 2
  for (int64_t n = begin + lane * V; n < end; n += 64 * V) {
    Vec<S> xp[kPw], xt[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j)
      if (j < ns) wa::load_group(tr[j], vt[j], n, end, xt[j]);
#pragma unroll
    for (int ii = 0; ii < kPw; ++ii)
      if (ip + ii < ns) wa::load_group(pr[ii], vp[ii], n, end, xp[ii]);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      if (n + k < end) {
        double tc[NS];
#pragma unroll
        for (int j = 0; j < NS; ++j) tc[j] = j < ns ? (double)E::load(xt[j].e[k]) - ct[j] : 0.0;
#pragma unroll
        for (int ii = 0; ii < kPw; ++ii) {
          if (ip + ii < ns) {
            const double pc = (double)E::load(xp[ii].e[k]) - cp[ii];
#pragma unroll
            for (int j = 0; j < NS; ++j) {
              if (j < ns) {
                const double e = al[ii][j] * tc[j] - pc;
                acc[ii][j] += e * e;
              }
            }
          }
        }
      }
    }
  }
  double* out = a.res + (b * a.rparts + part) * 64;
#pragma unroll
  for (int ii = 0; ii < kPw; ++ii) {
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      if (ip + ii < ns && j < ns) {                                     // uniform
        const double r = sdr::wave_sum(acc[ii][j]);
        if (lane == 0) out[8 * (ip + ii) + j] = r;
      }
    }
  }
}

// C: float or double, the type of the matrix and of best_metric
template <typename C>
__global__ __launch_bounds__(kThreads) void assign_kernel(Args a) {
  __shared__ double M[64], F[1 << kMaxS];
  __shared__ int has_nan, sel[kMaxS];
  const int tid = threadIdx.x, S = a.S, full = (1 << S) - 1;
  const int64_t b = blockIdx.x;
  if (tid == 0) { has_nan = 0; F[0] = 0.0; }
  __syncthreads();
  if (tid < 64) {
    const int i = tid >> 3, j = tid & 7;
    double v = 0.0;
    if (i < S && j < S) {
      const int64_t e = (b * S + i) * S + j;
      if (a.min) {
        v = (double)static_cast<const C*>(a.min)[e];
      } else {
        const sdr::Args m = metric_of(a);
        const int64_t L = sdr::row_length(m, b);
        const int64_t nparts = L > 0 ? sdr::ceil_div(L, res_sub(S)) : 0;
        double r = 0.0;
        for (int64_t c = 0; c < nparts && c < a.rparts; ++c) r += a.res[(b * a.rparts + c) * 64 + tid];
        double* st = a.pstat + e * sdr::kStat;
        st[6] = r;
        const double sig = st[5] * st[5] * st[3] + a.eps, noise = r + a.eps;
        v = (double)(C)(st[7] != 0.0 ? NAN : 10.0 * log10(sig / noise));
      }
      if (a.mout) static_cast<C*>(a.mout)[e] = (C)v;
      if (v != v) has_nan = 1;                                          // every writer stores the same value
    }
    M[tid] = v;
  }
  __syncthreads();
  const int bits = __popc(tid);
  for (int k = S - 1; k >= 0; --k) {
    if (tid <= full && bits == S - k) {
      bool first = true;
      double best = 0.0;
      for (int j = 0; j < S; ++j) {
        if ((tid >> j) & 1) {
          const double v = M[8 * k + j] + F[tid ^ (1 << j)];
          if (first || (a.minimize ? v < best : v > best)) { best = v; first = false; }
        }
      }
      F[tid] = best;
    }
    __syncthreads();
  }
  if (tid == 0) {
    const bool nan = has_nan != 0;
    int mask = full;
    for (int k = 0; k < S; ++k) {
      int pick = k;
      if (!nan) {
        pick = -1;
        for (int j = 0; j < S && pick < 0; ++j)
          if (((mask >> j) & 1) && M[8 * k + j] + F[mask ^ (1 << j)] == F[mask]) pick = j;
        if (pick < 0) pick = __ffs(mask) - 1;                           // a NaN total (inf - inf): still a permutation
        mask ^= 1 << pick;
      }
      sel[k] = pick;
      if (a.perm) a.perm[b * S + k] = pick;
    }
    if (a.best) static_cast<C*>(a.best)[b] = (C)(nan ? NAN : F[full] / (double)S);
  }
  __syncthreads();
  if (a.stat && tid < 8 * S) {
    const int k = tid >> 3, e = tid & 7;
    a.stat[(b * S + k) * sdr::kStat + e] = a.pstat[((b * S + k) * S + sel[k]) * sdr::kStat + e];
  }
}

template <int DT>
__global__ __launch_bounds__(kThreads) void pit_grad_kernel(Args a) {
  using E = Elem<DT>;
  using S = typename E::S;
  constexpr int V = 16 / sizeof(S);
  const int tid = threadIdx.x, ns = a.S;
  const int64_t row = (int64_t)blockIdx.x / a.gchunks, chunk = (int64_t)blockIdx.x - row * a.gchunks;
  const int64_t b = row / ns;
  const int i = (int)(row - b * ns);
  const int64_t pi_raw = a.perm_in[row];
  const int pi = (uint64_t)pi_raw < (uint64_t)ns ? (int)pi_raw : i;      // never indexed with a value outside [0, S)
  const sdr::Args m = metric_of(a);
  int64_t L = sdr::row_length(m, b);
  if (L < 0) L = 0;
  double c[6];
  sdr::grad_coef(m, a.stat + row * sdr::kStat, a.cot[b] / (double)ns, c);
  const int64_t cend = (chunk + 1) * sdr::kChunk < a.T ? (chunk + 1) * sdr::kChunk : a.T;
  const int64_t end = cend < L ? cend : L;                              // samples below it are read
  const S* p = row_of<DT>(a, b, i);
  const S* t = row_of<DT>(a, b, 8 + pi);
  S* gp = a.gp ? static_cast<S*>(a.gp) + row * a.T : nullptr;
  S* gt = a.gt ? static_cast<S*>(a.gt) + (b * ns + pi) * a.T : nullptr;
  const bool vp = wa::aligned16(p), vt = wa::aligned16(t), vgp = wa::aligned16(gp), vgt = wa::aligned16(gt);
#pragma unroll
  for (int g = 0; g < sdr::kChunk / (kThreads * V); ++g) {
    const int64_t i0 = chunk * sdr::kChunk + (int64_t)(g * kThreads + tid) * V;
    if (i0 >= cend) continue;
    Vec<S> xp, xt, op, ot;
    wa::load_group(p, vp, i0, end, xp);
    wa::load_group(t, vt, i0, end, xt);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const bool in = i0 + k < end;
      const double pv = (double)E::load(xp.e[k]), tv = (double)E::load(xt.e[k]);
      op.e[k] = in ? sdr::store_once<DT>(c[0] * pv + c[1] * tv + c[2]) : S(0);
      ot.e[k] = in ? sdr::store_once<DT>(c[3] * pv + c[4] * tv + c[5]) : S(0);
    }
    if (gp) wa::store_group(gp, vgp, i0, cend, op);
    if (gt) wa::store_group(gt, vgt, i0, cend, ot);
  }
}

// U: an unsigned integer of the element's size
template <typename U>
__global__ __launch_bounds__(kThreads) void gather_kernel(GatherArgs a) {
  constexpr int V = 16 / sizeof(U);
  const int tid = threadIdx.x;
  const int64_t row = (int64_t)blockIdx.x / a.chunks, chunk = (int64_t)blockIdx.x - row * a.chunks;
  const int64_t b = row / a.S;
  const int64_t from = a.perm[row];
  const bool valid = (uint64_t)from < (uint64_t)a.S;
  const U* src = static_cast<const U*>(a.src) + b * a.sb + (valid ? from : 0) * a.ss;
  U* dst = static_cast<U*>(a.out) + row * a.R;
  const bool vs = wa::aligned16(src), vd = wa::aligned16(dst);
#pragma unroll
  for (int g = 0; g < kGatherVecs; ++g) {
    const int64_t i0 = (chunk * kGatherVecs + g) * (int64_t)(kThreads * V) + (int64_t)tid * V;
    if (i0 >= a.R) continue;
    Vec<U> v;
    if (valid) {
      wa::load_group(src, vs, i0, a.R, v);
    } else {
#pragma unroll
      for (int k = 0; k < V; ++k) v.e[k] = (U)a.fill;
    }
    wa::store_group(dst, vd, i0, a.R, v);
  }
}
#endif

}  // namespace pit
}  // namespace aamd
