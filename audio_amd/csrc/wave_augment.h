// Waveform augmentation (F.add_noise / T.AddNoise, F.preemphasis / T.Preemphasis).
//
// add_noise.  The reference mixes noise into a batch at a requested SNR with about ten element-wise and reduction passes
// and two masked copies.  Here it is two launches with no temporaries:
//   reduce  one workgroup per (row, chunk of kChunk samples): float64 sums of w^2 and n^2 over the samples below the row's
//           length (a float32 square is exact in float64, so an energy depends on the summation order only, and that order
//           is fixed: element -> thread by index, a tree over the threads, the chunks in order), written as partial sums to
//           the caller's workspace.  No floating-point atomics: two calls give the same bits.
//   apply   every workgroup of a row adds the row's partial sums in the same order, so all of them hold the same scale
//               scale = 10 ** ((10 (log10 Es - log10 En) - snr) / 20)
//           evaluated in float64 as written (log10(0) = -inf is not special-cased) and rounded once to the compute type;
//           out = w + scale * n with the product and the sum rounded separately (no contraction), over the WHOLE row.
// The gradient is the same two launches (grad = 1): reduce also sums d = sum g n over the whole row, apply writes
//   grad_w = g + d (s / Es) m w,   grad_n = s g - d (s / En) m n,   grad_snr = -(ln 10 / 20) s d     (m: the length mask).
// `lengths` and `snr` are device arrays read here; nothing synchronises with the host.
//
// preemphasis.  y[i] = x[i] - c x[i-1], y[0] = x[0]; transposed (its adjoint): y[i] = x[i] - c x[i+1], y[L-1] = x[L-1].
// c is rounded to the compute type first, the product and the difference are rounded separately.
//
// Rounding.  The library is built with -ffp-contract=fast, under which the back end fuses a * b + c whatever a pragma in the
// source says, and HIP's __fmul_rn is a plain product.  A product that the reference rounds on its own goes through
// rounded(), an empty asm the optimiser cannot see through; it costs no instruction.
//
// Rows.  Every operand is (rows, L) with unit stride along time and its own row stride in elements: 0 for a broadcast row,
// L + k for rows cut from a wider tensor.  A thread owns the V = 16 / sizeof(element) consecutive samples at a fixed index of
// its chunk, whatever the addresses are; an operand whose row starts on a 16-byte boundary moves them as one 16-byte access,
// any other row sample by sample -- decided per operand and per row, so nothing is copied and the arithmetic (and the
// summation order) does not depend on the alignment.  float16 and bfloat16 are loaded and stored here and computed in
// float32, rounded once.
//
// The phase functions are AAMD_HD: tests/cpu_sim/sim_wave_augment.cpp replays them with g++.
#pragma once
#include "hd.h"
#include "spec_augment.h"   // sa::f16_to_f32 and its kin

namespace aamd {
namespace wa {

constexpr int kThreads = 256;
constexpr int kChunk = 4096;   // samples per workgroup, every dtype
constexpr int kBatch = 4;      // 16-byte vectors per thread whose loads are issued together

enum { kF32 = 0, kF64 = 1, kF16 = 2, kBF16 = 3 };   // = AAMD_SA_*

template <int DT> struct Elem;
template <> struct Elem<kF32> {
  using S = float; using C = float;
  static AAMD_HD C load(S v) { return v; }
  static AAMD_HD S store(C v) { return v; }
};
template <> struct Elem<kF64> {
  using S = double; using C = double;
  static AAMD_HD C load(S v) { return v; }
  static AAMD_HD S store(C v) { return v; }
};
template <> struct Elem<kF16> {
  using S = uint16_t; using C = float;
  static AAMD_HD C load(S v) { return sa::f16_to_f32(v); }
  static AAMD_HD S store(C v) { return sa::f32_to_f16(v); }
};
template <> struct Elem<kBF16> {
  using S = uint16_t; using C = float;
  static AAMD_HD C load(S v) { return sa::bf16_to_f32(v); }
  static AAMD_HD S store(C v) { return sa::f32_to_bf16(v); }
};

template <typename S>
struct alignas(16) Vec {
  S e[16 / sizeof(S)];
};

// v as a value of its own: what is computed from it next is not fused with what computed it
template <typename C>
AAMD_HD C rounded(C v) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm("" : "+v"(v));
#endif
  return v;
}

AAMD_HD bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
AAMD_HD int64_t n_chunks(int64_t L) { return (L + kChunk - 1) / kChunk; }

// samples [i0, i0 + V) of a row; those at or beyond `end` come back as zero bits
template <typename S>
AAMD_HD void load_group(const S* row, bool vec, int64_t i0, int64_t end, Vec<S>& v) {
  constexpr int V = 16 / sizeof(S);
  if (vec && i0 + V <= end) {
    v = *reinterpret_cast<const Vec<S>*>(row + i0);
    return;
  }
  for (int k = 0; k < V; ++k) v.e[k] = i0 + k < end ? row[i0 + k] : S(0);
}
template <typename S>
AAMD_HD void store_group(S* row, bool vec, int64_t i0, int64_t end, const Vec<S>& v) {
  constexpr int V = 16 / sizeof(S);
  if (vec && i0 + V <= end) {
    *reinterpret_cast<Vec<S>*>(row + i0) = v;
    return;
  }
  for (int k = 0; k < V; ++k)
    if (i0 + k < end) row[i0 + k] = v.e[k];
}

// ---- add_noise ------------------------------------------------------------------------------------------------------------
struct NoiseArgs {
  const void *w, *n, *g;        // (rows, L) through sw / sn / sg; g: the cotangent, gradient mode only
  void *out, *out2;             // dense (rows, L): w + s n; gradient mode: grad_w and grad_n
  double* ws;                   // [rows] grad_snr, then [rows][chunks][3] partial sums (Es, En, d)
  const double* snr;            // snr[row * ssnr], dB
  const int64_t* lengths;       // lengths[row * slen], or null: nothing is masked
  int64_t rows, L, sw, sn, sg, ssnr, slen, chunks;
  int32_t grad;
};

struct RowCoef {
  double s, a, b;               // scale; gradient mode: d s / Es and d s / En
};

AAMD_HD int64_t row_length(const NoiseArgs& a, int64_t row) {
  if (!a.lengths) return a.L;
  const int64_t l = a.lengths[row * a.slen];
  return l < 0 ? 0 : (l > a.L ? a.L : l);
}
AAMD_HD double* partials(const NoiseArgs& a, int64_t row, int64_t chunk) {
  return a.ws + a.rows + (row * a.chunks + chunk) * 3;
}

// One thread's share of a chunk's sums, elements in index order.
template <int DT>
AAMD_HD void reduce_thread(int tid, const NoiseArgs& a, int64_t row, int64_t chunk, double acc[3]) {
  using E = Elem<DT>;
  using S = typename E::S;
  constexpr int V = 16 / sizeof(S);
  const S* w = static_cast<const S*>(a.w) + row * a.sw;
  const S* n = static_cast<const S*>(a.n) + row * a.sn;
  const S* g = a.grad ? static_cast<const S*>(a.g) + row * a.sg : nullptr;
  const bool vw = aligned16(w), vn = aligned16(n), vg = aligned16(g);
  const int64_t len = row_length(a, row);
  const int64_t c0 = chunk * kChunk;
  const int64_t c1 = c0 + kChunk < a.L ? c0 + kChunk : a.L;
  const int64_t stop = a.grad ? c1 : (len < c1 ? len : c1);      // the forward reads nothing beyond the length
  double ew = 0.0, en = 0.0, d = 0.0;
  for (int64_t b0 = c0 + (int64_t)tid * V; b0 < stop; b0 += (int64_t)kBatch * kThreads * V) {
    Vec<S> wv[kBatch], nv[kBatch], gv[kBatch];
#pragma unroll
    for (int j = 0; j < kBatch; ++j) {
      const int64_t i0 = b0 + (int64_t)j * kThreads * V;
      if (i0 < stop) {
        load_group(w, vw, i0, c1, wv[j]);
        load_group(n, vn, i0, c1, nv[j]);
        if (a.grad) load_group(g, vg, i0, c1, gv[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < kBatch; ++j) {
      const int64_t i0 = b0 + (int64_t)j * kThreads * V;
      if (i0 < stop) {
#pragma unroll
        for (int k = 0; k < V; ++k) {
          const double nk = (double)E::load(nv[j].e[k]);
          if (i0 + k < len) {
            const double wk = (double)E::load(wv[j].e[k]);
            ew += wk * wk;
            en += nk * nk;
          }
          if (a.grad && i0 + k < c1) d += (double)E::load(gv[j].e[k]) * nk;
        }
      }
    }
  }
  acc[0] = ew; acc[1] = en; acc[2] = d;
}

// One thread's share of a row's partial sums, chunks in order.
AAMD_HD void partial_thread(int tid, const NoiseArgs& a, int64_t row, double acc[3]) {
  acc[0] = acc[1] = acc[2] = 0.0;
  for (int64_t c = tid; c < a.chunks; c += kThreads) {
    const double* p = partials(a, row, c);
    acc[0] += p[0];
    acc[1] += p[1];
    if (a.grad) acc[2] += p[2];
  }
}

// One step of the tree over the threads' sums (s: [3][kThreads]); the kernel separates the steps by barriers.
AAMD_HD void tree_step(int tid, int stride, double* s) {
  if (tid < stride) {
    s[tid] += s[tid + stride];
    s[kThreads + tid] += s[kThreads + tid + stride];
    s[2 * kThreads + tid] += s[2 * kThreads + tid + stride];
  }
}

// The reference's formula as written, in float64.  Zero energies give what IEEE arithmetic gives: 0, +inf or NaN.
AAMD_HD RowCoef row_coef(const NoiseArgs& a, int64_t row, double Es, double En, double d) {
  const double snr = a.snr[row * a.ssnr];
  const double original_snr_db = rounded(10.0 * (log10(Es) - log10(En)));
  RowCoef rc;
  rc.s = pow(10.0, (original_snr_db - snr) / 20.0);
  rc.a = a.grad ? d * (rc.s / Es) : 0.0;
  rc.b = a.grad ? d * (rc.s / En) : 0.0;
  return rc;
}
AAMD_HD double grad_snr_of(const RowCoef& rc, double d) {
  return -(2.302585092994045684 / 20.0) * rc.s * d;
}

template <int DT>
AAMD_HD void apply_thread(int tid, const NoiseArgs& a, int64_t row, int64_t chunk, const RowCoef& rc) {
  using E = Elem<DT>;
  using S = typename E::S;
  using C = typename E::C;
  constexpr int V = 16 / sizeof(S);
  const S* w = static_cast<const S*>(a.w) + row * a.sw;
  const S* n = static_cast<const S*>(a.n) + row * a.sn;
  const S* g = a.grad ? static_cast<const S*>(a.g) + row * a.sg : nullptr;
  S* o = static_cast<S*>(a.out) + row * a.L;
  S* o2 = a.grad ? static_cast<S*>(a.out2) + row * a.L : nullptr;
  const bool vw = aligned16(w), vn = aligned16(n), vg = aligned16(g), vo = aligned16(o), vo2 = aligned16(o2);
  const int64_t len = row_length(a, row);
  const int64_t c0 = chunk * kChunk;
  const int64_t c1 = c0 + kChunk < a.L ? c0 + kChunk : a.L;
  const C s = (C)rc.s, ca = (C)rc.a, cb = (C)rc.b;               // rounded once to the compute type
  for (int64_t b0 = c0 + (int64_t)tid * V; b0 < c1; b0 += (int64_t)kBatch * kThreads * V) {
    Vec<S> wv[kBatch], nv[kBatch], gv[kBatch];
#pragma unroll
    for (int j = 0; j < kBatch; ++j) {
      const int64_t i0 = b0 + (int64_t)j * kThreads * V;
      if (i0 < c1) {
        load_group(w, vw, i0, c1, wv[j]);
        load_group(n, vn, i0, c1, nv[j]);
        if (a.grad) load_group(g, vg, i0, c1, gv[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < kBatch; ++j) {
      const int64_t i0 = b0 + (int64_t)j * kThreads * V;
      if (i0 < c1) {
        Vec<S> r, r2;
#pragma unroll
        for (int k = 0; k < V; ++k) {
          const C wk = E::load(wv[j].e[k]), nk = E::load(nv[j].e[k]);
          if (!a.grad) {
            const C p = rounded(s * nk);
            r.e[k] = E::store(wk + p);
          } else {
            const C gk = E::load(gv[j].e[k]);
            const C m = i0 + k < len ? C(1) : C(0);
            const C tw = rounded(rounded(ca * wk) * m), tn = rounded(rounded(cb * nk) * m);
            const C sg = rounded(s * gk);
            r.e[k] = E::store(gk + tw);
            r2.e[k] = E::store(sg - tn);
          }
        }
        store_group(o, vo, i0, c1, r);
        if (a.grad) store_group(o2, vo2, i0, c1, r2);
      }
    }
  }
}

// ---- preemphasis ----------------------------------------------------------------------------------------------------------
struct PreArgs {
  const void* x;                // (rows, L) through sx
  void* out;                    // dense (rows, L)
  int64_t rows, L, sx, chunks;
  double coeff;
  int32_t transposed;
};

template <int DT>
AAMD_HD void pre_thread(int tid, const PreArgs& a, int64_t row, int64_t chunk) {
  using E = Elem<DT>;
  using S = typename E::S;
  using C = typename E::C;
  constexpr int V = 16 / sizeof(S);
  const S* x = static_cast<const S*>(a.x) + row * a.sx;
  S* o = static_cast<S*>(a.out) + row * a.L;
  const bool vx = aligned16(x), vo = aligned16(o);
  const int64_t c0 = chunk * kChunk;
  const int64_t c1 = c0 + kChunk < a.L ? c0 + kChunk : a.L;
  const C c = (C)a.coeff;
  for (int64_t b0 = c0 + (int64_t)tid * V; b0 < c1; b0 += (int64_t)kBatch * kThreads * V) {
    Vec<S> xv[kBatch];
    S halo[kBatch];             // the one sample beside the group: x[i0 - 1], transposed x[i0 + V]
#pragma unroll
    for (int j = 0; j < kBatch; ++j) {
      const int64_t i0 = b0 + (int64_t)j * kThreads * V;
      if (i0 < c1) {
        load_group(x, vx, i0, a.L, xv[j]);
        const int64_t h = a.transposed ? i0 + V : i0 - 1;
        halo[j] = (h >= 0 && h < a.L) ? x[h] : S(0);
      }
    }
#pragma unroll
    for (int j = 0; j < kBatch; ++j) {
      const int64_t i0 = b0 + (int64_t)j * kThreads * V;
      if (i0 < c1) {
        Vec<S> r;
#pragma unroll
        for (int k = 0; k < V; ++k) {
          const int64_t i = i0 + k;
          const C xk = E::load(xv[j].e[k]);
          C other;
          bool edge;
          if (a.transposed) {
            other = E::load(k + 1 < V ? xv[j].e[k + 1 < V ? k + 1 : k] : halo[j]);
            edge = i + 1 >= a.L;
          } else {
            other = E::load(k > 0 ? xv[j].e[k > 0 ? k - 1 : k] : halo[j]);
            edge = i == 0;
          }
          const C p = rounded(c * other);
          r.e[k] = edge ? xv[j].e[k] : E::store(xk - p);
        }
        store_group(o, vo, i0, c1, r);
      }
    }
  }
}

#if defined(__HIPCC__)
template <int DT>
__global__ __launch_bounds__(kThreads) void add_noise_reduce_kernel(NoiseArgs a) {
  __shared__ double s[3 * kThreads];
  const int tid = threadIdx.x;
  const int64_t row = (int64_t)blockIdx.x / a.chunks, chunk = (int64_t)blockIdx.x - row * a.chunks;
  double acc[3];
  reduce_thread<DT>(tid, a, row, chunk, acc);
  s[tid] = acc[0]; s[kThreads + tid] = acc[1]; s[2 * kThreads + tid] = acc[2];
  __syncthreads();
  for (int stride = kThreads / 2; stride > 0; stride >>= 1) {
    tree_step(tid, stride, s);
    __syncthreads();
  }
  if (tid < 3) partials(a, row, chunk)[tid] = s[tid * kThreads];
}

template <int DT>
__global__ __launch_bounds__(kThreads) void add_noise_apply_kernel(NoiseArgs a) {
  __shared__ double s[3 * kThreads];
  __shared__ RowCoef coef;
  const int tid = threadIdx.x;
  const int64_t row = (int64_t)blockIdx.x / a.chunks, chunk = (int64_t)blockIdx.x - row * a.chunks;
  double acc[3];
  partial_thread(tid, a, row, acc);
  s[tid] = acc[0]; s[kThreads + tid] = acc[1]; s[2 * kThreads + tid] = acc[2];
  __syncthreads();
  for (int stride = kThreads / 2; stride > 0; stride >>= 1) {
    tree_step(tid, stride, s);
    __syncthreads();
  }
  if (tid == 0) {
    const RowCoef rc = row_coef(a, row, s[0], s[kThreads], s[2 * kThreads]);
    coef = rc;
    if (a.grad && chunk == 0) a.ws[row] = grad_snr_of(rc, s[2 * kThreads]);
  }
  __syncthreads();
  const RowCoef rc = coef;
  apply_thread<DT>(tid, a, row, chunk, rc);
}

template <int DT>
__global__ __launch_bounds__(kThreads) void preemphasis_kernel(PreArgs a) {
  const int64_t row = (int64_t)blockIdx.x / a.chunks, chunk = (int64_t)blockIdx.x - row * a.chunks;
  pre_thread<DT>(threadIdx.x, a, row, chunk);
}
#endif

}  // namespace wa
}  // namespace aamd
