// Pointwise waveform ops (F.gain / T.Vol, F.contrast, F.DB_to_amplitude, F.mu_law_encoding / T.MuLawEncoding,
// F.mu_law_decoding / T.MuLawDecoding, T.Fade): one templated streaming kernel, pointwise_kernel<OP, DIN, DOUT>.
//
// The reference builds each of these from three to eight element-wise launches, a full read and write of the batch each.
// Here every op is one pass: one read of x, one write of the result, the arithmetic of the reference's expression in its
// order in between.
//
//   scale      x * p0, then clamped to [-1, 1] where `flag` is set (Vol); one product, so the bits are numpy's
//   contrast   t = x * p0 (p0 = pi / 2);  sin(t + p1 * sin(t * 4))                                 (p1 = amount / 750)
//   db_to_amp  p0 * pow(pow(10, 0.1 * x), p1)                                                      (p0 = ref, p1 = power)
//   mu_encode  v = sign(x) * log1p(mu * |x|) / log1p(mu);  int64((v + 1) / 2 * mu + 0.5), toward zero   (p0 = mu = Q - 1)
//   mu_decode  y = x / mu * 2 - 1;  sign(y) * (exp(|y| * log1p(mu)) - 1) / mu                      (p0 = mu; x may be integers)
//   fade       (fade_in[i] * fade_out[i]) * x[i]: the ramps are host tables of the tensor's type, table[0 .. n_in) and
//              table[n_in .. n_in + n_out); a sample outside both ramps is copied bit for bit, a sample inside one ramp
//              is one product, a sample inside both the product of the two table values (rounded) times x
//
// Arithmetic.  float32 and float64 compute in their own precision, float16 and bfloat16 are widened on load, computed in
// float32 and rounded once on store.  The scalar parameters arrive as doubles and are rounded once to the compute type.
// The transcendental functions are the accurate libm forms (log1pf, expf, sinf, powf and their double versions), never
// the fast intrinsics.  The library is built with -ffp-contract=fast: a product the reference rounds before it adds to it
// goes through wa::rounded().
//
// Rows.  x is (rows, L) with unit stride along time and one row stride in elements (0 for a single row, more than L for
// rows cut from a wider tensor); the result is dense.  A thread owns the G = 16 / min(sizeof in, sizeof out) consecutive
// samples at a fixed index of its chunk, whatever the addresses are: a row that starts on a 16-byte boundary moves them
// with 16-byte accesses, any other row sample by sample -- decided per row for the input and for the output, so nothing is
// copied first and the result does not depend on the alignment.
//
// The phase functions are AAMD_HD: tests/cpu_sim/sim_spectral_point.cpp replays them with g++.
#pragma once
#include <type_traits>

#include "hd.h"
#include "wave_augment.h"   // wa::Elem, wa::rounded, wa::aligned16

#if !defined(__HIPCC__)
using std::sin;
using std::exp;
using std::log1p;
using std::fabs;
#endif

namespace aamd {
namespace pw {

constexpr int kThreads = 256;
constexpr int kChunk = 4096;   // samples per workgroup, every type
constexpr int kBatch = 4;      // groups per thread whose loads are issued together

enum { kScale = 0, kContrast = 1, kDbToAmp = 2, kMuEncode = 3, kMuDecode = 4, kFade = 5, kOps = 6 };   // = AAMD_PW_*
// element types: 0 .. 3 are wa::kF32, kF64, kF16, kBF16 (= AAMD_SA_*); the integer codes of mu_decode and mu_encode follow
enum { kI64 = 4, kI32 = 5, kI16 = 6, kI8 = 7, kU8 = 8, kTypes = 9 };

// storage type S, compute type C; an integer type computes in float32 (the reference converts codes to float first)
template <int DT> struct Elem : wa::Elem<DT> {};
#if defined(__HIP_DEVICE_COMPILE__)
// float16 on the device: the hardware's conversions (round to nearest even, subnormals kept) in place of the bit arithmetic
// the CPU replay runs, which bounded the float16 ops (contrast on (256, 160000): 99.7 us with it, 67.1 us with these)
template <> struct Elem<wa::kF16> {
  using S = uint16_t; using C = float;
  static __device__ __forceinline__ C load(S v) {
    _Float16 h;
    __builtin_memcpy(&h, &v, 2);
    return (C)h;
  }
  static __device__ __forceinline__ S store(C v) {
    // rounded(): the conversion stays an instruction of its own.  Fused with the float32 product that feeds it, the fade of
    // a negative sample by a ramp value of zero came out as +0 on the device where the product is -0.
    const _Float16 h = (_Float16)wa::rounded(v);
    S u;
    __builtin_memcpy(&u, &h, 2);
    return u;
  }
};
#endif
template <typename I> struct IntElem {
  using S = I; using C = float;
  static AAMD_HD C load(S v) { return (C)v; }
};
template <> struct Elem<kI64> : IntElem<int64_t> {};
template <> struct Elem<kI32> : IntElem<int32_t> {};
template <> struct Elem<kI16> : IntElem<int16_t> {};
template <> struct Elem<kI8> : IntElem<int8_t> {};
template <> struct Elem<kU8> : IntElem<uint8_t> {};

template <typename S, int G>
struct alignas(16) Group {
  S e[G];
};

struct Args {
  const void* x;                // (rows, L) through sx
  void* out;                    // dense (rows, L)
  const void* table;            // fade: the two ramps in the tensor's type
  int64_t rows, L, sx, chunks;
  int64_t n_in, n_out;          // fade: ramp lengths, each <= L
  double p0, p1;
  int32_t flag;
};

AAMD_HD int64_t n_chunks(int64_t L) { return (L + kChunk - 1) / kChunk; }

// .to(torch.int64): truncation toward zero; what no int64 holds (infinities, NaN) becomes the most negative one
template <typename C>
AAMD_HD int64_t trunc_i64(C v) {
  if (!(v > (C)-9223372036854775808.0 && v < (C)9223372036854775808.0)) return INT64_MIN;
  return (int64_t)v;
}

template <typename C>
AAMD_HD C sign_of(C v) {       // torch.sign: 0 for 0 and for NaN
  return (C)((v > C(0)) - (v < C(0)));
}

AAMD_HD float pw_sin(float v) { return sinf(v); }
AAMD_HD double pw_sin(double v) { return sin(v); }
AAMD_HD float pw_exp(float v) { return expf(v); }
AAMD_HD double pw_exp(double v) { return exp(v); }
AAMD_HD float pw_log1p(float v) { return log1pf(v); }
AAMD_HD double pw_log1p(double v) { return log1p(v); }
AAMD_HD float pw_pow(float a, float b) { return powf(a, b); }
AAMD_HD double pw_pow(double a, double b) { return pow(a, b); }
AAMD_HD float pw_abs(float v) { return fabsf(v); }
AAMD_HD double pw_abs(double v) { return fabs(v); }

// What a thread needs of the arguments, rounded once to the compute type.
template <typename C>
struct Coef {
  C p0, p1, l1p;                // l1p: log1p(mu) of the two mu-law ops
};

template <int OP, typename C>
AAMD_HD Coef<C> coef_of(const Args& a) {
  Coef<C> k;
  k.p0 = (C)a.p0;
  k.p1 = (C)a.p1;
  k.l1p = (OP == kMuEncode || OP == kMuDecode) ? pw_log1p(k.p0) : C(0);
  return k;
}

template <int OP, typename C>
AAMD_HD C value_of(C x, const Coef<C>& k, int32_t flag) {
  if constexpr (OP == kScale) {
    const C v = x * k.p0;
    if (!flag) return v;
    return v < C(-1) ? C(-1) : (v > C(1) ? C(1) : v);         // a NaN stays
  }
  if constexpr (OP == kContrast) {
    const C t = wa::rounded(x * k.p0);
    const C u = wa::rounded(k.p1 * pw_sin(t * C(4)));
    return pw_sin(t + u);
  }
  if constexpr (OP == kDbToAmp) {
    const C t = wa::rounded(C(0.1) * x);
    return k.p0 * pw_pow(pw_pow(C(10), t), k.p1);
  }
  if constexpr (OP == kMuDecode) {
    const C y = wa::rounded(wa::rounded(x / k.p0) * C(2)) - C(1);
    const C e = pw_exp(wa::rounded(pw_abs(y) * k.l1p)) - C(1);
    return wa::rounded(sign_of(y) * e) / k.p0;
  }
  return x;
}

template <typename C>
AAMD_HD int64_t mu_code(C x, const Coef<C>& k) {
  const C m = wa::rounded(k.p0 * pw_abs(x));
  const C v = wa::rounded(sign_of(x) * pw_log1p(m)) / k.l1p;
  const C s = wa::rounded(wa::rounded((v + C(1)) / C(2)) * k.p0);
  return trunc_i64(s + C(0.5));
}

// One thread's share of a chunk: the groups at tid, tid + kThreads, ... of the chunk, kBatch of them in flight.
template <int OP, int DIN, int DOUT>
AAMD_HD void chunk_thread(int tid, const Args& a, int64_t row, int64_t chunk) {
  using EI = Elem<DIN>;
  using SI = typename EI::S;
  using C = typename EI::C;
  using EO = Elem<(DOUT < 4 ? DOUT : 0)>;
  using SO = typename std::conditional<OP == kMuEncode, int64_t, typename EO::S>::type;
  constexpr int kSmall = sizeof(SI) < sizeof(SO) ? (int)sizeof(SI) : (int)sizeof(SO);
  constexpr int G = 16 / kSmall;
  const SI* x = static_cast<const SI*>(a.x) + row * a.sx;
  SO* o = static_cast<SO*>(a.out) + row * a.L;
  const SI* tab = static_cast<const SI*>(a.table);
  const bool vx = wa::aligned16(x), vo = wa::aligned16(o);
  const int64_t c0 = chunk * kChunk;
  const int64_t c1 = c0 + kChunk < a.L ? c0 + kChunk : a.L;
  const int64_t out0 = a.L - a.n_out;                           // fade: the first sample of the fade-out ramp
  const Coef<C> k = coef_of<OP, C>(a);
  for (int64_t b0 = c0 + (int64_t)tid * G; b0 < c1; b0 += (int64_t)kBatch * kThreads * G) {
    Group<SI, G> xv[kBatch];
#pragma unroll
    for (int j = 0; j < kBatch; ++j) {
      const int64_t i0 = b0 + (int64_t)j * kThreads * G;
      if (i0 < c1) {
        if (vx && i0 + G <= c1) {
          xv[j] = *reinterpret_cast<const Group<SI, G>*>(x + i0);
        } else {
#pragma unroll
          for (int e = 0; e < G; ++e) xv[j].e[e] = i0 + e < c1 ? x[i0 + e] : SI(0);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < kBatch; ++j) {
      const int64_t i0 = b0 + (int64_t)j * kThreads * G;
      if (i0 < c1) {
        Group<SO, G> r;
#pragma unroll
        for (int e = 0; e < G; ++e) {
          const SI xs = xv[j].e[e];
          if constexpr (OP == kMuEncode) {
            r.e[e] = (SO)mu_code<C>(EI::load(xs), k);
          } else if constexpr (OP == kFade) {
            const int64_t i = i0 + e;
            const bool in = i < a.n_in, ou = i >= out0 && i < a.L;
            SO v = (SO)xs;                                      // outside the ramps: the bits as they are
            if (in && ou) {
              const C f = wa::rounded(EI::load(tab[i]) * EI::load(tab[a.n_in + (i - out0)]));
              v = (SO)EO::store((typename EO::C)(f * EI::load(xs)));
            } else if (in) {
              v = (SO)EO::store((typename EO::C)(EI::load(tab[i]) * EI::load(xs)));
            } else if (ou) {
              v = (SO)EO::store((typename EO::C)(EI::load(tab[a.n_in + (i - out0)]) * EI::load(xs)));
            }
            r.e[e] = v;
          } else {
            r.e[e] = (SO)EO::store((typename EO::C)value_of<OP, C>(EI::load(xs), k, a.flag));
          }
        }
        if (vo && i0 + G <= c1) {
          *reinterpret_cast<Group<SO, G>*>(o + i0) = r;
        } else {
#pragma unroll
          for (int e = 0; e < G; ++e)
            if (i0 + e < c1) o[i0 + e] = r.e[e];
        }
      }
    }
  }
}

#if defined(__HIPCC__)
template <int OP, int DIN, int DOUT>
__global__ __launch_bounds__(kThreads) void pointwise_kernel(Args a) {
  const int64_t row = (int64_t)blockIdx.x / a.chunks, chunk = (int64_t)blockIdx.x - row * a.chunks;
  chunk_thread<OP, DIN, DOUT>(threadIdx.x, a, row, chunk);
}
#endif

}  // namespace pw
}  // namespace aamd
