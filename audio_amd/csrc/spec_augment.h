// SpecAugment masking (F.mask_along_axis / F.mask_along_axis_iid, T.FrequencyMasking / T.TimeMasking / T.SpecAugment):
// a whole masking policy -- up to kMaxMasks masks, each along frequency or time -- in ONE streaming pass.
//
// The reference builds every mask from about a dozen element-wise launches and applies it with one masked_fill, a full
// read and write of the batch per mask.  With mask_value fixed the union of the masks does not depend on their order, so
// the policy is one copy with some elements replaced:  out[e, f, t] = masked(e, f, t) ? mask_value : x[e, f, t].
//
// Geometry.  The tensor is (examples, outer, inner) with `inner` the axis the caller's storage is contiguous along: time
// for a time-contiguous tensor, frequency for the frame-major storage of every MelSpectrogram output.  Masks are sorted by
// the host into inner-axis masks [0, n_inner) and outer-axis masks [n_inner, n_masks).  One workgroup serves a chunk of
// ONE example, so the example's bounds are computed once, into LDS, by the first n_masks threads:
//   iid:    from the raw uniform draws (device memory, [mask][2][examples] in the tensor's dtype) with the reference's
//           arithmetic, every product and difference rounded the way aten rounds it (float32 op-math for float16 and
//           bfloat16, rounded to the type after each op; no contraction into FMAs):
//             value = r0 * mask_param;  min_value = r1 * (size - value);  start = (long) min_value;  end = start + (long) value
//   shared: clamped integer bounds that arrive by value in the kernel arguments.
// Dense path (x is one dense block, both pointers 16-byte aligned): the flat tensor is cut into 16-byte vectors at
// multiples of 16 bytes from the base, whatever the row length.  Each thread owns kUnroll vectors per round: it forms their
// mask bits (one bit per element), issues the loads of all vectors that are not wholly masked, blends and stores.  A vector
// inside one row takes the interval form (a few integer ops per mask); a vector that crosses rows is walked element by
// element.  The elements of an example before its first and after its last whole vector are copied one by one.
// Gather path (any other strides or alignment): one element per thread and step through the strides; out is dense.
// Elements are moved as 2-, 4- or 8-byte integers: unmasked values are bit copies.
//
// The phase functions are AAMD_HD: tests/cpu_sim/sim_spec_augment.cpp replays them with g++.
#pragma once
#include "hd.h"

#include <string.h>

namespace aamd {
namespace sa {

constexpr int kMaxMasks = 32;
constexpr int kThreads = 256;
constexpr int kUnroll = 4;        // 16-byte vectors per thread whose loads are issued together
constexpr int kMaxBlocks = 2048;  // 256 CUs x 8: the rest of the work is strided over inside the workgroups

enum { kF32 = 0, kF64 = 1, kF16 = 2, kBF16 = 3 };

struct alignas(16) V16 {
  uint32_t w[4];
};

struct Plan {
  int64_t E, O, I;          // examples, outer and inner length
  int64_t xe, xo, xi;       // element strides of x (gather path)
  int64_t chunks;           // workgroups per example
  const void* draws;        // iid: [mask][2][E] uniform draws of the tensor's dtype
  const void* value_ptr;    // mask_value as one device element of the tensor's dtype, or null: value_bits
  uint64_t value_bits;
  int32_t n_masks, n_inner;
  int32_t dtype;            // kF32 ..: decides the arithmetic of the bounds only
  int32_t iid;
  int32_t slot[kMaxMasks];  // iid: the mask's row of `draws`
  int64_t param[kMaxMasks]; // iid: effective mask_param
  int32_t lo[kMaxMasks];    // shared: bounds clamped to [0, size], lo == hi == 0 when empty
  int32_t hi[kMaxMasks];
};

struct Bounds {
  int32_t lo[kMaxMasks], hi[kMaxMasks];
};

// ---- number formats ----------------------------------------------------------------------------------------------------
AAMD_HD uint32_t f32_bits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}
AAMD_HD float bits_f32(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}

AAMD_HD float f16_to_f32(uint16_t h) {
  const uint32_t s = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3ffu;
  if (e == 0) return bits_f32(s | f32_bits((float)m * 5.9604644775390625e-8f));   // zero, subnormal: m 2^-24 (exact)
  if (e == 31) return bits_f32(s | 0x7f800000u | (m << 13));
  return bits_f32(s | ((e + 112u) << 23) | (m << 13));
}

// round to nearest even, as aten's float -> Half conversion
AAMD_HD uint16_t f32_to_f16(float f) {
  uint32_t x = f32_bits(f);
  const uint32_t s = (x >> 16) & 0x8000u;
  x &= 0x7fffffffu;
  if (x > 0x7f800000u) return (uint16_t)(s | 0x7e00u);
  if (x >= 0x477ff000u) return (uint16_t)(s | 0x7c00u);                 // >= 65520 rounds to infinity
  if (x < 0x38800000u) {                                                // below 2^-14: a float16 subnormal or zero
    const float a = bits_f32(x) + 0.5f;                                 // the sum's low mantissa bits are the rounded result
    return (uint16_t)(s | (f32_bits(a) - 0x3f000000u));
  }
  const uint32_t odd = (x >> 13) & 1u;
  x += 0xc8000fffu + odd;                                               // rebias the exponent by -112, round half to even
  return (uint16_t)(s | (x >> 13));
}

AAMD_HD float bf16_to_f32(uint16_t h) { return bits_f32((uint32_t)h << 16); }

AAMD_HD uint16_t f32_to_bf16(float f) {
  uint32_t x = f32_bits(f);
  if ((x & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;
  x += 0x7fffu + ((x >> 16) & 1u);
  return (uint16_t)(x >> 16);
}

// .long(): truncation toward zero; what no int64 holds (infinities, NaN) becomes the most negative one
AAMD_HD int64_t trunc_f32(float v) {
  return (v >= -9.2e18f && v <= 9.2e18f) ? (int64_t)v : INT64_MIN;
}
AAMD_HD int64_t trunc_f64(double v) {
  return (v >= -9.2e18 && v <= 9.2e18) ? (int64_t)v : INT64_MIN;
}

// ---- bounds from the draws ---------------------------------------------------------------------------------------------
// [start, end) of one mask of one example; r0 and r1 are the raw bits of the two draws.
AAMD_HD void mask_bounds(int dtype, uint64_t r0, uint64_t r1, int64_t param, int64_t size, int64_t& start, int64_t& end) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (dtype == kF64) {
    double a, b;
    memcpy(&a, &r0, 8);
    memcpy(&b, &r1, 8);
    const double value = a * (double)param;
    const double min_value = b * ((double)size - value);
    start = trunc_f64(min_value);
    end = start + trunc_f64(value);
    return;
  }
  float value, min_value;
  if (dtype == kF32) {
    value = bits_f32((uint32_t)r0) * (float)param;
    min_value = bits_f32((uint32_t)r1) * ((float)size - value);
  } else if (dtype == kF16) {
    value = f16_to_f32(f32_to_f16(f16_to_f32((uint16_t)r0) * (float)param));
    const float room = f16_to_f32(f32_to_f16((float)size - value));
    min_value = f16_to_f32(f32_to_f16(f16_to_f32((uint16_t)r1) * room));
  } else {
    value = bf16_to_f32(f32_to_bf16(bf16_to_f32((uint16_t)r0) * (float)param));
    const float room = bf16_to_f32(f32_to_bf16((float)size - value));
    min_value = bf16_to_f32(f32_to_bf16(bf16_to_f32((uint16_t)r1) * room));
  }
  start = trunc_f32(min_value);
  end = start + trunc_f32(value);
}

// [start, end) cut to the axis [0, size); an empty mask is (0, 0)
AAMD_HD void clamp_bounds(int64_t start, int64_t end, int64_t size, int32_t& lo, int32_t& hi) {
  const int64_t a = start < 0 ? 0 : start, b = end > size ? size : end;
  if (b <= a) {
    lo = 0;
    hi = 0;
  } else {
    lo = (int32_t)a;
    hi = (int32_t)b;
  }
}

AAMD_HD uint64_t load_elem(const void* p, int64_t at, int es) {
  if (es == 2) return static_cast<const uint16_t*>(p)[at];
  if (es == 4) return static_cast<const uint32_t*>(p)[at];
  return static_cast<const uint64_t*>(p)[at];
}

AAMD_HD int elem_size(int dtype) { return dtype == kF64 ? 8 : (dtype == kF32 ? 4 : 2); }

// Prologue, thread m < n_masks: mask m's bounds for example e.
AAMD_HD void example_bounds(int m, const Plan& p, int64_t e, Bounds& b) {
  if (!p.iid) {
    b.lo[m] = p.lo[m];
    b.hi[m] = p.hi[m];
    return;
  }
  const int es = elem_size(p.dtype);
  const int64_t row = (int64_t)p.slot[m] * 2 * p.E;
  const uint64_t r0 = load_elem(p.draws, row + e, es), r1 = load_elem(p.draws, row + p.E + e, es);
  const int64_t size = m < p.n_inner ? p.I : p.O;
  int64_t start, end;
  mask_bounds(p.dtype, r0, r1, p.param[m], size, start, end);
  clamp_bounds(start, end, size, b.lo[m], b.hi[m]);
}

// ---- index maps --------------------------------------------------------------------------------------------------------
// element `rel` of an example -> (outer, inner); 32-bit division wherever the example is small enough
AAMD_HD void locate(const Plan& p, int64_t rel, int32_t& o, int32_t& i) {
  if (p.O * p.I <= 0xffffffffll) {
    const uint32_t q = (uint32_t)rel / (uint32_t)p.I;
    o = (int32_t)q;
    i = (int32_t)((uint32_t)rel - q * (uint32_t)p.I);
  } else {
    const int64_t q = rel / p.I;
    o = (int32_t)q;
    i = (int32_t)(rel - q * p.I);
  }
}

AAMD_HD bool element_masked(const Plan& p, const Bounds& b, int32_t o, int32_t i) {
  bool m = false;
  for (int k = 0; k < p.n_inner; ++k) m |= (i >= b.lo[k]) & (i < b.hi[k]);
  for (int k = p.n_inner; k < p.n_masks; ++k) m |= (o >= b.lo[k]) & (o < b.hi[k]);
  return m;
}

// bit k: element k of the n-element vector that starts at (o, i) is masked; the vector runs on into the following rows
AAMD_HD uint32_t vector_bits(const Plan& p, const Bounds& b, int32_t o, int32_t i, int n) {
  if ((int64_t)i + n <= p.I) {                          // inside one row: every mask is an interval of bit positions
    bool row = false;
    for (int k = p.n_inner; k < p.n_masks; ++k) row |= (o >= b.lo[k]) & (o < b.hi[k]);
    uint32_t bits = 0;
    for (int k = 0; k < p.n_inner; ++k) {
      int l = b.lo[k] - i, h = b.hi[k] - i;             // lo <= hi, so l <= h after both clamps
      l = l < 0 ? 0 : (l > n ? n : l);
      h = h < 0 ? 0 : (h > n ? n : h);
      bits |= (1u << h) - (1u << l);
    }
    return row ? (1u << n) - 1u : bits;
  }
  uint32_t bits = 0;
  for (int k = 0; k < n; ++k) {
    bits |= element_masked(p, b, o, i) ? 1u << k : 0u;
    if (++i == p.I) {
      i = 0;
      ++o;
    }
  }
  return bits;
}

template <int ES>
AAMD_HD V16 fill_vector(uint64_t v) {
  V16 f;
  if (ES == 8) {
    f.w[0] = f.w[2] = (uint32_t)v;
    f.w[1] = f.w[3] = (uint32_t)(v >> 32);
  } else {
    const uint32_t w = ES == 4 ? (uint32_t)v : ((uint32_t)(v & 0xffffu) * 0x10001u);
    f.w[0] = f.w[1] = f.w[2] = f.w[3] = w;
  }
  return f;
}

// elements whose bit is set come from `fill`, the others from `v`
template <int ES>
AAMD_HD V16 blend(V16 v, V16 fill, uint32_t bits) {
  V16 r;
  for (int d = 0; d < 4; ++d) {
    uint32_t m;
    if (ES == 8) m = ((bits >> (d >> 1)) & 1u) ? 0xffffffffu : 0u;
    else if (ES == 4) m = ((bits >> d) & 1u) ? 0xffffffffu : 0u;
    else m = (((bits >> (2 * d)) & 1u) ? 0xffffu : 0u) | (((bits >> (2 * d + 1)) & 1u) ? 0xffff0000u : 0u);
    r.w[d] = (v.w[d] & ~m) | (fill.w[d] & m);
  }
  return r;
}

template <int ES> struct Elem;
template <> struct Elem<2> { typedef uint16_t type; };
template <> struct Elem<4> { typedef uint32_t type; };
template <> struct Elem<8> { typedef uint64_t type; };

AAMD_HD uint64_t mask_value_bits(const Plan& p, int es) {
  return p.value_ptr ? load_elem(p.value_ptr, 0, es) : p.value_bits;
}

// ---- dense path --------------------------------------------------------------------------------------------------------
// The example's elements are [a, b) of the flat tensor; its whole vectors are [v0, v1).
template <int ES>
AAMD_HD void dense_body(int tid, int nthreads, const Plan& p, const Bounds& bd, int64_t e, int64_t chunk, const void* x,
                        void* out) {
  typedef typename Elem<ES>::type U;
  constexpr int V = 16 / ES;
  constexpr uint32_t kFull = (1u << V) - 1u, kNone = 0xffffffffu;
  const int64_t N = p.O * p.I, a = e * N, b = a + N;
  const int64_t v0 = (a + V - 1) / V;
  const int64_t v1 = b / V > v0 ? b / V : v0;
  const uint64_t value = mask_value_bits(p, ES);
  const U* xs = static_cast<const U*>(x);
  U* os = static_cast<U*>(out);
  if (chunk == 0) {                                     // the elements outside the whole vectors: fewer than V on each side
    const int64_t head_end = v0 * V < b ? v0 * V : b;
    const int64_t tail_at = v1 * V > head_end ? v1 * V : head_end;
    for (int side = 0; side < 2; ++side) {
      const int64_t at = (side ? tail_at : a) + tid, stop = side ? b : head_end;
      if (at < stop) {
        int32_t o, i;
        locate(p, at - a, o, i);
        os[at] = element_masked(p, bd, o, i) ? (U)value : xs[at];
      }
    }
  }
  const int64_t per = (v1 - v0 + p.chunks - 1) / p.chunks;
  const int64_t first = v0 + chunk * per;
  const int64_t last = first + per < v1 ? first + per : v1;
  const V16 fill = fill_vector<ES>(value);
  const V16* xv = static_cast<const V16*>(x);
  V16* ov = static_cast<V16*>(out);
  for (int64_t base = first + tid; base < last; base += (int64_t)nthreads * kUnroll) {
    V16 val[kUnroll];
    uint32_t bits[kUnroll];
#pragma unroll
    for (int k = 0; k < kUnroll; ++k) {
      const int64_t v = base + (int64_t)k * nthreads;
      bits[k] = kNone;
      if (v < last) {
        int32_t o, i;
        locate(p, v * V - a, o, i);
        bits[k] = vector_bits(p, bd, o, i, V);
      }
    }
#pragma unroll
    for (int k = 0; k < kUnroll; ++k) {
      val[k] = fill;
      if (bits[k] != kNone && bits[k] != kFull) val[k] = xv[base + (int64_t)k * nthreads];   // no load for a masked vector
    }
#pragma unroll
    for (int k = 0; k < kUnroll; ++k)
      if (bits[k] != kNone) ov[base + (int64_t)k * nthreads] = blend<ES>(val[k], fill, bits[k]);
  }
}

// ---- gather path -------------------------------------------------------------------------------------------------------
template <int ES>
AAMD_HD void gather_body(int tid, int nthreads, const Plan& p, const Bounds& bd, int64_t e, int64_t chunk, const void* x,
                         void* out) {
  typedef typename Elem<ES>::type U;
  const int64_t N = p.O * p.I;
  const int64_t per = (N + p.chunks - 1) / p.chunks;
  const int64_t first = chunk * per;
  const int64_t last = first + per < N ? first + per : N;
  const U value = (U)mask_value_bits(p, ES);
  const U* xs = static_cast<const U*>(x) + e * p.xe;
  U* os = static_cast<U*>(out) + e * N;
  for (int64_t rel = first + tid; rel < last; rel += nthreads) {
    int32_t o, i;
    locate(p, rel, o, i);
    os[rel] = element_masked(p, bd, o, i) ? value : xs[(int64_t)o * p.xo + (int64_t)i * p.xi];
  }
}

// Launch geometry (shared by the C ABI and the CPU replay): which path, and how many workgroups per example.
inline bool plan_is_dense(const Plan& p, const void* x, const void* out) {
  const bool dense = (p.I == 1 || p.xi == 1) && (p.O == 1 || p.xo == p.I) && (p.E == 1 || p.xe == p.O * p.I);
  return dense && (((uintptr_t)x | (uintptr_t)out) & 15) == 0;
}

// The masks in kernel order: inner-axis masks first.  params != null: iid (bounds from the draws), else shared bounds.
inline void plan_masks(Plan& p, int time_inner, int n_masks, const int32_t* axes, const int64_t* params, const int64_t* starts,
                       const int64_t* ends) {
  p.n_masks = n_masks;
  p.iid = params ? 1 : 0;
  int at = 0;
  for (int pass = 0; pass < 2; ++pass) {
    for (int m = 0; m < n_masks; ++m) {
      const bool inner = (axes[m] == 1) == (time_inner != 0);      // 1: AAMD_SA_TIME
      if (inner != (pass == 0)) continue;
      p.slot[at] = m;
      if (params) p.param[at] = params[m];
      else clamp_bounds(starts[m], ends[m], inner ? p.I : p.O, p.lo[at], p.hi[at]);
      ++at;
    }
    if (pass == 0) p.n_inner = at;
  }
}

inline void plan_chunks(Plan& p, bool dense, int elem_bytes) {
  const int64_t N = p.O * p.I;
  const int64_t items = dense ? (N * elem_bytes + 15) / 16 : N;
  const int64_t per_block = (int64_t)kThreads * (dense ? kUnroll : 1);
  int64_t want = (items + per_block - 1) / per_block;
  int64_t cap = kMaxBlocks / (p.E > 0 ? p.E : 1);
  if (cap < 1) cap = 1;
  if (want > cap) want = cap;
  p.chunks = want < 1 ? 1 : want;
}

#if defined(__HIPCC__)
template <int ES, int DENSE>
__global__ __launch_bounds__(kThreads) void spec_augment_kernel(const void* __restrict__ x, void* __restrict__ out, Plan p) {
  __shared__ Bounds bd;
  const int64_t e = blockIdx.x / p.chunks, chunk = blockIdx.x - e * p.chunks;
  if ((int)threadIdx.x < p.n_masks) example_bounds((int)threadIdx.x, p, e, bd);
  __syncthreads();
  if (DENSE) dense_body<ES>((int)threadIdx.x, kThreads, p, bd, e, chunk, x, out);
  else gather_body<ES>((int)threadIdx.x, kThreads, p, bd, e, chunk, x, out);
}
#endif

}  // namespace sa
}  // namespace aamd
