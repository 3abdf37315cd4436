// CPU replay of the SpecAugment masking kernel (audio_amd/csrc/spec_augment.h compiled with g++, no GPU): the bounds
// arithmetic on its own, and the whole kernel -- "the first n_masks threads fill the bounds, __syncthreads(), every thread
// runs the body" as loops over workgroups and thread ids, with the launch geometry of the C ABI (plan_masks, plan_is_dense,
// plan_chunks).  TEST INFRASTRUCTURE ONLY.
#include <cstdint>

#include "../../audio_amd/csrc/spec_augment.h"

using namespace aamd;

extern "C" {

// start / end of n masks from raw draw bits (r0, r1: n elements of the dtype's width, widened to uint64 by the caller)
void sim_sa_bounds(int dtype, const uint64_t* r0, const uint64_t* r1, int64_t n, int64_t param, int64_t size, int64_t* start,
                   int64_t* end) {
  for (int64_t k = 0; k < n; ++k) sa::mask_bounds(dtype, r0[k], r1[k], param, size, start[k], end[k]);
}

// element `rel` of an (O, I) example -> (outer, inner), and the mask bits of the n-element vector that starts there
// under one inner mask [ilo, ihi) and one outer mask [olo, ohi)
uint32_t sim_sa_vector_bits(int64_t O, int64_t I, int64_t rel, int n, int32_t ilo, int32_t ihi, int32_t olo, int32_t ohi,
                            int32_t* oi) {
  sa::Plan p{};
  p.E = 1; p.O = O; p.I = I;
  p.n_masks = 2; p.n_inner = 1;
  sa::Bounds b{};
  b.lo[0] = ilo; b.hi[0] = ihi; b.lo[1] = olo; b.hi[1] = ohi;
  sa::locate(p, rel, oi[0], oi[1]);
  return sa::vector_bits(p, b, oi[0], oi[1], n);
}

// The kernel.  Returns 1 when the dense path ran, 0 for the gather path, < 0 on a bad argument.
int sim_sa_run(const void* x, void* out, int64_t E, int64_t O, int64_t I, int64_t xe, int64_t xo, int64_t xi, int dtype,
               int time_inner, int n_masks, const int32_t* axes, const int64_t* params, const void* draws,
               const int64_t* starts, const int64_t* ends, uint64_t value_bits, const void* value_ptr, int force_gather) {
  if (n_masks < 0 || n_masks > sa::kMaxMasks) return -1;
  sa::Plan p{};
  p.E = E; p.O = O; p.I = I;
  p.xe = xe; p.xo = xo; p.xi = xi;
  p.draws = draws; p.value_ptr = value_ptr; p.value_bits = value_bits;
  p.dtype = dtype;
  sa::plan_masks(p, time_inner, n_masks, axes, draws ? params : nullptr, starts, ends);
  const int es = sa::elem_size(dtype);
  const bool dense = !force_gather && sa::plan_is_dense(p, x, out);
  sa::plan_chunks(p, dense, es);
  for (int64_t blk = 0; blk < E * p.chunks; ++blk) {
    const int64_t e = blk / p.chunks, chunk = blk - e * p.chunks;
    sa::Bounds bd{};
    for (int tid = 0; tid < n_masks; ++tid) sa::example_bounds(tid, p, e, bd);
    for (int tid = 0; tid < sa::kThreads; ++tid) {
      if (dense) {
        if (es == 2) sa::dense_body<2>(tid, sa::kThreads, p, bd, e, chunk, x, out);
        else if (es == 4) sa::dense_body<4>(tid, sa::kThreads, p, bd, e, chunk, x, out);
        else sa::dense_body<8>(tid, sa::kThreads, p, bd, e, chunk, x, out);
      } else {
        if (es == 2) sa::gather_body<2>(tid, sa::kThreads, p, bd, e, chunk, x, out);
        else if (es == 4) sa::gather_body<4>(tid, sa::kThreads, p, bd, e, chunk, x, out);
        else sa::gather_body<8>(tid, sa::kThreads, p, bd, e, chunk, x, out);
      }
    }
  }
  return dense ? 1 : 0;
}

}  // extern "C"
