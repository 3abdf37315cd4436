// CPU replay of the waveform augmentation kernels (audio_amd/csrc/wave_augment.h compiled with g++, no GPU): each driver
// mirrors its __global__ kernel, "all threads run phase X, then __syncthreads()" replaced by a loop over thread ids, with
// the launch geometry and the workspace layout of the C ABI.  TEST INFRASTRUCTURE ONLY.
#include <cstdint>
#include <vector>

#include "../../audio_amd/csrc/wave_augment.h"

using namespace aamd;

static void tree(std::vector<double>& s) {
  for (int stride = wa::kThreads / 2; stride > 0; stride >>= 1)
    for (int tid = 0; tid < wa::kThreads; ++tid) wa::tree_step(tid, stride, s.data());
}

template <int DT>
static int add_noise(wa::NoiseArgs a) {
  std::vector<double> s(3 * wa::kThreads);
  for (int64_t blk = 0; blk < a.rows * a.chunks; ++blk) {          // add_noise_reduce_kernel
    const int64_t row = blk / a.chunks, chunk = blk - row * a.chunks;
    for (int tid = 0; tid < wa::kThreads; ++tid) {
      double acc[3];
      wa::reduce_thread<DT>(tid, a, row, chunk, acc);
      s[tid] = acc[0]; s[wa::kThreads + tid] = acc[1]; s[2 * wa::kThreads + tid] = acc[2];
    }
    tree(s);
    for (int tid = 0; tid < 3; ++tid) wa::partials(a, row, chunk)[tid] = s[tid * wa::kThreads];
  }
  for (int64_t blk = 0; blk < a.rows * a.chunks; ++blk) {          // add_noise_apply_kernel
    const int64_t row = blk / a.chunks, chunk = blk - row * a.chunks;
    for (int tid = 0; tid < wa::kThreads; ++tid) {
      double acc[3];
      wa::partial_thread(tid, a, row, acc);
      s[tid] = acc[0]; s[wa::kThreads + tid] = acc[1]; s[2 * wa::kThreads + tid] = acc[2];
    }
    tree(s);
    const wa::RowCoef rc = wa::row_coef(a, row, s[0], s[wa::kThreads], s[2 * wa::kThreads]);
    if (a.grad && chunk == 0) a.ws[row] = wa::grad_snr_of(rc, s[2 * wa::kThreads]);
    for (int tid = 0; tid < wa::kThreads; ++tid) wa::apply_thread<DT>(tid, a, row, chunk, rc);
  }
  return 0;
}

template <int DT>
static int preemphasis(wa::PreArgs a) {
  for (int64_t blk = 0; blk < a.rows * a.chunks; ++blk) {
    const int64_t row = blk / a.chunks, chunk = blk - row * a.chunks;
    for (int tid = 0; tid < wa::kThreads; ++tid) wa::pre_thread<DT>(tid, a, row, chunk);
  }
  return 0;
}

extern "C" {

int sim_wa_chunk() { return wa::kChunk; }

int64_t sim_wa_workspace_doubles(int64_t rows, int64_t L) { return rows + rows * wa::n_chunks(L) * 3; }

// ws: sim_wa_workspace_doubles() doubles.  Returns < 0 on an unknown dtype.
int sim_wa_add_noise(int dtype, const void* w, const void* n, const void* g, void* out, void* out2, double* ws, int64_t rows,
                     int64_t L, int64_t sw, int64_t sn, int64_t sg, const double* snr, int64_t ssnr, const int64_t* lengths,
                     int64_t slen, int grad) {
  wa::NoiseArgs a{};
  a.w = w; a.n = n; a.g = g; a.out = out; a.out2 = out2; a.ws = ws; a.snr = snr; a.lengths = lengths;
  a.rows = rows; a.L = L; a.sw = sw; a.sn = sn; a.sg = sg; a.ssnr = ssnr; a.slen = slen;
  a.chunks = wa::n_chunks(L);
  a.grad = grad;
  switch (dtype) {
    case wa::kF32: return add_noise<wa::kF32>(a);
    case wa::kF64: return add_noise<wa::kF64>(a);
    case wa::kF16: return add_noise<wa::kF16>(a);
    case wa::kBF16: return add_noise<wa::kBF16>(a);
    default: return -1;
  }
}

int sim_wa_preemphasis(int dtype, const void* x, void* out, int64_t rows, int64_t L, int64_t sx, double coeff, int transposed) {
  wa::PreArgs a{};
  a.x = x; a.out = out; a.rows = rows; a.L = L; a.sx = sx; a.chunks = wa::n_chunks(L);
  a.coeff = coeff; a.transposed = transposed;
  switch (dtype) {
    case wa::kF32: return preemphasis<wa::kF32>(a);
    case wa::kF64: return preemphasis<wa::kF64>(a);
    case wa::kF16: return preemphasis<wa::kF16>(a);
    case wa::kBF16: return preemphasis<wa::kBF16>(a);
    default: return -1;
  }
}

}  // extern "C"
