// CPU replay of the beamforming kernels (audio_amd/csrc/beamform.h compiled with g++, no GPU): each driver mirrors its
// __global__ kernel, "all threads run phase X, then __syncthreads()" replaced by a loop over thread ids, with the launch
// geometry of the C ABI.  TEST INFRASTRUCTURE ONLY.
#include <cstdint>
#include <vector>

#include "../../audio_amd/csrc/beamform.h"

using namespace aamd;

template <typename T, int NO>
static void psd_run(const bf::PsdArgs& a) {
  constexpr int TC = bf::TimeChunk<T>::v;
  std::vector<cplx<T>> tile(bf::kMaxC * TC * bf::kFP);
  std::vector<T> mtile(2 * TC * bf::kFP);
  std::vector<bf::PsdState<NO>> st(bf::kThreads);
  const int64_t tiles = bf::freq_tiles(a.F);
  for (int64_t blk = 0; blk < a.B * tiles; ++blk) {
    const int64_t b = blk / tiles, f0 = (blk - b * tiles) * bf::kFT;
    for (int tid = 0; tid < bf::kThreads; ++tid) bf::psd_init_thread<NO>(tid, a.C, st[tid]);
    for (int64_t t0 = 0; t0 < a.T; t0 += TC) {
      for (int tid = 0; tid < bf::kThreads; ++tid) bf::psd_load_thread<T>(tid, a, b, f0, t0, tile.data(), mtile.data());
      for (int tid = 0; tid < bf::kThreads; ++tid) bf::psd_accum_thread<T, NO>(tid, a, tile.data(), mtile.data(), st[tid]);
    }
    for (int tid = 0; tid < bf::kThreads; ++tid) bf::psd_store_thread<T, NO>(tid, a, b, f0, st[tid]);
  }
}

template <typename T>
static int psd_any(const bf::PsdArgs& a) {
  const int no = bf::outputs_per_thread(a.C);
  if (no <= 1) psd_run<T, 1>(a);
  else if (no <= 3) psd_run<T, 3>(a);
  else psd_run<T, 9>(a);
  return 0;
}

template <typename T>
static int weights_any(const bf::WArgs& a) {
  bf::Team s;
  const int C = a.C, W = a.C + a.K, L = bf::kTeam;
  for (int64_t bin = 0; bin < a.bins; ++bin) {
    for (int l = 0; l < L; ++l) bf::w_load<T>(l, a, bin, s);
    for (int k = 0; k < C; ++k) {
      const int p = bf::w_pivot(k, C, s);
      for (int l = 0; l < L; ++l) bf::w_swap(l, k, p, W, s);
      for (int l = 0; l < L; ++l) bf::w_eliminate(l, k, C, W, s);
    }
    for (int l = 0; l < L; ++l) bf::w_backsub(l, C, a.K, s);
    if (a.mode != bf::kRtfPower) {
      for (int l = 0; l < L; ++l) bf::w_finish<T>(l, a, bin, s);
      continue;
    }
    for (int l = 0; l < L; ++l) bf::w_power_start<T>(l, a, bin, s);
    for (int it = 0; it < a.n_iter - 2; ++it) {
      for (int l = 0; l < L; ++l) bf::w_power_step(l, C, s);
      for (int l = 0; l < L; ++l) bf::w_power_copy(l, C, s);
    }
    for (int l = 0; l < L; ++l) bf::w_power_finish<T>(l, a, bin, s);
  }
  return 0;
}

template <typename T>
static int apply_any(const bf::ApplyArgs& a) {
  std::vector<cplx<T>> wl(bf::kMaxC * bf::kWave * bf::ApplyVec<T>::v);
  const int U = bf::unit_tile<T>();
  const int64_t ut = bf::apply_unit_tiles(a.fmajor ? a.F : a.T, U), lt = bf::apply_line_tiles(a.fmajor ? a.T : a.F);
  for (int64_t blk0 = 0; blk0 < a.B * ut * lt; ++blk0) {
    int64_t blk = blk0;
    const int64_t iu = blk % ut;
    blk /= ut;
    const int64_t il = blk % lt, b = blk / lt;
    for (int tid = 0; tid < bf::kThreads; ++tid) bf::apply_weights_thread<T>(tid, a, b, iu * U, il * bf::kLines, wl.data());
    for (int tid = 0; tid < bf::kThreads; ++tid) bf::apply_thread<T>(tid, a, b, iu * U, il * bf::kLines, wl.data());
  }
  return 0;
}

static int fmajor_of(int64_t F, int64_t T, int64_t sf, int64_t st) { return st == 1 ? 0 : (sf == 1 ? 1 : (T <= 1 ? 0 : 1)); }

extern "C" {

int sim_bf_freq_tile() { return bf::kFT; }
int sim_bf_time_chunk() { return bf::kTCMax; }

// dims: B, C, F, T; xs: four strides of x in complex elements; m1s / m2s: three strides each
int sim_bf_psd(int dtype, const void* x, const int64_t* dims, const int64_t* xs, const void* m1, const int64_t* m1s,
               const void* m2, const int64_t* m2s, int normalize, double eps, void* out) {
  bf::PsdArgs a{};
  a.x = {x, xs[0], xs[1], xs[2], xs[3]};
  a.B = dims[0]; a.C = (int32_t)dims[1]; a.F = dims[2]; a.T = dims[3];
  a.fmajor = fmajor_of(a.F, a.T, xs[2], xs[3]);
  a.mask[0] = m1; a.mask[1] = m2;
  if (m1) { a.mb[0] = m1s[0]; a.mf[0] = m1s[1]; a.mt[0] = m1s[2]; }
  if (m2) { a.mb[1] = m2s[0]; a.mf[1] = m2s[1]; a.mt[1] = m2s[2]; }
  a.out = out; a.n_out = m2 ? 2 : 1; a.normalize = normalize; a.eps = eps;
  return dtype == bf::kC64 ? psd_any<float>(a) : psd_any<double>(a);
}

int sim_bf_weights(int dtype, int mode, const void* a_, const void* b, const void* u, void* out, int64_t batch, int64_t freq,
                   int C, int K, int ref, int loading, double diag_eps, double eps, int n_iter, int adjoint) {
  bf::WArgs a{};
  a.a = a_; a.b = b; a.u = ref >= 0 ? nullptr : u; a.out = out; a.bins = batch * freq; a.F = freq; a.C = C;
  a.K = mode == bf::kRtf ? 1 : (mode == bf::kSolve ? K : C);
  a.mode = mode; a.ref = ref >= 0 ? ref : -1; a.loading = loading; a.n_iter = n_iter; a.adjoint = adjoint;
  a.diag_eps = diag_eps; a.eps = eps;
  return dtype == bf::kC64 ? weights_any<float>(a) : weights_any<double>(a);
}

int sim_bf_apply(int dtype, const void* w, const void* x, const int64_t* dims, const int64_t* xs, void* out, const int64_t* os) {
  bf::ApplyArgs a{};
  a.w = w; a.x = {x, xs[0], xs[1], xs[2], xs[3]};
  a.B = dims[0]; a.C = (int32_t)dims[1]; a.F = dims[2]; a.T = dims[3];
  a.fmajor = fmajor_of(a.F, a.T, xs[2], xs[3]);
  a.out = out; a.ob = os[0]; a.of = os[1]; a.ot = os[2];
  return dtype == bf::kC64 ? apply_any<float>(a) : apply_any<double>(a);
}

}  // extern "C"
