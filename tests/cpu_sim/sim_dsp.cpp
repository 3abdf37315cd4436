// CPU replay of the synthesis kernels (audio_amd/csrc/dsp_synth.h compiled with g++, no GPU): each driver mirrors its
// kernel, "all threads run phase X, then __syncthreads()" replaced by a loop over thread ids, with the launch geometry and
// the LDS layout of the C ABI.  TEST INFRASTRUCTURE ONLY.
#include <cstdint>
#include <vector>

#include "../../audio_amd/csrc/dsp_synth.h"

using namespace aamd;

template <int DT>
static void run_osc(const dsp::OscArgs& a) {                           // osc_sums_kernel, then osc_apply_kernel
  using C = typename wa::Elem<DT>::C;
  const dsp::OscGeom g = dsp::osc_geom(a.N);
  std::vector<double> sub(dsp::kThreads), start(dsp::kThreads), run(dsp::kThreads);
  std::vector<C> vals(2 * dsp::kOscLdsValues);
  for (int64_t blk = 0; a.chunks > 1 && blk < a.rows * (a.chunks - 1); ++blk) {
    const int64_t row = blk / (a.chunks - 1), chunk = blk - row * (a.chunks - 1);
    for (int tid = 0; tid < dsp::kThreads; ++tid) sub[tid] = dsp::osc_slice_sum<DT>(tid, a, g, row, chunk);
    for (int tid = 0; tid < dsp::kThreads; ++tid) dsp::osc_chunk_sum(tid, a, g, row, chunk, sub.data());
  }
  for (int64_t blk = 0; blk < a.rows * a.chunks; ++blk) {
    const int64_t row = blk / a.chunks, chunk = blk - row * a.chunks;
    for (int tid = 0; tid < dsp::kThreads; ++tid) {
      sub[tid] = dsp::osc_slice_sum<DT>(tid, a, g, row, chunk);
      dsp::osc_start(tid, a, row, chunk, start.data());
    }
    for (int tid = 0; tid < dsp::kThreads; ++tid) run[tid] = dsp::osc_base(tid, a, g, start.data(), sub.data());
    for (int s0 = 0; s0 < g.S; s0 += g.SB) {
      for (int tid = 0; tid < dsp::kThreads; ++tid) dsp::osc_steps<DT>(tid, a, g, row, chunk, s0, run[tid], vals.data());
      if (a.reduction != dsp::kNone)
        for (int tid = 0; tid < dsp::kThreads; ++tid) dsp::osc_reduce<DT>(tid, a, g, row, chunk, s0, vals.data());
    }
  }
}

template <int DT>
static void run_fw(const dsp::FwArgs& a) {                             // fw_kernel
  using C = typename wa::Elem<DT>::C;
  std::vector<C> xs(dsp::fw_lds_values(a.L));
  for (int64_t blk = 0; blk < a.rows * a.tiles; ++blk) {
    const int64_t row = blk / a.tiles, tile = blk - row * a.tiles;
    for (int tid = 0; tid < dsp::kThreads; ++tid) dsp::fw_stage<DT>(tid, a, row, tile, xs.data());
    for (int tid = 0; tid < dsp::kThreads; ++tid) dsp::fw_outputs<DT>(tid, a, row, tile, xs.data());
  }
}

template <int DT>
static void run_sinc(const dsp::SincArgs& a) {                         // sinc_kernel
  std::vector<double> part(2 * dsp::kThreads);
  for (int64_t row = 0; row < a.rows; ++row) {
    for (int tid = 0; tid < dsp::kThreads; ++tid) dsp::sinc_partial<DT>(tid, a, row, part.data());
    for (int tid = 0; tid < dsp::kThreads; ++tid) dsp::sinc_write<DT>(tid, a, row, part.data());
  }
}

template <int DT>
static void run_fir(const dsp::FirArgs& a) {                           // fir_kernel
  using C = typename wa::Elem<DT>::C;
  std::vector<C> lds((size_t)a.n + 2 * ((size_t)a.n - 1));
  for (int64_t row = 0; row < a.rows; ++row) {
    for (int tid = 0; tid < dsp::kThreads; ++tid) dsp::fir_stage<DT>(tid, a, row, lds.data());
    for (int tid = 0; tid < dsp::kThreads; ++tid) dsp::fir_write<DT>(tid, a, row, lds.data());
  }
}

template <int DT>
static void run_pitch(const dsp::PitchArgs& a) {                       // pitch_kernel
  for (int64_t i = 0; i < (a.M * a.N + dsp::kThreads - 1) / dsp::kThreads * dsp::kThreads; ++i) dsp::pitch_one<DT>(a, i);
}

#define SIM_DISPATCH(dtype, F, a)                 \
  switch (dtype) {                                \
    case wa::kF32: F<wa::kF32>(a); break;         \
    case wa::kF64: F<wa::kF64>(a); break;         \
    case wa::kF16: F<wa::kF16>(a); break;         \
    case wa::kBF16: F<wa::kBF16>(a); break;       \
    default: return -1;                           \
  }

extern "C" {

int sim_dsp_tiles(int which) {
  const int v[5] = {dsp::kOscChunk, dsp::kFwTile, dsp::kMaxTaps, dsp::kMaxOsc, dsp::kMaxMags};
  return which >= 0 && which < 5 ? v[which] : 0;
}

// the LDS values an oscillator launch of N oscillators uses, and what the kernel reserves
int sim_osc_lds(int N) { return N >= 1 && N <= dsp::kMaxOsc ? dsp::osc_lds_values(N) : -1; }
int sim_osc_lds_reserved() { return dsp::kOscLdsValues; }

// the buffers of the C ABI on the host; -1 on an argument it refuses, -2 beyond a limit
int sim_oscillator_bank(int dtype, const void* freq, const void* amp, void* out, int64_t rows, int64_t T, int64_t N, int64_t sf,
                        int64_t sa, double sample_rate, int reduction) {
  if (rows < 0 || T < 0 || N < 0 || reduction < 0 || reduction > 2) return -1;
  if (N > dsp::kMaxOsc) return -2;
  if (rows == 0 || T == 0 || N == 0) return 0;
  dsp::OscArgs a{};
  a.chunks = (T + dsp::kOscChunk - 1) / dsp::kOscChunk;
  std::vector<double> ws((size_t)(rows * a.chunks * N), -7.0);
  a.freq = freq; a.amp = amp; a.out = out; a.sums = ws.data();
  a.rows = rows; a.T = T; a.sf = sf; a.sa = sa; a.sample_rate = sample_rate; a.N = (int32_t)N; a.reduction = reduction;
  SIM_DISPATCH(dtype, run_osc, a)
  return 0;
}

int sim_filter_waveform(int dtype, const void* x, const void* h, void* out, int64_t rows, int64_t T, int64_t sx, int64_t F, int L,
                        int batched) {
  if (rows < 0 || T < 0 || F < 1 || L < 1 || T % F) return -1;
  if (L > dsp::kMaxTaps) return -2;
  if (rows == 0 || T == 0) return 0;
  dsp::FwArgs a{};
  a.x = x; a.h = h; a.out = out; a.rows = rows; a.T = T; a.sx = sx; a.F = F; a.C = T / F;
  a.tiles = (T + dsp::kFwTile - 1) / dsp::kFwTile; a.L = L; a.batched = batched;
  SIM_DISPATCH(dtype, run_fw, a)
  return 0;
}

int sim_sinc_impulse_response(int dtype, const void* cutoff, void* out, int64_t rows, int W, int high_pass) {
  if (W < 1 || !(W & 1) || rows < 0) return -1;
  dsp::SincArgs a{};
  a.cutoff = cutoff; a.out = out; a.rows = rows; a.W = W; a.high_pass = high_pass;
  if (dtype == wa::kF64) run_sinc<wa::kF64>(a);
  else if (dtype == wa::kF32) run_sinc<wa::kF32>(a);
  else return -1;
  return 0;
}

int sim_frequency_impulse_response(int dtype, const void* mags, const void* table, void* out, int64_t rows, int n) {
  if (n < 2 || rows < 0) return -1;
  if (n > dsp::kMaxMags) return -2;
  dsp::FirArgs a{};
  a.mags = mags; a.table = table; a.out = out; a.rows = rows; a.n = n;
  if (dtype == wa::kF64) run_fir<wa::kF64>(a);
  else if (dtype == wa::kF32) run_fir<wa::kF32>(a);
  else return -1;
  return 0;
}

int sim_extend_pitch(int dtype, const void* base, const void* pattern, void* out, int64_t M, int64_t N) {
  if (M < 0 || N < 0) return -1;
  dsp::PitchArgs a{};
  a.base = base; a.pattern = pattern; a.out = out; a.M = M; a.N = N;
  SIM_DISPATCH(dtype, run_pitch, a)
  return 0;
}

}  // extern "C"
