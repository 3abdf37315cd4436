// CPU replay of the voice-activity kernels (audio_amd/csrc/vad.h compiled with g++, no GPU): each driver mirrors its
// __global__ kernel, "all threads run phase X, then __syncthreads()" replaced by a loop over thread ids, with the launch
// geometry and the workspace layout of the C ABI.  TEST INFRASTRUCTURE ONLY.
#include <cstdint>
#include <vector>

#include "../../audio_amd/csrc/vad.h"

using namespace aamd;

template <int DT>
static void spec(const vad::MeasArgs& a) {                          // spec_kernel
  std::vector<float> lds(2 * (size_t)vad::plane(a.N));
  float* re = lds.data();
  float* im = re + vad::plane(a.N);
  for (int64_t blk = 0; blk < a.rows * a.frames; ++blk) {
    const int64_t row = blk / a.frames, f = blk - row * a.frames;
    for (int tid = 0; tid < vad::kThreads; ++tid) vad::frame_load<DT>(tid, a, row, f, re, im);
    for (int s = 0; s < a.logN; ++s)
      for (int tid = 0; tid < vad::kThreads; ++tid) vad::fft_stage(tid, a.N, s, a.tw, a.logN, re, im);
    for (int tid = 0; tid < vad::kThreads; ++tid) vad::spec_write(tid, a, row, f, re, im);
  }
}

static void smooth(const vad::MeasArgs& a) {                        // smooth_kernel
  const int nb = a.s1 - a.s0;
  for (int64_t q = 0; q < a.rows * nb; ++q) vad::smooth_thread(a, q / nb, (int)(q % nb));
}

static void ceps(const vad::MeasArgs& a) {                          // ceps_kernel
  const int n2 = a.N >> 1;
  std::vector<float> lds(2 * (size_t)vad::plane(n2)), red(vad::kThreads);
  float* re = lds.data();
  float* im = re + vad::plane(n2);
  for (int64_t blk = 0; blk < a.rows * a.frames; ++blk) {
    const int64_t row = blk / a.frames, f = blk - row * a.frames;
    for (int tid = 0; tid < vad::kThreads; ++tid) vad::ceps_load(tid, a, row, f, re, im);
    for (int s = 0; s < a.logN - 1; ++s)
      for (int tid = 0; tid < vad::kThreads; ++tid) vad::fft_stage(tid, n2, s, a.tw, a.logN, re, im);
    for (int tid = 0; tid < vad::kThreads; ++tid) red[tid] = vad::ceps_partial(tid, a, re, im);
    for (int stride = vad::kThreads >> 1; stride > 0; stride >>= 1)
      for (int tid = 0; tid < vad::kThreads; ++tid) vad::sum_step(tid, stride, red.data());
    a.meas[row * a.frames + f] = vad::measure_of(red[0], a.c1 - a.c0);
  }
}

extern "C" {

int sim_vad_tiles(int which) {
  return which == 0 ? vad::kThreads : (which == 1 ? vad::kMaxN : (which == 2 ? vad::kMinN : vad::kTrigThreads));
}
int64_t sim_vad_frames(int64_t T, int64_t L, int64_t P) { return vad::n_frames(T, L, P); }

// tables: w[L], cw[s1 - s0], tw[N]; ws: rows * frames * (s1 - s0) floats; meas: rows * frames.  < 0 on a bad argument.
int sim_vad_measure(int dtype, const void* x, int64_t rows, int64_t T, int64_t sx, int L, int N, int P, int s0, int s1, int c0,
                    int c1, int boot_max, double smooth_mult, double up, double down, double nra, const float* tables, float* ws,
                    float* meas) {
  if (N < vad::kMinN || N > vad::kMaxN || (N & (N - 1)) || L < 1 || L > N || s0 < 1 || s0 >= s1 || s1 > N / 2 || c0 < 0 ||
      c0 >= c1 || c1 > N / 4)
    return -2;
  vad::MeasArgs a{};
  a.x = x; a.w = tables; a.cw = tables + L; a.tw = tables + L + (s1 - s0); a.d = ws; a.meas = meas;
  a.rows = rows; a.T = T; a.sx = rows > 1 ? sx : 0; a.frames = vad::n_frames(T, L, P);
  a.smooth = smooth_mult; a.up = (float)up; a.down = (float)down; a.nra = (float)nra;
  a.L = L; a.N = N; a.logN = 0;
  while ((1 << a.logN) < N) ++a.logN;
  a.P = P; a.s0 = s0; a.s1 = s1; a.c0 = c0; a.c1 = c1; a.boot_max = boot_max;
  if (rows == 0 || a.frames == 0) return 0;
  switch (dtype) {
    case wa::kF32: spec<wa::kF32>(a); break;
    case wa::kF64: spec<wa::kF64>(a); break;
    case wa::kF16: spec<wa::kF16>(a); break;
    case wa::kBF16: spec<wa::kBF16>(a); break;
    default: return -1;
  }
  smooth(a);
  ceps(a);
  return 0;
}

int sim_vad_trigger(const float* meas, int64_t rows, int64_t frames, int64_t M, int64_t gap, int64_t P, int64_t fixed,
                    double level, double trig, int64_t* first, int64_t* start, int64_t* joint) {
  vad::TrigArgs a{};
  a.meas = meas; a.rows = rows; a.frames = frames; a.M = M; a.gap = gap; a.P = P; a.fixed = fixed;
  a.level = level; a.trig = trig; a.first = first; a.start = start; a.joint = joint;
  for (int64_t blk = 0; blk < (rows + vad::kTrigThreads - 1) / vad::kTrigThreads; ++blk)      // trigger_kernel
    for (int tid = 0; tid < vad::kTrigThreads; ++tid)
      if (blk * vad::kTrigThreads + tid < rows) vad::trigger_row(a, blk * vad::kTrigThreads + tid);
  if (!joint) return 0;
  std::vector<int64_t> sf(vad::kThreads), sr(vad::kThreads);                                  // joint_kernel
  for (int tid = 0; tid < vad::kThreads; ++tid) vad::joint_scan(tid, a, sf[tid], sr[tid]);
  for (int stride = vad::kThreads >> 1; stride > 0; stride >>= 1)
    for (int tid = 0; tid < vad::kThreads; ++tid) vad::joint_min_step(tid, stride, sf.data(), sr.data());
  const int64_t f = sf[0], r0 = sr[0];
  if (f == vad::kNone) {
    joint[0] = -1;
    return 0;
  }
  for (int tid = 0; tid < vad::kThreads; ++tid) sf[tid] = vad::joint_flush(tid, a, f, r0);
  for (int stride = vad::kThreads >> 1; stride > 0; stride >>= 1)
    for (int tid = 0; tid < vad::kThreads; ++tid) vad::joint_max_step(tid, stride, sf.data());
  joint[0] = vad::start_of(a, f, sf[0]);
  return 0;
}

}  // extern "C"
