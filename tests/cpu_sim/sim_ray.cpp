// CPU replay of the ray-tracing kernels (audio_amd/csrc/ray_trace.h compiled with g++, no GPU): the driver mirrors
// trace_kernel and convert_kernel, "all threads run phase X, then __syncthreads()" replaced by a loop over thread ids, the
// barrier-wide OR by a loop, and the 64-bit atomic add by a plain add (integer addition commutes: the order of the lanes
// cannot show), with the launch geometry of the C ABI.  TEST INFRASTRUCTURE ONLY.
#include <cstdint>
#include <cmath>

#include "../../audio_amd/csrc/ray_trace.h"

using namespace aamd;

namespace {

struct PlainSink {
  long long* acc;
  int64_t size;
  int64_t adds = 0, outside = 0;
  void add(int64_t idx, long long q) {
    ++adds;
    if (idx < 0 || idx >= size) {                                        // the kernel's bound checks failed: reported, not written
      ++outside;
      return;
    }
    acc[idx] = (long long)((unsigned long long)acc[idx] + (unsigned long long)q);
  }
};

template <int DT>
bool prologue(const ray::Args& a, int64_t b, ray::Room& rm) {           // the head of both kernels
  for (int tid = 0; tid < ray::kThreads; ++tid) ray::load_room<DT>(tid, ray::kThreads, a, b, rm);
  bool bad = false;
  for (int tid = 0; tid < ray::kThreads; ++tid) bad = ray::room_bad_part(tid, ray::kThreads, a, rm) || bad;
  return bad;
}

template <int DT, int D, int NBC>
void trace(const ray::Args& a, PlainSink& sink) {                       // trace_kernel
  for (int64_t blk = 0; blk < a.B * a.blocks_per_room; ++blk) {
    const int64_t b = blk / a.blocks_per_room, run = blk - b * a.blocks_per_room;
    ray::Room rm{};
    if (prologue<DT>(a, b, rm)) continue;
    for (int tid = 0; tid < ray::kThreads; ++tid) {
      const int64_t i = run * ray::kThreads + tid;
      if (i >= a.N) continue;
      ray::trace_ray<D, NBC>(a, rm, b, i, (int)ray::bounce_bound(a, rm), sink);
    }
  }
}

template <int DT, int D>
void trace_bands(const ray::Args& a, PlainSink& sink) {
  switch (ray::band_class(a.NB)) {
    case 1: trace<DT, D, 1>(a, sink); break;
    case 4: trace<DT, D, 4>(a, sink); break;
    default: trace<DT, D, 8>(a, sink); break;
  }
}

template <int DT>
void run(ray::Args a, PlainSink& sink) {
  a.blocks_per_room = (a.N + ray::kThreads - 1) / ray::kThreads;
  if (a.D == 2) trace_bands<DT, 2>(a, sink);
  else trace_bands<DT, 3>(a, sink);
  const int64_t per_room = (int64_t)a.M * a.NB * a.bins;
  a.blocks_per_room = (per_room + ray::kThreads - 1) / ray::kThreads;
  for (int64_t blk = 0; blk < a.B * a.blocks_per_room; ++blk) {        // convert_kernel
    const int64_t b = blk / a.blocks_per_room, part = blk - b * a.blocks_per_room;
    ray::Room rm{};
    const bool bad = prologue<DT>(a, b, rm);
    for (int tid = 0; tid < ray::kThreads; ++tid) ray::convert<DT>(a, b, per_room, part * ray::kThreads + tid, bad);
  }
}

}  // namespace

extern "C" {

int sim_ray_tiles(int which) {
  const int t[7] = {ray::kThreads, ray::kMaxBands, ray::kMaxMics, ray::kMaxRays, ray::kMaxBins, ray::kMaxBounces, ray::kHeadroom};
  return which >= 0 && which < 7 ? t[which] : 0;
}

// the buffers of aamd_ray_trace on the host; < 0 on an argument the C ABI refuses; stats[0] = adds, stats[1] = adds whose
// index fell outside the accumulator (must be 0)
int sim_ray(int dtype, const void* room, const void* source, const void* mic, const void* absorption, const void* scattering,
            int64_t* acc, void* out, int64_t B, int64_t M, int D, int NB, int64_t N, int64_t bins, int k, double mic_radius,
            double sound_speed, double energy_thres, double time_thres, double hist_bin_size, int64_t* stats) {
  if ((dtype != ray::kF32 && dtype != ray::kF64) || (D != 2 && D != 3) || B < 0 || M < 0 || NB < 1 || N < 1 || bins < 1) return -1;
  if (!(mic_radius > 0 && sound_speed > 0 && energy_thres > 0 && time_thres > 0 && hist_bin_size > 0) || k < -1000 || k > 1000) return -1;
  if (NB > ray::kMaxBands || M > ray::kMaxMics || N > ray::kMaxRays || bins > ray::kMaxBins) return -2;
  ray::Args a{};
  a.room = room; a.source = source; a.mic = mic; a.absorption = absorption; a.scattering = scattering;
  a.acc = reinterpret_cast<long long*>(acc); a.out = out;
  a.B = B; a.N = N; a.bins = bins;
  a.e0 = 2.0 / (double)N; a.s_max = time_thres * sound_speed; a.r2 = mic_radius * mic_radius;
  a.w_bin = sound_speed * hist_bin_size; a.energy_thres = energy_thres; a.scale = std::ldexp(1.0, k);
  a.D = D; a.M = (int32_t)M; a.NB = NB; a.k = k;
  PlainSink sink{a.acc, B * M * NB * bins};
  if (dtype == ray::kF64) run<ray::kF64>(a, sink);
  else run<ray::kF32>(a, sink);
  stats[0] = sink.adds;
  stats[1] = sink.outside;
  return 0;
}

}  // extern "C"
