// Ray-traced energy histograms of the C ABI (csrc/ray_trace.h): exported constants, the trace launch and the convert launch.
#include "api_common.h"
#include "ray_trace.h"

using namespace aamd;

namespace {

template <int DT, int D>
int launch_trace(const ray::Args& a, int64_t blocks, hipStream_t s) {
  switch (ray::band_class(a.NB)) {
    case 1: return launch(ray::trace_kernel<DT, D, 1>, blocks, ray::kThreads, 0, s, a);
    case 4: return launch(ray::trace_kernel<DT, D, 4>, blocks, ray::kThreads, 0, s, a);
    default: return launch(ray::trace_kernel<DT, D, 8>, blocks, ray::kThreads, 0, s, a);
  }
}

template <int DT>
int launch_both(ray::Args a, hipStream_t s) {
  a.blocks_per_room = (a.N + ray::kThreads - 1) / ray::kThreads;
  const int rc = a.D == 2 ? launch_trace<DT, 2>(a, a.B * a.blocks_per_room, s) : launch_trace<DT, 3>(a, a.B * a.blocks_per_room, s);
  if (rc != AAMD_OK) return rc;
  a.blocks_per_room = ((int64_t)a.M * a.NB * a.bins + ray::kThreads - 1) / ray::kThreads;
  return launch(ray::convert_kernel<DT>, a.B * a.blocks_per_room, ray::kThreads, 0, s, a);
}

}  // namespace

extern "C" {

int32_t aamd_ray_tiles(int32_t which) {
  static_assert(ray::kMaxBands == AAMD_RAY_MAX_BANDS && ray::kMaxMics == AAMD_RAY_MAX_MICS && ray::kMaxRays == AAMD_RAY_MAX_RAYS &&
                    ray::kMaxBins == AAMD_RAY_MAX_BINS && ray::kMaxBounces == AAMD_RAY_MAX_BOUNCES &&
                    ray::kHeadroom == AAMD_RAY_HEADROOM, "the header's limits are the kernel's");
  static_assert(ray::kF32 == AAMD_SA_F32 && ray::kF64 == AAMD_SA_F64, "the element codes are the header's");
  switch (which) {
    case 0: return ray::kThreads;
    case 1: return ray::kMaxBands;
    case 2: return ray::kMaxMics;
    case 3: return ray::kMaxRays;
    case 4: return ray::kMaxBins;
    case 5: return ray::kMaxBounces;
    case 6: return ray::kHeadroom;
    default: return 0;
  }
}

int aamd_ray_trace(int32_t dtype, const void* room, const void* source, const void* mic, const void* absorption,
                   const void* scattering, int64_t* acc, void* out, int64_t batch, int64_t mics, int32_t dims, int32_t bands,
                   int64_t num_rays, int64_t num_bins, int32_t scale_log2, double mic_radius, double sound_speed,
                   double energy_thres, double time_thres, double hist_bin_size, void* stream) {
  DeviceScope dev_scope_(out);
  AAMD_CHECK_ARG(dtype == AAMD_SA_F32 || dtype == AAMD_SA_F64, "ray_trace: the element type must be float32 or float64");
  AAMD_CHECK_ARG(dims == 2 || dims == 3, "ray_trace: rooms have 2 or 3 dimensions");
  AAMD_CHECK_ARG(batch >= 0 && mics >= 0 && bands >= 1 && num_rays >= 1 && num_bins >= 1, "ray_trace: bad sizes");
  AAMD_CHECK_ARG(mic_radius > 0 && sound_speed > 0 && energy_thres > 0 && time_thres > 0 && hist_bin_size > 0 &&
                     mic_radius < INFINITY && sound_speed < INFINITY && energy_thres < INFINITY && time_thres < INFINITY &&
                     hist_bin_size < INFINITY, "ray_trace: the radius, the speed, the thresholds and the bin size must be positive and finite");
  AAMD_CHECK_ARG(scale_log2 >= -1000 && scale_log2 <= 1000, "ray_trace: the scale's exponent must lie in [-1000, 1000]");
  if (bands > AAMD_RAY_MAX_BANDS) return fail(AAMD_EUNSUPPORTED, "audio_amd: ray_trace: the kernel serves up to 8 bands");
  if (mics > AAMD_RAY_MAX_MICS) return fail(AAMD_EUNSUPPORTED, "audio_amd: ray_trace: the kernel serves up to 16 microphones");
  if (num_rays > AAMD_RAY_MAX_RAYS) return fail(AAMD_EUNSUPPORTED, "audio_amd: ray_trace: the kernel serves up to 2^24 rays");
  if (num_bins > AAMD_RAY_MAX_BINS) return fail(AAMD_EUNSUPPORTED, "audio_amd: ray_trace: the kernel serves up to 65536 bins");
  if (batch == 0 || mics == 0) return AAMD_OK;
  const int64_t per_room = mics * bands * num_bins;              // <= 2^23
  AAMD_CHECK_ARG(batch < (1ll << 31) / ((num_rays + ray::kThreads - 1) / ray::kThreads) &&
                     batch < (1ll << 31) / ((per_room + ray::kThreads - 1) / ray::kThreads), "ray_trace: too many workgroups");
  AAMD_CHECK_ARG(room && source && mic && absorption && scattering && acc && out, "null buffer");
  const uintptr_t el = dtype == AAMD_SA_F64 ? 7 : 3;
  AAMD_CHECK_ARG((((uintptr_t)room | (uintptr_t)source | (uintptr_t)mic | (uintptr_t)absorption | (uintptr_t)scattering |
                   (uintptr_t)out) & el) == 0 && ((uintptr_t)acc & 7) == 0, "ray_trace: a buffer is misaligned");
  ray::Args a{};
  a.room = room; a.source = source; a.mic = mic; a.absorption = absorption; a.scattering = scattering;
  a.acc = reinterpret_cast<long long*>(acc); a.out = out;
  a.B = batch; a.N = num_rays; a.bins = num_bins;
  a.e0 = 2.0 / (double)num_rays; a.s_max = time_thres * sound_speed; a.r2 = mic_radius * mic_radius;
  a.w_bin = sound_speed * hist_bin_size; a.energy_thres = energy_thres; a.scale = ldexp(1.0, scale_log2);
  a.D = dims; a.M = (int32_t)mics; a.NB = bands; a.k = scale_log2;
  hipStream_t s = (hipStream_t)stream;
  return dtype == AAMD_SA_F64 ? launch_both<ray::kF64>(a, s) : launch_both<ray::kF32>(a, s);
}

}  // extern "C"
