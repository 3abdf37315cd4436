// Image-source room impulse responses of the C ABI (csrc/rir.h): exported constants and the one launch.
#include "api_common.h"
#include "rir.h"

using namespace aamd;

extern "C" {

int32_t aamd_rir_tiles(int32_t which) {
  static_assert(rir::kMaxFl == AAMD_RIR_MAX_FILTER && rir::kMaxOrder == AAMD_RIR_MAX_ORDER, "the header's limits are the kernel's");
  static_assert(rir::kF32 == AAMD_SA_F32 && rir::kF64 == AAMD_SA_F64, "the element codes are the header's");
  return which == 0 ? rir::kTile : (which == 1 ? rir::kChunk : (which == 2 ? rir::kMaxFl : (which == 3 ? rir::kMaxOrder : 0)));
}

int aamd_simulate_rir(int32_t dtype, const void* room, const void* source, const void* mic, const void* absorption,
                      const int16_t* lattice, int64_t n_img, void* out, int64_t batch, int64_t mics, int32_t dims,
                      int32_t max_order, int32_t filter_len, int64_t out_len, double sample_rate, double sound_speed,
                      void* stream) {
  DeviceScope dev_scope_(out);
  AAMD_CHECK_ARG(dtype == AAMD_SA_F32 || dtype == AAMD_SA_F64, "simulate_rir: the element type must be float32 or float64");
  AAMD_CHECK_ARG(dims == 2 || dims == 3, "simulate_rir: rooms have 2 or 3 dimensions");
  AAMD_CHECK_ARG(max_order >= 0 && filter_len >= 3 && (filter_len & 1), "simulate_rir: max_order >= 0 and an odd filter of 3 or more taps");
  if (max_order > AAMD_RIR_MAX_ORDER) return fail(AAMD_EUNSUPPORTED, "audio_amd: simulate_rir: the kernel serves max_order up to 64");
  if (filter_len > AAMD_RIR_MAX_FILTER)
    return fail(AAMD_EUNSUPPORTED, "audio_amd: simulate_rir: the kernel serves delay filters up to 1025 taps");
  AAMD_CHECK_ARG(batch >= 0 && mics >= 0 && out_len >= 1 && n_img >= 1, "simulate_rir: bad sizes");
  AAMD_CHECK_ARG(out_len < (1ll << 31) - rir::kTile - AAMD_RIR_MAX_FILTER && n_img < (1ll << 31), "simulate_rir: too many samples or images");
  const int64_t o = max_order, images = dims == 2 ? 2 * o * o + 2 * o + 1 : (2 * o + 1) * (2 * o * o + 2 * o + 3) / 3;
  AAMD_CHECK_ARG(n_img == images, "simulate_rir: the lattice table is not that of max_order and the dimensions");
  if (batch == 0 || mics == 0) return AAMD_OK;
  const int64_t tiles = (out_len + rir::kTile - 1) / rir::kTile;
  AAMD_CHECK_ARG(batch < (1ll << 31) && mics < (1ll << 31) && batch * mics < (1ll << 31) && batch * mics * tiles < (1ll << 31),
                 "simulate_rir: too many workgroups");
  AAMD_CHECK_ARG(room && source && mic && absorption && lattice && out, "null buffer");
  const uintptr_t el = dtype == AAMD_SA_F64 ? 7 : 3;
  AAMD_CHECK_ARG((((uintptr_t)room | (uintptr_t)source | (uintptr_t)mic | (uintptr_t)absorption | (uintptr_t)out) & el) == 0 &&
                     ((uintptr_t)lattice & 1) == 0, "simulate_rir: a buffer is misaligned");
  rir::Args a{};
  a.room = room; a.source = source; a.mic = mic; a.absorption = absorption; a.lattice = lattice; a.out = out;
  a.B = batch; a.M = mics; a.L = out_len; a.n_img = n_img; a.tiles = tiles;
  a.sample_rate = sample_rate; a.sound_speed = sound_speed;
  a.D = dims; a.order = max_order; a.pad = filter_len / 2;
  hipStream_t s = (hipStream_t)stream;
  const size_t lds = rir::lds_bytes(a.order, a.pad);
  if (dtype == AAMD_SA_F64) return launch(rir::rir_kernel<rir::kF64>, batch * mics * tiles, rir::kThreads, lds, s, a);
  return launch(rir::rir_kernel<rir::kF32>, batch * mics * tiles, rir::kThreads, lds, s, a);
}

}  // extern "C"
