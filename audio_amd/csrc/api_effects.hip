// SoX-style effects of the C ABI (csrc/effects.h): exported constants, workspace query, overdrive, phaser, flanger.
#include "api_common.h"
#include "effects.h"

using namespace aamd;

namespace {

int elem_size(int32_t dtype) { return dtype == AAMD_SA_F64 ? 8 : (dtype == AAMD_SA_F32 ? 4 : 2); }
int comp_size(int32_t dtype) { return dtype == AAMD_SA_F64 ? 8 : 4; }
bool ring_fits(int32_t dtype, int64_t L) {
  return dtype == AAMD_SA_F64 ? fx::ring_in_lds<double>(L) : fx::ring_in_lds<float>(L);
}

template <int DT, bool FLANGER>
int delay_launch(const fx::DelayArgs& a, hipStream_t s) {
  using C = typename wa::Elem<DT>::C;
  const int64_t groups = fx::n_groups(a.rows);
  if (fx::ring_in_lds<C>(a.L)) {
    const size_t lds = (size_t)(fx::tile_bytes<C>() + fx::ring_bytes<C>(a.L));
    if (lds > 48 * 1024 && lds > dev_props().lds_per_block_optin)
      return fail(AAMD_EUNSUPPORTED, "audio_amd: effects: this device has less LDS than the delay ring was planned for");
    return launch(fx::delay_kernel<DT, FLANGER, true>, groups, fx::kRows, lds, s, a);
  }
  return launch(fx::delay_kernel<DT, FLANGER, false>, groups, fx::kRows, (size_t)fx::tile_bytes<C>(), s, a);
}

template <bool FLANGER>
int delay_dispatch(int32_t dtype, const fx::DelayArgs& a, hipStream_t s) {
  switch (dtype) {
    case AAMD_SA_F32: return delay_launch<wa::kF32, FLANGER>(a, s);
    case AAMD_SA_F64: return delay_launch<wa::kF64, FLANGER>(a, s);
    case AAMD_SA_F16: return delay_launch<wa::kF16, FLANGER>(a, s);
    default: return delay_launch<wa::kBF16, FLANGER>(a, s);
  }
}

template <int DT>
int overdrive_launch(const fx::OdArgs& a, hipStream_t s) {
  const int64_t blocks = a.rows * a.chunks;
  if (a.chunks > 1) {
    const int rc = launch(fx::overdrive_reduce_kernel<DT>, blocks, fx::kOdThreads, 0, s, a);
    if (rc != AAMD_OK) return rc;
  }
  return launch(fx::overdrive_apply_kernel<DT>, blocks, fx::kOdThreads, 0, s, a);
}

int check_rows(const char* what, int32_t dtype, const void* x, const void* out, int64_t rows, int64_t length,
               int64_t row_stride) {
  AAMD_CHECK_ARG(dtype >= AAMD_SA_F32 && dtype <= AAMD_SA_BF16, std::string(what) + ": unknown element type");
  AAMD_CHECK_ARG(rows >= 0 && length >= 0 && row_stride >= 0, std::string(what) + ": bad sizes");
  AAMD_CHECK_ARG(rows < (1ll << 31) && length < (1ll << 40), std::string(what) + ": too many rows or samples");
  if (rows == 0 || length == 0) return AAMD_OK;
  AAMD_CHECK_ARG(x && out, "null buffer");
  AAMD_CHECK_ARG((((uintptr_t)x | (uintptr_t)out) & (uintptr_t)(elem_size(dtype) - 1)) == 0,
                 std::string(what) + ": a buffer is not aligned to its element");
  return AAMD_OK;
}

}  // namespace

extern "C" {

int32_t aamd_effects_tiles(int32_t which) {
  return which == 0 ? fx::kRows : (which == 1 ? fx::kTile : (which == 2 ? fx::kOdChunk : 0));
}

int64_t aamd_effects_workspace(int32_t effect, int32_t dtype, int64_t rows, int64_t length, int64_t ring) {
  if (rows <= 0 || length <= 0 || dtype < AAMD_SA_F32 || dtype > AAMD_SA_BF16) return 0;
  if (effect == AAMD_FX_OVERDRIVE) return rows * fx::od_chunks(length) * 8;
  if (effect != AAMD_FX_PHASER && effect != AAMD_FX_FLANGER) return 0;
  if (ring < 1 || ring > fx::kFlangerMaxRing || ring_fits(dtype, ring)) return 0;
  return fx::n_groups(rows) * fx::kRows * ring * comp_size(dtype);
}

int aamd_overdrive(int32_t dtype, const void* x, void* out, void* workspace, int64_t rows, int64_t length,
                   int64_t row_stride, double gain, double colour, void* stream) {
  DeviceScope dev_scope_(x);
  const int rc0 = check_rows("overdrive", dtype, x, out, rows, length, row_stride);
  if (rc0 != AAMD_OK || rows == 0 || length == 0) return rc0;
  fx::OdArgs a{};
  a.x = x; a.out = out; a.ws = static_cast<double*>(workspace);
  a.rows = rows; a.T = length; a.sx = rows > 1 ? row_stride : 0; a.chunks = fx::od_chunks(length);
  a.gain = gain; a.colour = colour;
  AAMD_CHECK_ARG(rows * a.chunks < (1ll << 31), "overdrive: too many workgroups");
  AAMD_CHECK_ARG(a.chunks == 1 || (workspace && ((uintptr_t)workspace & 7) == 0), "overdrive: workspace missing or misaligned");
  hipStream_t s = (hipStream_t)stream;
  switch (dtype) {
    case AAMD_SA_F32: return overdrive_launch<wa::kF32>(a, s);
    case AAMD_SA_F64: return overdrive_launch<wa::kF64>(a, s);
    case AAMD_SA_F16: return overdrive_launch<wa::kF16>(a, s);
    default: return overdrive_launch<wa::kBF16>(a, s);
  }
}

int aamd_phaser(int32_t dtype, const void* x, void* out, void* workspace, int64_t rows, int64_t length, int64_t row_stride,
                const int32_t* table, int64_t table_len, int64_t ring, double gain_in, double gain_out, double decay,
                void* stream) {
  DeviceScope dev_scope_(x);
  static_assert(fx::kPhaserMaxRing == AAMD_PHASER_MAX_RING && fx::kFlangerMaxRing == AAMD_FLANGER_MAX_RING &&
                    fx::kMaxTable == AAMD_EFFECTS_MAX_TABLE, "the header's limits are the kernels'");
  const int rc0 = check_rows("phaser", dtype, x, out, rows, length, row_stride);
  if (rc0 != AAMD_OK) return rc0;
  AAMD_CHECK_ARG(ring >= 1 && table_len >= 1, "phaser: the delay ring and the modulation table need at least one entry");
  if (ring > AAMD_PHASER_MAX_RING) return fail(AAMD_EUNSUPPORTED, "audio_amd: phaser: the kernel serves delay rings up to 512 samples");
  if (table_len > AAMD_EFFECTS_MAX_TABLE)
    return fail(AAMD_EUNSUPPORTED, "audio_amd: phaser: the kernel serves modulation tables up to 2^24 entries");
  if (rows == 0 || length == 0) return AAMD_OK;
  AAMD_CHECK_ARG(table && ((uintptr_t)table & 3) == 0, "phaser: table missing or misaligned");
  AAMD_CHECK_ARG(ring_fits(dtype, ring) || (workspace && ((uintptr_t)workspace & 15) == 0),
                 "phaser: workspace missing or misaligned");
  fx::DelayArgs a{};
  a.x = x; a.out = out; a.ws = workspace; a.table = table;
  a.rows = rows; a.T = length; a.sx = rows > 1 ? row_stride : 0; a.M = table_len;
  a.g0 = gain_in; a.g1 = decay; a.g2 = gain_out;
  a.L = (int32_t)ring; a.channels = 1; a.quadratic = 0;
  return delay_dispatch<false>(dtype, a, (hipStream_t)stream);
}

int aamd_flanger(int32_t dtype, const void* x, void* out, void* workspace, int64_t rows, int64_t length, int64_t row_stride,
                 int32_t channels, const float* table, int64_t table_len, const int64_t* channel_phase, int64_t ring,
                 double feedback_gain, double in_gain, double delay_gain, int32_t quadratic, int32_t general, void* stream) {
  DeviceScope dev_scope_(x);
  const int rc0 = check_rows("flanger", dtype, x, out, rows, length, row_stride);
  if (rc0 != AAMD_OK) return rc0;
  AAMD_CHECK_ARG(channels >= 1 && channels <= fx::kMaxChannels && channel_phase, "flanger: 1 to 4 channels");
  AAMD_CHECK_ARG(rows % channels == 0, "flanger: rows must be a multiple of channels");
  AAMD_CHECK_ARG(ring >= 2 && table_len >= 1, "flanger: the delay ring needs two entries and the modulation table one");
  if (ring > AAMD_FLANGER_MAX_RING)
    return fail(AAMD_EUNSUPPORTED, "audio_amd: flanger: the kernels serve delay rings up to 4096 samples");
  if (table_len > AAMD_EFFECTS_MAX_TABLE)
    return fail(AAMD_EUNSUPPORTED, "audio_amd: flanger: the kernels serve modulation tables up to 2^24 entries");
  if (rows == 0 || length == 0) return AAMD_OK;
  AAMD_CHECK_ARG(table && ((uintptr_t)table & 3) == 0, "flanger: table missing or misaligned");
  fx::DelayArgs a{};
  a.x = x; a.out = out; a.ws = workspace; a.table = table;
  a.rows = rows; a.T = length; a.sx = rows > 1 ? row_stride : 0; a.M = table_len;
  for (int c = 0; c < channels; ++c) {
    AAMD_CHECK_ARG(channel_phase[c] >= 0, "flanger: negative channel phase");
    a.cph[c] = channel_phase[c];
  }
  a.g0 = feedback_gain; a.g1 = in_gain; a.g2 = delay_gain;
  a.L = (int32_t)ring; a.channels = channels; a.quadratic = quadratic ? 1 : 0;
  hipStream_t s = (hipStream_t)stream;
  if (feedback_gain == 0.0 && !general) {
    const int64_t chunks = wa::n_chunks(length);
    AAMD_CHECK_ARG(rows * chunks < (1ll << 31), "flanger: too many workgroups");
    switch (dtype) {
      case AAMD_SA_F32: return launch(fx::stream_kernel<wa::kF32>, rows * chunks, wa::kThreads, 0, s, a, chunks);
      case AAMD_SA_F64: return launch(fx::stream_kernel<wa::kF64>, rows * chunks, wa::kThreads, 0, s, a, chunks);
      case AAMD_SA_F16: return launch(fx::stream_kernel<wa::kF16>, rows * chunks, wa::kThreads, 0, s, a, chunks);
      default: return launch(fx::stream_kernel<wa::kBF16>, rows * chunks, wa::kThreads, 0, s, a, chunks);
    }
  }
  AAMD_CHECK_ARG(ring_fits(dtype, ring) || (workspace && ((uintptr_t)workspace & 15) == 0),
                 "flanger: workspace missing or misaligned");
  return delay_dispatch<true>(dtype, a, s);
}

}  // extern "C"
