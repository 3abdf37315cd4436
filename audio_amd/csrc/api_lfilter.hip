// IIR filter of the C ABI: wave-scan biquad cascades and the per-sequence direct form.
#include <cstdlib>

#include "api_common.h"
#include "lfilter.h"
#include "lfilter_wave.h"

using namespace aamd;

namespace {

template <int D>
int launch_lfilter(const float* x, const float* a, const float* b, float* y, int64_t n_seq,
                   int channels, int64_t length, int n_order, int n_rows, int n_stages, int clamp,
                   hipStream_t s) {
  using L = LfLds<D>;
  const size_t lds = L::bytes(n_stages);
  if (lds > 160 * 1024) return fail(AAMD_EUNSUPPORTED, "audio_amd: lfilter cascade too long for LDS");
  const int blocks = grid_for(n_seq, 1, dev_props().cu_count * 8);
  return launch(lfilter_kernel<D>, blocks, kLfThreads, lds, s, x, a, b, y, n_seq, channels, length, n_order, n_rows, n_stages,
                clamp);
}

// the lab build's environment overrides (tools only); the product build has none
int lfilter_lab() {
#ifdef AAMD_LAB
  static const int lab = [] { const char* e = std::getenv("AAMD_LFW_LAB"); return e ? std::atoi(e) : 0; }();
  return lab;
#else
  return 0;
#endif
}

// what a call runs on the current device: lfw::pick with this device's CU count and LDS opt-in (launcher and aamd_lfilter_plan)
lfw::Pick lfilter_pick(const void* x, const void* y, int64_t n_seq, int64_t length, int n_order, int n_stages) {
  const int cu = dev_props().cu_count;
  if (force_generic()) return lfw::Pick{lfw::kPickGeneral, 0, grid_for(n_seq, 1, cu * 8), 0};
  const size_t cap = dev_props().lds_per_block_optin ? dev_props().lds_per_block_optin : 64 * 1024;
  int force_w = 0, force_pipe = -1;
#ifdef AAMD_LAB
  static const int lab_w = [] { const char* e = std::getenv("AAMD_LFW_W"); return e ? std::atoi(e) : 0; }();
  static const int lab_pipe = [] { const char* e = std::getenv("AAMD_LFW_PIPE"); return e ? std::atoi(e) : -1; }();
  force_w = lab_w;
  force_pipe = lab_pipe;
#endif
  const bool vec_ok = (reinterpret_cast<uintptr_t>(x) % 16 == 0) && (reinterpret_cast<uintptr_t>(y) % 16 == 0) &&
                      (length % 4 == 0) && lfilter_lab() != 64;      // lab 64: the dword copies also for aligned rows
  return lfw::pick(n_seq, length, n_order, n_stages, vec_ok, cap, cu, force_w, force_pipe);
}

}  // namespace

extern "C" {

int aamd_lfilter_plan(const void* x, const void* y, int64_t batch, int32_t channels, int64_t length, int32_t n_order,
                      int32_t n_stages, int32_t out[4]) {
  DeviceScope dev_scope_(x);
  AAMD_CHECK_ARG(out != nullptr, "null out");
  AAMD_CHECK_ARG(batch >= 0 && channels >= 1 && length >= 0, "bad sizes");
  AAMD_CHECK_ARG(n_order >= 1 && n_stages >= 1, "n_order and n_stages must be >= 1");
  const lfw::Pick pk = lfilter_pick(x, y, batch * channels, length, n_order, n_stages);
  out[0] = pk.kernel;
  out[1] = pk.W;
  out[2] = pk.blocks;
  out[3] = (int32_t)pk.lds;
  return AAMD_OK;
}

int aamd_lfilter_f32(const float* x, const float* a, const float* b, float* y, int64_t batch,
                     int32_t channels, int64_t length, int32_t n_order, int32_t n_coeff_rows,
                     int32_t n_stages, int32_t clamp, void* stream) {
  DeviceScope dev_scope_(x);
  AAMD_CHECK_ARG(x && a && b && y, "null buffer");
  AAMD_CHECK_ARG(batch >= 0 && channels >= 1 && length >= 0, "bad sizes");
  AAMD_CHECK_ARG(n_order >= 1 && n_stages >= 1, "n_order and n_stages must be >= 1");
  AAMD_CHECK_ARG(clamp >= 0 && clamp <= 2, "clamp must be 0, 1 (after every stage) or 2 (after the last stage only)");
  AAMD_CHECK_ARG(n_coeff_rows == 1 || n_coeff_rows == channels, "n_coeff_rows must be 1 or channels");
  const int64_t n_seq = batch * channels;
  if (n_seq == 0 || length == 0) return AAMD_OK;
  hipStream_t s = (hipStream_t)stream;
  const int d = n_order - 1;
  // biquad-class filters: W waves per sequence with shuffle scans (lfilter_wave.h); lfw::pick chooses W and the kernel
  const lfw::Pick pk = lfilter_pick(x, y, n_seq, length, n_order, n_stages);
  if (pk.kernel != lfw::kPickGeneral) {
    const int W = pk.W, blocks = pk.blocks;
    const size_t lds = pk.lds;
    const int lab = lfilter_lab();
    const bool vec_ok = pk.kernel == lfw::kPickWave8Vec || pk.kernel == lfw::kPickWave16Vec;
#define AAMD_LFW(LL, MW, VV)                                                                                       \
    return launch(lfw::lfilter_wave_kernel<LL, MW, VV>, blocks, 64 * W, lds, s, x, a, b, y, n_seq, channels, length, \
                  n_order, n_coeff_rows, n_stages, clamp);
#ifndef AAMD_LAB
#define AAMD_LFW_LABS(MW)                                                                                          \
    { if (vec_ok) AAMD_LFW(0, MW, true) else AAMD_LFW(0, MW, false) }
#else
#define AAMD_LFW_LABS(MW)                                                                                          \
    switch (vec_ok ? lab : 0) {                                                                                  \
      case 1: AAMD_LFW(1, MW, true) break;                                                                       \
      case 2: AAMD_LFW(2, MW, true) break;                                                                       \
      case 4: AAMD_LFW(4, MW, true) break;                                                                       \
      case 8: AAMD_LFW(8, MW, true) break;                                                                       \
      case 15: AAMD_LFW(15, MW, true) break;                                                                     \
      case 16: AAMD_LFW(16, MW, true) break;                                                                     \
      case 32: AAMD_LFW(32, MW, true) break;                                                                     \
      case 63: AAMD_LFW(63, MW, true) break;                                                                     \
      case 128: AAMD_LFW(128, MW, true) break;                                                                   \
      case 256: AAMD_LFW(256, MW, true) break;                                                                   \
      case 512: AAMD_LFW(512, MW, true) break;                                                                   \
      case 896: AAMD_LFW(896, MW, true) break;                                                                   \
      default:                                                                                                   \
        if (vec_ok) AAMD_LFW(0, MW, true) else AAMD_LFW(0, MW, false)                                            \
    }
#endif
    if (pk.kernel == lfw::kPickMover) {   // 8 filter waves + 4 mover waves that own the copies and the stores
#define AAMD_LFWM(LL)                                                                                              \
      return launch(lfw::lfilter_wave_mover_kernel<LL>, blocks, 64 * (8 + lfw::kMovers), lds, s, x, a, b, y, n_seq,  \
                    channels, length, n_order, n_coeff_rows, n_stages, clamp);
#ifdef AAMD_LAB
      switch (lab) {
        case 1: AAMD_LFWM(1) break;
        case 16: AAMD_LFWM(16) break;
        case 32: AAMD_LFWM(32) break;
        case 48: AAMD_LFWM(48) break;
        default: AAMD_LFWM(0)
      }
#else
      AAMD_LFWM(0)
#endif
#undef AAMD_LFWM
    } else if (pk.kernel == lfw::kPickPipe) {   // two tiles per wave, copies and stores spread over the stages (8 waves)
#define AAMD_LFWP(LL)                                                                                              \
      return launch(lfw::lfilter_wave_pipe_kernel<LL>, blocks, 512, lds, s, x, a, b, y, n_seq, channels, length,     \
                    n_order, n_coeff_rows, n_stages, clamp);
#ifdef AAMD_LAB
      switch (lab) {
        case 1: AAMD_LFWP(1) break;
        case 15: AAMD_LFWP(15) break;
        case 16: AAMD_LFWP(16) break;
        case 32: AAMD_LFWP(32) break;
        case 48: AAMD_LFWP(48) break;
        case 50: AAMD_LFWP(50) break;
        case 52: AAMD_LFWP(52) break;
        case 56: AAMD_LFWP(56) break;
        case 63: AAMD_LFWP(63) break;
        default: AAMD_LFWP(0)
      }
#else
      AAMD_LFWP(0)
#endif
#undef AAMD_LFWP
    } else if (pk.kernel == lfw::kPickWave8Vec || pk.kernel == lfw::kPickWave8) {      // 512 threads: the 256-register instantiation
      AAMD_LFW_LABS(8)
    } else {
      AAMD_LFW_LABS(16)
    }
#undef AAMD_LFW_LABS
#undef AAMD_LFW
  }
#define AAMD_LF(D) return launch_lfilter<D>(x, a, b, y, n_seq, channels, length, n_order, n_coeff_rows, n_stages, clamp, s)
  if (d <= 1) AAMD_LF(1);
  if (d <= 2) AAMD_LF(2);
  if (d <= 3) AAMD_LF(3);
  if (d <= 4) AAMD_LF(4);
  if (d <= 6) AAMD_LF(6);
  if (d <= 8) AAMD_LF(8);
  if (d <= 12) AAMD_LF(12);
  if (d <= 16) AAMD_LF(16);
#undef AAMD_LF
  return fail(AAMD_EUNSUPPORTED, "audio_amd: lfilter order > 16 not supported");
}

}  // extern "C"
