// Launcher internals shared by the api_*.hip sources (api_common.h) and the entry points of the C ABI that belong to no
// kernel family.  No torch dependency, no global mutable state except a thread-local error string, the kernel policy and a
// per-process cache of immutable device properties.
#include "api_common.h"

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <mutex>

#include "stft_generic.h"

namespace aamd {

namespace {
thread_local std::string g_err;
std::atomic<int> g_policy{-1};
}  // namespace

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

int launch_check() {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(AAMD_EHIP, std::string("audio_amd: kernel launch failed: ") + hipGetErrorString(e));
  return AAMD_OK;
}

int policy() {
  int p = g_policy.load(std::memory_order_relaxed);
  if (p < 0) {
    p = 0;
    if (std::getenv("AAMD_FORCE_GENERIC") != nullptr) p |= AAMD_POLICY_FORCE_GENERIC;
    if (std::getenv("AAMD_MEL400_WIDE") != nullptr) p |= AAMD_POLICY_MEL400_WIDE;
    if (std::getenv("AAMD_ISTFT_ATOMIC") != nullptr) p |= AAMD_POLICY_ISTFT_ATOMIC;
    if (std::getenv("AAMD_RESAMPLE_FP32") != nullptr) p |= AAMD_POLICY_RESAMPLE_FP32;
    if (std::getenv("AAMD_FFTCONV_NO_FDL") != nullptr) p |= AAMD_POLICY_FFTCONV_NO_FDL;
    if (std::getenv("AAMD_FFTCONV_FDL") != nullptr) p |= AAMD_POLICY_FFTCONV_FDL;
    if (std::getenv("AAMD_RESAMPLE_B32") != nullptr) p |= AAMD_POLICY_RESAMPLE_B32;
    if (std::getenv("AAMD_MEL400_NO_POOL") != nullptr) p |= AAMD_POLICY_MEL400_NO_POOL;
    if (std::getenv("AAMD_MEL400_SCALAR") != nullptr) p |= AAMD_POLICY_MEL400_SCALAR;
    int expected = -1;
    g_policy.compare_exchange_strong(expected, p);
    p = g_policy.load(std::memory_order_relaxed);
  }
  return p;
}

DevProps& dev_props() {
  static DevProps props[64];
  static std::mutex mu;
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (dev < 0 || dev >= 64) dev = 0;
  std::lock_guard<std::mutex> lock(mu);
  DevProps& p = props[dev];
  if (!p.ok) {
    hipDeviceProp_t dp;
    if (hipGetDeviceProperties(&dp, dev) == hipSuccess) {
      p.cu_count = dp.multiProcessorCount;
      p.lds_per_block = dp.sharedMemPerBlock;
      p.lds_per_block_optin = dp.sharedMemPerBlockOptin ? dp.sharedMemPerBlockOptin : dp.sharedMemPerBlock;
      p.ok = true;
    } else {
      p.cu_count = 256;
      p.lds_per_block = 64 * 1024;
      p.lds_per_block_optin = 160 * 1024;
    }
  }
  return p;
}

int grid_for(int64_t n, int per_block, int max_blocks) {
  int64_t b = (n + per_block - 1) / per_block;
  if (b > max_blocks) b = max_blocks;
  if (b < 1) b = 1;
  return (int)b;
}

static int frames_expected(const aamd_stft_desc* d) {
  int64_t lp = d->length + 2 * (int64_t)d->pad + (d->center ? 2 * (int64_t)(d->n_fft / 2) : 0);
  if (lp < d->n_fft) return -1;
  return (int)(1 + (lp - d->n_fft) / d->hop);
}

int validate_desc(const aamd_stft_desc* d, StftGeom& g) {
  AAMD_CHECK_ARG(d != nullptr, "null stft desc");
  AAMD_CHECK_ARG(d->rows >= 0 && d->length >= 0, "negative sizes");
  AAMD_CHECK_ARG(d->n_fft >= 1 && d->hop >= 1 && d->pad >= 0, "n_fft, hop must be >= 1 and pad >= 0");
  AAMD_CHECK_ARG(d->row_stride >= d->length, "row_stride < length");
  AAMD_CHECK_ARG(d->pad_mode >= 0 && d->pad_mode <= 3, "bad pad_mode");
  if (d->n_fft > 8192) return fail(AAMD_EUNSUPPORTED, "audio_amd: n_fft > 8192 not supported");
  const int64_t l1 = d->length + 2 * (int64_t)d->pad;
  if (d->center && d->pad_mode == AAMD_PAD_REFLECT)
    AAMD_CHECK_ARG(d->n_fft / 2 < l1, "reflect padding needs n_fft/2 < padded length");
  if (d->center && d->pad_mode == AAMD_PAD_CIRCULAR)
    AAMD_CHECK_ARG(d->n_fft / 2 <= l1, "circular padding needs n_fft/2 <= padded length");
  if (d->center && d->pad_mode == AAMD_PAD_REPLICATE) AAMD_CHECK_ARG(l1 >= 1, "empty input");
  const int T = frames_expected(d);
  AAMD_CHECK_ARG(T >= 1, "input shorter than n_fft");
  AAMD_CHECK_ARG(T == d->n_frames, "n_frames does not match 1 + (L' - n_fft)/hop");
  g.rows = d->rows; g.length = d->length; g.row_stride = d->row_stride;
  g.n_fft = d->n_fft; g.hop = d->hop; g.pad = d->pad; g.center = d->center;
  g.pad_mode = d->pad_mode; g.onesided = d->onesided; g.n_frames = d->n_frames;
  g.n_freq = d->onesided ? d->n_fft / 2 + 1 : d->n_fft;
  g.scale = d->scale; g.power = d->power;
  g.n_stages = plan_radices(d->n_fft, g.radix);
  if (g.n_stages < 0) return fail(AAMD_EUNSUPPORTED, "audio_amd: n_fft has too many prime factors");
  return AAMD_OK;
}

int validate_bands(const aamd_mel_bands* b, int n_freq, MelBandsDev& mb) {
  AAMD_CHECK_ARG(b != nullptr, "null mel bands");
  AAMD_CHECK_ARG(b->n_mels >= 1 && b->max_width >= 1 && b->max_width <= n_freq, "bad mel band table");
  AAMD_CHECK_ARG(b->lo && b->width && b->weights, "null mel band pointers");
  mb.n_mels = b->n_mels; mb.max_width = b->max_width;
  mb.lo = b->lo; mb.width = b->width; mb.weights = b->weights; mb.order = b->lane_order;
  mb.table400 = b->table400;
  mb.table_sig = b->table400 ? b->table_sig : 0;
  return AAMD_OK;
}

}  // namespace aamd

using namespace aamd;

extern "C" {

int aamd_abi_version(void) { return AAMD_ABI_VERSION; }

int aamd_set_kernel_policy(int flags) {
  const int prev = policy();
  if (flags >= 0) g_policy.store(flags & (AAMD_POLICY_FORCE_GENERIC | AAMD_POLICY_MEL400_WIDE | AAMD_POLICY_ISTFT_ATOMIC |
                                          AAMD_POLICY_RESAMPLE_FP32 | AAMD_POLICY_FFTCONV_NO_FDL | AAMD_POLICY_FFTCONV_FDL |
                                          AAMD_POLICY_FFTCONV_COMPLEX | AAMD_POLICY_RESAMPLE_B32 | AAMD_POLICY_MEL400_NO_POOL |
                                          AAMD_POLICY_MEL400_SCALAR));
  return prev;
}

const char* aamd_last_error(void) { return g_err.c_str(); }

int aamd_device_info(char* name, int32_t name_len, int32_t* cu_count, int64_t* hbm_bytes) {
  int dev = 0;
  AAMD_HIP(hipGetDevice(&dev));
  hipDeviceProp_t dp;
  AAMD_HIP(hipGetDeviceProperties(&dp, dev));
  if (name && name_len > 0) {
    std::snprintf(name, (size_t)name_len, "%s", dp.gcnArchName);
  }
  if (cu_count) *cu_count = dp.multiProcessorCount;
  if (hbm_bytes) *hbm_bytes = (int64_t)dp.totalGlobalMem;
  return AAMD_OK;
}

// Box probe (bench.py `box_calibration`): every workgroup runs the same fixed chain of dependent fp32 FMAs in all of its
// waves and records shader cycles (s_memtime), 100 MHz wall ticks (s_memrealtime) and the XCD it ran on.  cycles / ticks is
// the shader clock this box sustains under vector-ALU load; the spread of the per-XCD means is the XCD skew.  Boxes of one
// pool ran the same binary between 65.9 and 72.5 us: this is what the bench line reports beside its
// number so that a slow box can be told from a slow kernel.
__global__ void __launch_bounds__(256) box_probe_kernel(long long* __restrict__ rec, int iters) {
  float a0 = 1.0f + threadIdx.x * 1e-6f, a1 = 0.5f, a2 = 0.25f, a3 = 0.125f;
  const float m = 0.99999f, c = 1e-7f;
  const long long c0 = (long long)clock64(), w0 = (long long)wall_clock64();
  for (int i = 0; i < iters; ++i) {
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      a0 = fmaf(a0, m, c); a1 = fmaf(a1, m, c); a2 = fmaf(a2, m, c); a3 = fmaf(a3, m, c);
    }
  }
  const long long c1 = (long long)clock64(), w1 = (long long)wall_clock64();
  unsigned xcc = 0;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
  if (threadIdx.x == 0) {
    long long* r = rec + 4 * (long long)blockIdx.x;
    r[0] = c1 - c0; r[1] = w1 - w0; r[2] = (long long)(xcc & 15u); r[3] = w0;
  }
  if (a0 + a1 + a2 + a3 == 123456.0f) rec[0] = 0;       // keeps the chains alive
}

int aamd_box_probe(int64_t* rec, int32_t n_blocks, int32_t iters, void* stream) {
  DeviceScope dev_scope_(rec);
  AAMD_CHECK_ARG(rec != nullptr && n_blocks >= 1 && iters >= 1, "box probe: rec[4 * n_blocks], n_blocks >= 1, iters >= 1");
  return launch(box_probe_kernel, n_blocks, 256, 0, (hipStream_t)stream, reinterpret_cast<long long*>(rec), (int)iters);
}

}  // extern "C"
