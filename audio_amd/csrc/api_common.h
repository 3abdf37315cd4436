// Launcher internals shared by the api_*.hip sources of libaudio_amd.so (definitions: api_common.hip): the error string,
// argument / HIP checks, the kernel-selection policy, the device scope and properties, and the one launch idiom.
// Everything here is hidden: the library exports the aamd_* functions of include/audio_amd.h and nothing of this.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <utility>

#include "../../include/audio_amd.h"

#pragma GCC visibility push(hidden)
namespace aamd {

struct StftGeom;      // stft_generic.h
struct MelBandsDev;

// sets the calling thread's error string (aamd_last_error) and returns `code`
int fail(int code, const std::string& msg);

#define AAMD_CHECK_ARG(cond, msg) \
  do { if (!(cond)) return fail(AAMD_EINVAL, std::string("audio_amd: ") + msg); } while (0)

#define AAMD_HIP(expr)                                                                   \
  do {                                                                                   \
    hipError_t e_ = (expr);                                                              \
    if (e_ != hipSuccess)                                                                \
      return fail(AAMD_EHIP, std::string("audio_amd: HIP error: ") + hipGetErrorString(e_) + \
                                 " at " #expr);                                          \
  } while (0)

int launch_check();

// Kernel-selection switches (tests / A-B experiments): a process-wide bit mask, initialised ONCE from the environment
// (AAMD_FORCE_GENERIC, AAMD_MEL400_WIDE, AAMD_ISTFT_ATOMIC) and changed afterwards only through
// aamd_set_kernel_policy() -- no getenv() on the launch path.
int policy();
inline bool force_generic() { return (policy() & AAMD_POLICY_FORCE_GENERIC) != 0; }

// The launches size their grids from, and set function attributes on, the CURRENT device.  In a process that sees
// several GPUs (not the one-process-per-GPU deployment) the caller's tensors may live on another one: make the
// device that owns the buffer current for the duration of the call.  Costs nothing when one GPU is visible.
struct DeviceScope {
  int prev = -1;
  explicit DeviceScope(const void* p) {
    static const int n_dev = [] { int n = 1; (void)hipGetDeviceCount(&n); return n; }();
    if (n_dev <= 1 || p == nullptr) return;
    int cur = 0, own = 0;
    if (hipGetDevice(&cur) != hipSuccess) return;
    if (hipPointerGetAttribute(&own, HIP_POINTER_ATTRIBUTE_DEVICE_ORDINAL, const_cast<void*>(p)) != hipSuccess) {
      (void)hipGetLastError();
      return;
    }
    if (own != cur && own >= 0 && own < n_dev && hipSetDevice(own) == hipSuccess) prev = cur;
  }
  ~DeviceScope() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
  DeviceScope(const DeviceScope&) = delete;
  DeviceScope& operator=(const DeviceScope&) = delete;
};

struct DevProps {
  int cu_count = 0;
  size_t lds_per_block = 0;
  size_t lds_per_block_optin = 0;
  bool ok = false;
};

DevProps& dev_props();      // of the current device

int grid_for(int64_t n, int per_block, int max_blocks);

// the descriptor / band table checks of every STFT-shaped entry point; they fill the kernels' argument structs
int validate_desc(const aamd_stft_desc* d, StftGeom& g);
int validate_bands(const aamd_mel_bands* b, int n_freq, MelBandsDev& mb);

// One kernel launch: more than 48 KB of dynamic LDS is opted into first.  (A launch that must fit the device's opt-in
// limit checks lds_per_block_optin itself, with its own message, before it comes here.)
template <class K, class... A>
int launch(K kern, int64_t blocks, int threads, size_t lds, hipStream_t s, A&&... args) {
  if (lds > 48 * 1024)
    AAMD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3((unsigned)threads), lds, s, std::forward<A>(args)...);
  return launch_check();
}

}  // namespace aamd
#pragma GCC visibility pop
