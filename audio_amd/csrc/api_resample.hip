// Sinc resampler of the C ABI: scalar, banded matrix-core (fp32 / binary16-split) and sparse kernels.
#include <cstdlib>

#include "api_common.h"
#include "resample.h"
#include "resample_mfma.h"

using namespace aamd;

extern "C" {

int aamd_resample_f32(const float* wav, const float* kernel, float* out, int64_t rows, int64_t length,
                      int64_t row_stride, int32_t orig, int32_t new_, int32_t width, int64_t out_len,
                      void* stream) {
  DeviceScope dev_scope_(wav);
  AAMD_CHECK_ARG(wav && kernel && out, "null buffer");
  AAMD_CHECK_ARG(rows >= 0 && length >= 0 && orig >= 1 && new_ >= 1 && width >= 0, "bad sizes");
  AAMD_CHECK_ARG(row_stride >= length, "row_stride < length");
  const int64_t expect = (new_ * length + orig - 1) / orig;
  AAMD_CHECK_ARG(out_len == expect, "out_len must be ceil(new*length/orig)");
  if (rows == 0 || out_len == 0) return AAMD_OK;
  ResampleGeom g;
  g.rows = rows; g.length = length; g.row_stride = row_stride; g.out_len = out_len;
  g.orig = orig; g.new_ = new_; g.width = width; g.taps = 2 * width + orig;
  const int64_t nq = (out_len + new_ - 1) / new_;
  // aim for ~2048 outputs per workgroup, halo within 96 KiB of LDS
  int qt = (2048 + new_ - 1) / new_;
  if (qt < 1) qt = 1;
  if (qt > nq) qt = (int)nq;
  const int64_t lds_budget = 96 * 1024 / sizeof(float);
  while (qt > 1 && (int64_t)(qt - 1) * orig + g.taps > lds_budget) --qt;
  g.qt = qt;
  g.use_lds = ((int64_t)(qt - 1) * orig + g.taps <= lds_budget) ? 1 : 0;
  g.nq_tiles = (int)((nq + qt - 1) / qt);
  const int64_t blocks = rows * g.nq_tiles;
  AAMD_CHECK_ARG(blocks < (1ll << 31), "too many tiles for one launch");
  const size_t lds = g.use_lds ? ((size_t)(qt - 1) * orig + g.taps) * sizeof(float) : 0;
  return launch(resample_kernel, blocks, 256, lds, (hipStream_t)stream, g, wav, kernel, out);
}

// tools only (tools/rsm_census.py): the time stamps the f16 resampler records under AAMD_RSM_LAB=64
int aamd_debug_rsm_census(long long* host, int n) {
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(rsm::g_rsm_census), sizeof(long long) * (size_t)n) == hipSuccess ? 0 : -1;
}

int aamd_resample_banded_f32(const float* wav, const float* kernel, float* out, int64_t rows,
                             int64_t length, int64_t row_stride, int32_t orig, int32_t new_, int32_t width,
                             int64_t out_len, const aamd_resample_bands* bands, void* stream) {
  return aamd_resample_prepared_f32(wav, kernel, out, rows, length, row_stride, orig, new_, width, out_len, bands, nullptr, stream);
}

int64_t aamd_resample_frag_bytes(int32_t orig, int32_t new_, const aamd_resample_bands* bands) {
  if (bands == nullptr || new_ < 1 || bands->n_tiles != (new_ + 15) / 16) return 0;
  const int ks = rsm::pick_ks(bands->tap_span, orig);
  return ks == 0 ? 0 : rsm::frag_bytes(bands->n_tiles, ks);
}

int aamd_resample_frag_build_f32(const float* kernel, int32_t orig, int32_t new_, int32_t width,
                                 const aamd_resample_bands* bands, void* frag, void* stream) {
  DeviceScope dev_scope_(kernel);
  AAMD_CHECK_ARG(kernel && frag && bands, "null buffer");
  AAMD_CHECK_ARG(orig >= 1 && new_ >= 1 && width >= 0, "bad sizes");
  const int n_tiles = (new_ + 15) / 16;
  AAMD_CHECK_ARG(bands->n_tiles == n_tiles && bands->tap_lo != nullptr && bands->tap_span >= 1, "band table must have ceil(new/16) tiles");
  const int ks = rsm::pick_ks(bands->tap_span, orig);
  if (ks == 0) return fail(AAMD_EUNSUPPORTED, "audio_amd: band wider than 448 taps: no matrix-core kernel, no prepared fragments");
  AAMD_CHECK_ARG(reinterpret_cast<uintptr_t>(frag) % 16 == 0, "fragment table must be 16-byte aligned");
  const int taps = 2 * width + orig;
  for (int t = 0; t < n_tiles; ++t)
    AAMD_CHECK_ARG(bands->tap_lo[t] >= 0 && bands->tap_lo[t] < taps, "tap_lo outside the tap table");
  rsm::Geom g{};
  g.orig = orig; g.new_ = new_; g.width = width; g.taps = taps;
  for (int pt0 = 0; pt0 < n_tiles; pt0 += rsm::kMaxPhaseTiles) {          // (the band starts ride in the kernel arguments, 14 tiles a launch)
    g.pt0 = pt0;
    g.n_pt = n_tiles - pt0 < rsm::kMaxPhaseTiles ? n_tiles - pt0 : rsm::kMaxPhaseTiles;
    for (int t = 0; t < g.n_pt; ++t) g.tap_lo[t] = bands->tap_lo[pt0 + t];
    const int n = g.n_pt * (ks / 8) * 64;
    hipLaunchKernelGGL(rsm::frag_build_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g, ks, kernel,
                       static_cast<uint32_t*>(frag));
  }
  return launch_check();
}

int aamd_resample_prepared_f32(const float* wav, const float* kernel, float* out, int64_t rows,
                               int64_t length, int64_t row_stride, int32_t orig, int32_t new_, int32_t width,
                               int64_t out_len, const aamd_resample_bands* bands, const void* frag, void* stream) {
  DeviceScope dev_scope_(wav);
  const int n_tiles = (new_ + 15) / 16;
  const int ks = bands ? rsm::pick_ks(bands->tap_span, orig) : 0;
  if (bands == nullptr || ks == 0 || force_generic())
    return aamd_resample_f32(wav, kernel, out, rows, length, row_stride, orig, new_, width, out_len, stream);
  AAMD_CHECK_ARG(wav && kernel && out, "null buffer");
  AAMD_CHECK_ARG(rows >= 0 && length >= 0 && orig >= 1 && new_ >= 1 && width >= 0, "bad sizes");
  AAMD_CHECK_ARG(row_stride >= length, "row_stride < length");
  AAMD_CHECK_ARG(out_len == (new_ * length + orig - 1) / orig, "out_len must be ceil(new*length/orig)");
  AAMD_CHECK_ARG(bands->n_tiles == n_tiles && bands->tap_lo != nullptr && bands->tap_span >= 1,
                 "band table must have ceil(new/16) tiles");
  if (rows == 0 || out_len == 0) return AAMD_OK;
  const int taps = 2 * width + orig;
  for (int t = 0; t < n_tiles; ++t)
    AAMD_CHECK_ARG(bands->tap_lo[t] >= 0 && bands->tap_lo[t] < taps, "tap_lo outside the tap table");
  rsm::Geom g{};
#ifdef AAMD_LAB
  static const int rsm_lab = [] { const char* e = std::getenv("AAMD_RSM_LAB"); return e ? std::atoi(e) : 0; }();   // tools only
  g.lab = rsm_lab;
#endif
  g.frag = static_cast<const uint32_t*>(frag);       // (read by the f16 kernels only)
  AAMD_CHECK_ARG(reinterpret_cast<uintptr_t>(frag) % 16 == 0, "fragment table must be 16-byte aligned");
  g.rows = rows; g.length = length; g.row_stride = row_stride; g.out_len = out_len;
  g.orig = orig; g.new_ = new_; g.width = width; g.taps = taps;
  g.vec_in = (reinterpret_cast<uintptr_t>(wav) % 16 == 0) && (row_stride % 4 == 0);
  g.vec_out = (reinterpret_cast<uintptr_t>(out) % 16 == 0) && (out_len % 4 == 0) && (new_ % 4 == 0);
  const int64_t nq = (out_len + new_ - 1) / new_;
  const int max_cw = rsm::max_compute_waves(ks);
  const size_t lds_cap = dev_props().lds_per_block_optin ? dev_props().lds_per_block_optin : 64 * 1024;
  for (int pt0 = 0; pt0 < n_tiles; pt0 += max_cw) {
    g.pt0 = pt0;
    g.n_pt = n_tiles - pt0 < max_cw ? n_tiles - pt0 : max_cw;
    int max_lo = 0;
    for (int t = 0; t < g.n_pt; ++t) {
      g.tap_lo[t] = bands->tap_lo[pt0 + t];
      if (g.tap_lo[t] > max_lo) max_lo = g.tap_lo[t];
    }
    const bool f16 = (policy() & AAMD_POLICY_RESAMPLE_FP32) == 0;
    const bool rd64 = f16 && rsm::b64_ok(ks, orig) && (policy() & AAMD_POLICY_RESAMPLE_B32) == 0;
    if (!rsm::plan_chunk(g, ks, f16, nq, max_lo, lds_cap))   // a single q-group does not fit (huge orig): scalar kernel
      return aamd_resample_f32(wav, kernel, out, rows, length, row_stride, orig, new_, width, out_len, stream);
    const int qg = g.qg;
    const int qc = rsm::chunk_q(g);
    const size_t lds = 2 * (size_t)g.buf_floats * sizeof(float) + (f16 ? 48 : 0);       // + the chunk-maximum slots and arrival counters
    g.chunks_per_row = (int)((nq + qc - 1) / qc);
    g.n_chunks = rows * g.chunks_per_row;
    AAMD_CHECK_ARG(g.n_chunks < (1ll << 31), "too many chunks for one launch");
    // persistent workgroups: as many per CU as the 16 wave slots (128 registers) and the LDS hold -- a one-tile rate pair
    // has only a handful of compute waves per workgroup
    const int wg_waves = g.n_pt * qg + g.n_loaders;
    int per_cu = ks >= 80 ? 1 : 16 / wg_waves;
    if (per_cu > (int)(lds_cap / lds)) per_cu = (int)(lds_cap / lds);
    if (per_cu < 1) per_cu = 1;
    int64_t blocks = (int64_t)dev_props().cu_count * per_cu;
    if (blocks > g.n_chunks) blocks = g.n_chunks;
    g.chunks_per_block = (int)((g.n_chunks + blocks - 1) / blocks);
    blocks = (g.n_chunks + g.chunks_per_block - 1) / g.chunks_per_block;
    const int threads = 64 * wg_waves;
#ifdef AAMD_LAB
#define AAMD_RSM_F16(KS) (g.lab == 0 ? rsm::resample_f16_kernel<KS, 0> : g.lab == 64 ? rsm::resample_f16_kernel<KS, 1> : rsm::resample_f16_kernel<KS, 2>)
#define AAMD_RSM_RD64(KS) (g.lab == 64 ? (full ? rsm::kernel_rd64<KS, 1, 1>() : rsm::kernel_rd64<KS, 1>()) : (full ? rsm::kernel_rd64<KS, 0, 1>() : rsm::kernel_rd64<KS, 0>()))
#else
#define AAMD_RSM_F16(KS) (rsm::resample_f16_kernel<KS, 0>)
#define AAMD_RSM_RD64(KS) (full ? rsm::kernel_rd64<KS, 0, 1>() : rsm::kernel_rd64<KS, 0>())
#endif
#define AAMD_RSM(KS)                                                                                  \
  do {                                                                                                \
    auto kern = !f16 ? rsm::resample_mfma_kernel<KS> : AAMD_RSM_F16(KS);                              \
    /* 8-byte operand reads: odd orig, KS = 80 / 104 / 112 (resample_mfma.h, b64_rot) */              \
    const bool full = rd64 && rsm::chunk_is_full(g, KS);   /* padded chunk: the branch-free loader instantiation */ \
    if (f16 && rd64) kern = AAMD_RSM_RD64(KS);                                                        \
    rc = launch(kern, blocks, threads, lds, (hipStream_t)stream, g, wav, kernel, out);                \
  } while (0)
    int rc;
    switch (ks) {
      case 16: AAMD_RSM(16); break;
      case 48: AAMD_RSM(48); break;
      case 80: AAMD_RSM(80); break;
      case 104: AAMD_RSM(104); break;      // (odd orig only: pick_ks)
      default: AAMD_RSM(112); break;
    }
#undef AAMD_RSM
#undef AAMD_RSM_F16
#undef AAMD_RSM_RD64
    if (rc != AAMD_OK) return rc;
  }
  return AAMD_OK;
}

int aamd_resample_sparse_f32(const float* wav, const float* taps_compact, const int32_t* tap_lo, float* out, int64_t rows,
                             int64_t length, int64_t row_stride, int32_t orig, int32_t new_, int32_t width, int32_t span,
                             int64_t out_len, void* stream) {
  DeviceScope dev_scope_(wav);
  AAMD_CHECK_ARG(wav && taps_compact && tap_lo && out, "null buffer");
  AAMD_CHECK_ARG(rows >= 0 && length >= 0 && orig >= 1 && new_ >= 1 && width >= 0 && span >= 1, "bad sizes");
  AAMD_CHECK_ARG(row_stride >= length, "row_stride < length");
  AAMD_CHECK_ARG(out_len == ((int64_t)new_ * length + orig - 1) / orig, "out_len must be ceil(new*length/orig)");
  const int64_t n = rows * out_len;
  if (n == 0) return AAMD_OK;
  AAMD_CHECK_ARG((n + 255) / 256 < (1ll << 31), "too many samples for one launch");
  return launch(resample_sparse_kernel, (n + 255) / 256, 256, 0, (hipStream_t)stream, wav, taps_compact, tap_lo, out, rows,
                length, row_stride, orig, new_, width, span, out_len);
}

}  // extern "C"
