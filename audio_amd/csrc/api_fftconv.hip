// FFT convolution of the C ABI: overlap-save plans 1 - 3 and the tiled time-domain kernel.
#include "api_common.h"
#include "fftconv.h"
#include "fftconv_os.h"
#include "fftconv_fdr.h"

using namespace aamd;

namespace {

// taps above this use overlap-save on the LDS FFT; below, the tiled time-domain kernel is cheaper
const int64_t kFftConvMinTaps = 192;

bool fftconv_use_fft(int64_t n_taps) {
  return n_taps > kFftConvMinTaps && !force_generic();
}

// partitions of the delay-line plan, 0 when the tap count (or the policy) rules it out
int64_t fftconv_fdl_parts(int64_t n_taps) {
  const int64_t np = (n_taps + fco::kHop - 1) / fco::kHop;
  return ((policy() & AAMD_POLICY_FFTCONV_NO_FDL) || np < 2 || np > fco::kMaxFdlParts) ? 0 : np;
}
// the plan of one call: the cost model of fco::plan_fdl, or (policy, tests) the delay line whenever it is possible at all
bool fftconv_pick_fdl(int64_t rows, int64_t taps, int64_t out_len, fco::FdlGeom& f) {
  if (!fftconv_fdl_parts(taps)) return false;
  const bool cheaper = fco::plan_fdl(rows, taps, out_len, dev_props().cu_count, f);
  return cheaper || ((policy() & AAMD_POLICY_FFTCONV_FDL) && f.n_blocks >= 2);
}

// the real-block kernel (fftconv_fdr.h, plan 3): EVERY FFT-eligible tap count up to 32768 (round 5; 24576 in round 4) -- plain
// overlap-save on real blocks up to 8192 taps (one partition, no delay line), the register delay line of up to three delayed
// spectra for 8193 .. 32768 -- unless ANY of the three FFTCONV
// policy bits is set: NO_FDL / FDL / COMPLEX all select the complex-block kernels (plans 1 / 2) for all tap counts, also for
// <= 8192 taps where plan 3 is not a delay line at all (the bits exist for A/B runs against the round-1..3 kernels)
bool fftconv_pick_fdr(int64_t rows, int64_t taps, int64_t out_len, fdr::Geom& g) {
  if (policy() & (AAMD_POLICY_FFTCONV_NO_FDL | AAMD_POLICY_FFTCONV_FDL | AAMD_POLICY_FFTCONV_COMPLEX)) return false;
  return fdr::plan(rows, taps, out_len, dev_props().cu_count, g);
}

}  // namespace

extern "C" {

int64_t aamd_fftconvolve_workspace(int64_t rows, int64_t n_x_rows, int64_t n_y_rows, int64_t nx, int64_t ny) {
  (void)rows;
  const bool swap = ny > nx;
  const int64_t taps = swap ? nx : ny;
  const int64_t tap_rows = swap ? n_x_rows : n_y_rows;
  if (!fftconv_use_fft(taps)) return 0;
  fco::Geom g{};
  fco::plan(taps, 1, g);
  // twiddles | tap spectra (of whichever plan runs) | delay-line rings, one per workgroup (the slice is not known here)
  const int64_t np_fdl = fftconv_fdl_parts(taps);
  const int64_t n_spec = tap_rows * (np_fdl > g.n_part ? np_fdl : g.n_part);
  return (int64_t)sizeof(fco::C32) * fco::kN * (1 + n_spec + (np_fdl > 2 ? np_fdl - 2 : 0) * dev_props().cu_count);
}

int aamd_fftconvolve_plan(int64_t rows, int64_t nx, int64_t ny, int64_t out_len) {
  const int64_t taps = ny > nx ? nx : ny;
  if (!fftconv_use_fft(taps)) return 0;
  fdr::Geom fg{};
  if (fftconv_pick_fdr(rows, taps, out_len, fg)) return 3;
  fco::FdlGeom f{};
  return fftconv_pick_fdl(rows, taps, out_len, f) ? 2 : 1;
}

int aamd_fftconvolve_f32(const float* x, const float* y, float* out, int64_t rows, int64_t n_x_rows,
                         int64_t n_y_rows, int64_t nx, int64_t ny, const int64_t* x_row_of,
                         const int64_t* y_row_of, int64_t start, int64_t out_len, void* workspace,
                         void* stream) {
  return aamd_fftconvolve_staged_f32(x, y, out, rows, n_x_rows, n_y_rows, nx, ny, x_row_of, y_row_of, start, out_len,
                                     workspace, AAMD_FFTCONV_PREPARE | AAMD_FFTCONV_RUN, stream);
}

// stages: PREPARE lays the twiddles and the tap spectra of the plan down in the workspace (two small launches), RUN walks the
// rows.  A caller that convolves many batches with ONE impulse response prepares once and runs with the same workspace
// afterwards (the plan must be the same: aamd_fftconvolve_plan, same policy, same tap rows).
int aamd_fftconvolve_staged_f32(const float* x, const float* y, float* out, int64_t rows, int64_t n_x_rows,
                                int64_t n_y_rows, int64_t nx, int64_t ny, const int64_t* x_row_of,
                                const int64_t* y_row_of, int64_t start, int64_t out_len, void* workspace,
                                int32_t stages, void* stream) {
  const bool prep = (stages & AAMD_FFTCONV_PREPARE) != 0, run = (stages & AAMD_FFTCONV_RUN) != 0;
  AAMD_CHECK_ARG((prep || run) && !(stages & ~(AAMD_FFTCONV_PREPARE | AAMD_FFTCONV_RUN)), "stages: PREPARE, RUN or both");
  DeviceScope dev_scope_(run ? (const void*)x : (const void*)workspace);
  AAMD_CHECK_ARG(!run || (x && y && out), "null buffer");
  AAMD_CHECK_ARG(!prep || y, "null tap buffer");
  AAMD_CHECK_ARG(rows >= 0 && nx >= 1 && ny >= 1 && n_x_rows >= 1 && n_y_rows >= 1, "bad sizes");
  AAMD_CHECK_ARG(start >= 0 && out_len >= 0 && start + out_len <= nx + ny - 1, "slice outside the full convolution");
  if (rows == 0 || out_len == 0) return AAMD_OK;
  // stream the SHORTER operand as taps (convolution commutes)
  const bool swap = ny > nx;
  const float* xa = swap ? y : x;
  const float* ya = swap ? x : y;
  const int64_t nxa = swap ? ny : nx, nya = swap ? nx : ny;
  const int64_t tap_rows = swap ? n_x_rows : n_y_rows;
  const int64_t* xmap = swap ? y_row_of : x_row_of;
  const int64_t* ymap = swap ? x_row_of : y_row_of;
  hipStream_t s = (hipStream_t)stream;
  AAMD_CHECK_ARG(!prep || ya, "null tap buffer");
  if (fftconv_use_fft(nya)) {
    AAMD_CHECK_ARG(workspace != nullptr, "fftconvolve needs the workspace of aamd_fftconvolve_workspace()");
    AAMD_CHECK_ARG(reinterpret_cast<uintptr_t>(workspace) % 8 == 0, "workspace must be 8-byte aligned");
    fco::Geom g{};
    g.rows = rows; g.nx = nxa; g.ny = nya; g.start = start; g.out_len = out_len;
    fco::plan(nya, out_len, g);
    fco::C32* tw = reinterpret_cast<fco::C32*>(workspace);
    fco::C32* H = tw + fco::kN;
    const size_t lds = (size_t)fco::kLdsComplex * sizeof(fco::C32);
    AAMD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(fco::spectrum_kernel),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    AAMD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(fco::overlap_save_kernel),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (prep) hipLaunchKernelGGL(fco::twiddle_kernel, dim3(fco::kN / 256), dim3(256), 0, s, tw);
    fdr::Geom fg{};
    fg.rows = rows; fg.nx = nxa; fg.ny = nya; fg.start = start; fg.out_len = out_len;
    if (fftconv_pick_fdr(rows, nya, out_len, fg)) {
      // real blocks of 16384 samples as 8192-point complex FFTs, the delay line in registers (fftconv_fdr.h).  The tap spectra
      // (8192 complex per partition) fit the space the workspace reserves for the complex-block plans (16384 per partition).
      const size_t lds_r = (size_t)fdr::kLdsComplex * sizeof(fco::C32);
      AAMD_CHECK_ARG(tap_rows * fg.n_part < (1ll << 31) && rows * fg.segs < (1ll << 31), "too many tap rows / work items");
      if (prep) {
        AAMD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(fdr::spectrum_kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_r));
        hipLaunchKernelGGL(fdr::spectrum_kernel, dim3((unsigned)(tap_rows * fg.n_part)), dim3(fdr::kThreads), lds_r, s, nya,
                           fg.n_part, ya, tw, H);
      }
      if (!run) return launch_check();
      int64_t blocks = dev_props().cu_count;
      if (blocks > rows * fg.segs) blocks = rows * fg.segs;
#define AAMD_FDR(NP) return launch(fdr::delay_line_kernel<NP>, blocks, fdr::kThreads, lds_r, s, fg, xa, tw, H, xmap, ymap, out)
      if (fg.n_part == 1) AAMD_FDR(1); else if (fg.n_part == 2) AAMD_FDR(2); else if (fg.n_part == 3) AAMD_FDR(3); else AAMD_FDR(4);
#undef AAMD_FDR
    }
    fco::FdlGeom f{};
    f.rows = rows; f.nx = nxa; f.ny = nya; f.start = start; f.out_len = out_len;
    if (fftconv_pick_fdl(rows, nya, out_len, f)) {
      // frequency-domain delay line: one forward + one inverse FFT per block step
      fco::Geom gs = g;
      gs.n_part = f.n_part; gs.part_taps = fco::kHop;
      AAMD_CHECK_ARG(tap_rows * f.n_part < (1ll << 31), "too many tap rows");
      if (prep)
        hipLaunchKernelGGL(fco::spectrum_kernel, dim3((unsigned)(tap_rows * f.n_part)), dim3(fco::kThreads), lds, s, gs,
                           ya, tw, H);
      if (!run) return launch_check();
      const int64_t n_spec = tap_rows * (f.n_part > g.n_part ? f.n_part : g.n_part);
      fco::C32* ring = H + n_spec * fco::kN;
      int64_t blocks = dev_props().cu_count;
      if (blocks > rows * f.segs) blocks = rows * f.segs;
#define AAMD_FDL(NP) return launch(fco::overlap_save_fdl_kernel<NP>, blocks, fco::kPhys, lds, s, f, xa, tw, H, ring, xmap, ymap, out)
      switch (f.n_part) {
        case 2: AAMD_FDL(2);
        case 3: AAMD_FDL(3);
        default: AAMD_FDL(4);
      }
#undef AAMD_FDL
    }
    AAMD_CHECK_ARG(tap_rows * g.n_part < (1ll << 31), "too many tap rows");
    if (prep)
      hipLaunchKernelGGL(fco::spectrum_kernel, dim3((unsigned)(tap_rows * g.n_part)), dim3(fco::kThreads), lds, s, g,
                         ya, tw, H);
    if (!run) return launch_check();
    const int64_t items = rows * g.n_pairs;
    int64_t blocks = dev_props().cu_count;
    if (blocks > items) blocks = items;
    hipLaunchKernelGGL(fco::overlap_save_kernel, dim3((unsigned)blocks), dim3(fco::kPhys), lds, s, g, xa, tw, H,
                       xmap, ymap, out);
    return launch_check();
  }
  if (!run) return AAMD_OK;             // the time-domain kernel reads the taps as they are: nothing to prepare
  FcGeom g;
  g.rows = rows; g.start = start; g.out_len = out_len;
  g.nx = nxa;
  g.ny = nya;
  g.n_tiles = (int)((out_len + kFcTN - 1) / kFcTN);
  const int64_t blocks = rows * g.n_tiles;
  AAMD_CHECK_ARG(blocks < (1ll << 31), "too many tiles for one launch");
  return launch(fftconv_direct_kernel, blocks, kFcThreads, 0, s, g, xa, ya, xmap, ymap, out);
}

}  // extern "C"
