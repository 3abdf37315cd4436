// STOI / ESTOI of the C ABI (csrc/stoi.h): exported constants, the workspace query and the five launches.
#include "api_common.h"
#include "stoi.h"

using namespace aamd;

namespace {

struct Layout {
  int64_t K_max, M_max, nb_e, nt_seg;
  int64_t e, part, tob, kept, bad, n_kept, total;       // byte offsets, each a multiple of 8
};

int64_t up8(int64_t v) { return (v + 7) & ~(int64_t)7; }

Layout layout_of(int32_t dtype, int64_t rows, int64_t T) {
  Layout l{};
  l.K_max = stoi::frames_of(T);
  l.M_max = l.K_max > 0 ? l.K_max - 1 : 0;
  l.nb_e = l.K_max > 0 ? stoi::ceil_div(l.K_max, stoi::kEnergyFrames) : 1;
  l.nt_seg = l.M_max >= stoi::kSeg ? stoi::ceil_div(l.M_max - stoi::kSeg + 1, stoi::kSegTile) : 0;
  const int64_t csize = dtype == AAMD_SA_F64 ? 8 : 4;
  l.e = 0;
  l.part = l.e + rows * l.K_max * 8;
  l.tob = l.part + rows * l.nt_seg * 8;
  l.kept = l.tob + up8(rows * 2 * l.M_max * stoi::kBands * csize);
  l.bad = l.kept + up8(rows * l.K_max * 4);
  l.n_kept = l.bad + up8(rows * l.nb_e * 4);
  l.total = l.n_kept + up8(rows * 4);
  return l;
}

template <int DT>
int run(const stoi::Args& a, hipStream_t s) {
  using C = typename stoi::Elem<DT>::C;
  int rc = launch(stoi::energy_kernel<DT>, a.rows * a.nb_e, stoi::kThreads, 0, s, a);
  if (rc != AAMD_OK) return rc;
  rc = launch(stoi::select_kernel, a.rows, stoi::kThreads, 0, s, a);
  if (rc != AAMD_OK) return rc;
  if (a.nt_seg > 0) {
    rc = launch(stoi::tob_kernel<DT>, a.rows * stoi::ceil_div(a.M_max, stoi::kTobFrames), stoi::kThreads, stoi::tob_lds_bytes<C>(), s, a);
    if (rc != AAMD_OK) return rc;
    rc = launch(stoi::segment_kernel<C>, a.rows * a.nt_seg, stoi::kThreads, 0, s, a);
    if (rc != AAMD_OK) return rc;
  }
  return launch(stoi::finish_kernel<C>, a.rows, stoi::kFinishThreads, 0, s, a);
}

}  // namespace

extern "C" {

int32_t aamd_stoi_tiles(int32_t which) {
  switch (which) {
    case 0: return stoi::kThreads;
    case 1: return stoi::kEnergyFrames;
    case 2: return stoi::kTobFrames;
    case 3: return stoi::kSegTile;
    case 4: return stoi::kFinishThreads;
    default: return 0;
  }
}

int64_t aamd_stoi_workspace(int32_t dtype, int64_t rows, int64_t length) {
  if (rows <= 0 || length < 0 || length >= (1ll << 40)) return 0;
  return layout_of(dtype, rows, length).total;
}

int aamd_stoi(int32_t dtype, const void* preds, const void* target, int64_t rows, int64_t length, int64_t preds_stride,
              int64_t target_stride, const void* lengths, int32_t lengths_int64, int32_t extended, void* workspace, void* out,
              void* stream) {
  DeviceScope dev_scope_(out);
  AAMD_CHECK_ARG(dtype >= AAMD_SA_F32 && dtype <= AAMD_SA_BF16, "stoi: unknown element type");
  AAMD_CHECK_ARG(rows >= 0 && length >= 0 && preds_stride >= 0 && target_stride >= 0, "stoi: bad sizes");
  AAMD_CHECK_ARG(rows < (1ll << 31) && length < (1ll << 40), "stoi: too many rows or samples");
  if (rows == 0) return AAMD_OK;
  AAMD_CHECK_ARG(rows == 1 || (preds_stride >= length && target_stride >= length), "stoi: rows overlap");
  const Layout l = layout_of(dtype, rows, length);
  AAMD_CHECK_ARG(rows * l.nb_e < (1ll << 31) && rows * stoi::ceil_div(l.M_max, stoi::kTobFrames) < (1ll << 31),
                 "stoi: too many workgroups");
  AAMD_CHECK_ARG(workspace && out && ((preds && target) || length == 0), "null buffer");
  const uintptr_t emask = (uintptr_t)((dtype == AAMD_SA_F64 ? 8 : (dtype == AAMD_SA_F32 ? 4 : 2)) - 1);
  AAMD_CHECK_ARG((((uintptr_t)preds | (uintptr_t)target) & emask) == 0, "stoi: a waveform is not aligned to its element");
  AAMD_CHECK_ARG(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)out & (dtype == AAMD_SA_F64 ? 7 : 3)) == 0 &&
                     ((uintptr_t)lengths & (lengths_int64 ? 7 : 3)) == 0,
                 "stoi: a buffer is misaligned");
  char* ws = static_cast<char*>(workspace);
  stoi::Args a{};
  a.x = target; a.y = preds; a.lengths = lengths;
  a.rows = rows; a.T = length; a.sx = rows > 1 ? target_stride : 0; a.sy = rows > 1 ? preds_stride : 0;
  a.K_max = l.K_max; a.M_max = l.M_max; a.nb_e = l.nb_e; a.nt_seg = l.nt_seg;
  a.len64 = lengths_int64 ? 1 : 0; a.extended = extended ? 1 : 0;
  a.e = reinterpret_cast<double*>(ws + l.e);
  a.part = reinterpret_cast<double*>(ws + l.part);
  a.tob = ws + l.tob;
  a.kept = reinterpret_cast<int32_t*>(ws + l.kept);
  a.bad = reinterpret_cast<int32_t*>(ws + l.bad);
  a.n_kept = reinterpret_cast<int32_t*>(ws + l.n_kept);
  a.out = out;
  hipStream_t s = (hipStream_t)stream;
  switch (dtype) {
    case AAMD_SA_F32: return run<wa::kF32>(a, s);
    case AAMD_SA_F64: return run<wa::kF64>(a, s);
    case AAMD_SA_F16: return run<wa::kF16>(a, s);
    default: return run<wa::kBF16>(a, s);
  }
}

}  // extern "C"
