// CPU replay of the STOI kernels (audio_amd/csrc/stoi.h compiled with g++, no GPU): each driver mirrors its kernel with the
// launch geometry of the C ABI -- "all threads run a phase, then __syncthreads()" is a loop over thread ids, LDS is a local
// array.  The caller owns every buffer, the workspaces included, so a test can look at each phase's output.  What a kernel
// leaves unwritten stays as the caller filled it.  TEST INFRASTRUCTURE ONLY.
#include <cstdint>
#include <vector>

#include "../../audio_amd/csrc/stoi.h"

using namespace aamd;
using stoi::kThreads;

template <int DT>
static void energy_block(const stoi::Args& a, int64_t row, int64_t blk) {
  double w[stoi::kFrame], red[kThreads];
  int any_bad = 0;
  const int64_t L = stoi::row_length(a, row);
  for (int tid = 0; tid < kThreads; ++tid) w[tid] = stoi::window64(tid);
  for (int tid = 0; tid < kThreads; ++tid) {
    red[tid] = stoi::energy_partial<DT>(tid, a, row, L, blk, w);
    if (stoi::nonfinite_thread<DT>(tid, a, row, L, blk)) any_bad = 1;
  }
  for (int stride = 16; stride > 0; stride >>= 1)
    for (int tid = 0; tid < kThreads; ++tid) stoi::energy_tree_step(tid, stride, red);    // ascending tid reads unwritten slots
  for (int tid = 0; tid < kThreads; ++tid) stoi::energy_write(tid, a, row, L, blk, red);
  a.bad[row * a.nb_e + blk] = any_bad;
}

static void select_row(const stoi::Args& a, int64_t row) {
  double smax[kThreads];
  int cnt[2][kThreads], mine[kThreads];
  const int64_t L = stoi::row_length(a, row);
  int64_t K_all = L < 0 ? 0 : stoi::frames_of(L);
  if (K_all > a.K_max) K_all = a.K_max;
  int any_bad = L < 0 ? 1 : 0;
  for (int tid = 0; tid < kThreads; ++tid) {
    if (stoi::select_bad(tid, a, row)) any_bad = 1;
    smax[tid] = stoi::select_max(tid, a, row, K_all);
  }
  for (int stride = kThreads >> 1; stride > 0; stride >>= 1)
    for (int tid = 0; tid < kThreads; ++tid) stoi::max_step(tid, stride, smax);
  const double mx = smax[0];
  for (int tid = 0; tid < kThreads; ++tid) cnt[0][tid] = mine[tid] = stoi::select_count(tid, a, row, K_all, mx);
  int cur = 0;
  for (int stride = 1; stride < kThreads; stride <<= 1) {
    for (int tid = 0; tid < kThreads; ++tid) stoi::scan_step(tid, stride, cnt[cur], cnt[cur ^ 1]);
    cur ^= 1;
  }
  for (int tid = 0; tid < kThreads; ++tid) stoi::select_write(tid, a, row, K_all, mx, cnt[cur][tid] - mine[tid]);
  a.n_kept[row] = any_bad ? -1 : cnt[cur][kThreads - 1];
}

template <int DT>
static void tob_block(const stoi::Args& a, int64_t row, int64_t blk) {
  using C = typename stoi::Elem<DT>::C;
  std::vector<C> lds(stoi::kTobWords, (C)12345);
  C *w = lds.data() + stoi::kTobW, *twr = lds.data() + stoi::kTobTwr, *twi = lds.data() + stoi::kTobTwi;
  C *xs = lds.data() + stoi::kTobXs, *ys = lds.data() + stoi::kTobYs;
  int64_t K, M;
  if (!stoi::row_frames(a, row, K, M) || blk * stoi::kTobFrames >= M) return;
  const int64_t L = stoi::row_length(a, row);
  const int64_t K_all = L < 0 ? 0 : stoi::frames_of(L);
  for (int tid = 0; tid < kThreads; ++tid) stoi::tob_tables(tid, w, twr, twi);
  for (int tid = 0; tid < kThreads; ++tid) stoi::tob_gather<DT>(tid, a, row, K, K_all, blk, w, xs, ys);
  for (int rnd = 0; rnd < stoi::kTobFrames / 4; ++rnd) {
    for (int wave = 0; wave < 4; ++wave) {
      C* re = lds.data() + stoi::kTobPlanes + wave * 2 * stoi::kPlane;
      C* im = re + stoi::kPlane;
      C* pw = lds.data() + stoi::kTobPw + wave * 2 * stoi::kBins;
      const int fl = rnd * 4 + wave;
      const int64_t m = blk * stoi::kTobFrames + fl;
      if (m >= M) continue;
      for (int lane = 0; lane < 64; ++lane) stoi::tob_frame_load(lane, fl, w, xs, ys, re, im);
      for (int s = 1; s < stoi::kLogFft; ++s)
        for (int lane = 0; lane < 64; ++lane) stoi::tob_fft_stage(lane, s, twr, twi, re, im);
      for (int lane = 0; lane < 64; ++lane) stoi::tob_power(lane, re, im, pw);
      for (int lane = 0; lane < 64; ++lane) stoi::tob_bands(lane, a, row, m, pw);
    }
  }
}

template <typename C>
static void segment_block(const stoi::Args& a, int64_t row, int64_t tile) {
  double tx[stoi::kSegRows * stoi::kBands], ty[stoi::kSegRows * stoi::kBands], stat[stoi::kSegTile * stoi::kBands * 4], red[kThreads];
  int64_t K, M;
  if (!stoi::row_frames(a, row, K, M)) return;
  const int64_t J = M - stoi::kSeg + 1, s0 = tile * stoi::kSegTile;
  if (s0 >= J) return;
  for (int tid = 0; tid < kThreads; ++tid) stoi::seg_stage<C>(tid, a, row, M, s0, tx, ty);
  auto live = [&](int tid) { return tid / stoi::kBands < stoi::kSegTile && s0 + tid / stoi::kBands < J; };
  if (a.extended)
    for (int tid = 0; tid < kThreads; ++tid)
      if (live(tid)) stoi::seg_estoi_rows(tid / stoi::kBands, tid % stoi::kBands, tx, ty, stat + tid * 4);
  for (int tid = 0; tid < kThreads; ++tid) {
    const int sl = tid / stoi::kBands, b = tid % stoi::kBands;
    double v = 0.0;
    if (live(tid)) {
      if (a.extended)
        v = stoi::seg_estoi_col(sl, b, tx, ty, stat + sl * stoi::kBands * 4) +
            stoi::seg_estoi_col(sl, b + stoi::kBands, tx, ty, stat + sl * stoi::kBands * 4);
      else
        v = stoi::seg_stoi_lane(sl, b, tx, ty);
    }
    red[tid] = v;
  }
  for (int stride = kThreads >> 1; stride > 0; stride >>= 1)
    for (int tid = 0; tid < kThreads; ++tid) stoi::sum_step(tid, stride, red);
  a.part[row * a.nt_seg + tile] = red[0];
}

template <typename C>
static void finish_row(const stoi::Args& a, int64_t row) {
  double red[stoi::kFinishThreads];
  int64_t J, tiles;
  const double fixed = stoi::finish_fixed(a, row, J, tiles);
  for (int tid = 0; tid < stoi::kFinishThreads; ++tid) red[tid] = stoi::finish_partial(tid, a, row, tiles);
  for (int stride = stoi::kFinishThreads >> 1; stride > 0; stride >>= 1)
    for (int tid = 0; tid < stoi::kFinishThreads; ++tid) stoi::sum_step(tid, stride, red);
  static_cast<C*>(a.out)[row] = (C)(J > 0 ? stoi::score_of(a, red[0], J) : fixed);
}

template <int DT>
static void run(const stoi::Args& a) {
  using C = typename stoi::Elem<DT>::C;
  for (int64_t row = 0; row < a.rows; ++row)
    for (int64_t blk = 0; blk < a.nb_e; ++blk) energy_block<DT>(a, row, blk);
  for (int64_t row = 0; row < a.rows; ++row) select_row(a, row);
  if (a.nt_seg > 0) {
    const int64_t nblk = stoi::ceil_div(a.M_max, stoi::kTobFrames);
    for (int64_t row = 0; row < a.rows; ++row)
      for (int64_t blk = 0; blk < nblk; ++blk) tob_block<DT>(a, row, blk);
    for (int64_t row = 0; row < a.rows; ++row)
      for (int64_t tile = 0; tile < a.nt_seg; ++tile) segment_block<C>(a, row, tile);
  }
  for (int64_t row = 0; row < a.rows; ++row) finish_row<C>(a, row);
}

extern "C" {

int sim_stoi_tiles(int which) {
  const int v[5] = {stoi::kThreads, stoi::kEnergyFrames, stoi::kTobFrames, stoi::kSegTile, stoi::kFinishThreads};
  return which >= 0 && which < 5 ? v[which] : 0;
}

// dims out: K_max, M_max, nb_e, nt_seg of rows of T samples (the launcher's layout)
void sim_stoi_dims(int64_t T, int64_t* dims) {
  dims[0] = stoi::frames_of(T);
  dims[1] = dims[0] > 0 ? dims[0] - 1 : 0;
  dims[2] = dims[0] > 0 ? stoi::ceil_div(dims[0], stoi::kEnergyFrames) : 1;
  dims[3] = dims[1] >= stoi::kSeg ? stoi::ceil_div(dims[1] - stoi::kSeg + 1, stoi::kSegTile) : 0;
}

int sim_stoi(int dtype, const void* preds, const void* target, int64_t rows, int64_t T, int64_t sp, int64_t st, const void* lengths,
             int len64, int extended, double* e, int32_t* bad, int32_t* kept, int32_t* n_kept, void* tob, double* part, void* out) {
  int64_t dims[4];
  sim_stoi_dims(T, dims);
  stoi::Args a{};
  a.x = target; a.y = preds; a.lengths = lengths;
  a.rows = rows; a.T = T; a.sx = rows > 1 ? st : 0; a.sy = rows > 1 ? sp : 0;
  a.K_max = dims[0]; a.M_max = dims[1]; a.nb_e = dims[2]; a.nt_seg = dims[3];
  a.len64 = len64; a.extended = extended;
  a.e = e; a.bad = bad; a.kept = kept; a.n_kept = n_kept; a.tob = tob; a.part = part; a.out = out;
  switch (dtype) {
    case 0: run<wa::kF32>(a); break;
    case 1: run<wa::kF64>(a); break;
    case 2: run<wa::kF16>(a); break;
    case 3: run<wa::kBF16>(a); break;
    default: return -1;
  }
  return 0;
}

}  // extern "C"
