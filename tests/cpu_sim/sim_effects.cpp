// CPU replay of the effects kernels (audio_amd/csrc/effects.h compiled with g++, no GPU): each driver mirrors its __global__
// kernel, "all threads run phase X, then __syncthreads()" replaced by a loop over thread ids, with the launch geometry and
// the workspace layout of the C ABI.  TEST INFRASTRUCTURE ONLY.
#include <cstdint>
#include <vector>

#include "../../audio_amd/csrc/effects.h"

using namespace aamd;

template <int DT, bool FLANGER>
static int delay(fx::DelayArgs a) {                                 // delay_kernel
  using C = typename wa::Elem<DT>::C;
  std::vector<C> tile((size_t)fx::kRows * fx::kPitch), rings((size_t)fx::kRows * a.L);
  std::vector<uint32_t> tab((size_t)fx::kMaxChannels * fx::kTile);
  for (int64_t grp = 0; grp < fx::n_groups(a.rows); ++grp) {
    std::vector<fx::Lane<C>> st(fx::kRows);
    for (int lane = 0; lane < fx::kRows; ++lane) {
      const int64_t row = grp * fx::kRows + lane;
      const bool active = row < a.rows;
      fx::lane_init(st[lane]);
      if (active) fx::ring_clear(a, rings.data() + lane);
    }
    for (int64_t t0 = 0; t0 < a.T; t0 += fx::kTile) {
      for (int lane = 0; lane < fx::kRows; ++lane) {
        wa::Vec<typename wa::Elem<DT>::S> regs[fx::kTile * sizeof(typename wa::Elem<DT>::S) / 16];
        fx::tile_fetch<DT>(lane, a, grp, t0, regs);
        fx::tile_put<DT>(lane, a, grp, t0, regs, tile.data());
        fx::table_load(lane, a, t0, tab.data());
      }
      const int n = a.T - t0 < fx::kTile ? (int)(a.T - t0) : fx::kTile;
      for (int lane = 0; lane < fx::kRows; ++lane) {
        const int64_t row = grp * fx::kRows + lane;
        if (row >= a.rows) continue;
        const uint32_t* mytab = tab.data() + (row % a.channels) * fx::kTile;
        if (FLANGER) fx::flanger_lane(a, st[lane], tile.data() + lane * fx::kPitch, rings.data() + lane, mytab, n);
        else fx::phaser_lane(a, st[lane], tile.data() + lane * fx::kPitch, rings.data() + lane, mytab, n);
      }
      for (int lane = 0; lane < fx::kRows; ++lane) fx::tile_store<DT>(lane, a, grp, t0, tile.data());
    }
  }
  return 0;
}

template <int DT>
static int stream(fx::DelayArgs a) {                                // stream_kernel
  const int64_t chunks = wa::n_chunks(a.T);
  for (int64_t blk = 0; blk < a.rows * chunks; ++blk) {
    const int64_t row = blk / chunks, chunk = blk - row * chunks;
    for (int tid = 0; tid < wa::kThreads; ++tid) fx::stream_thread<DT>(tid, a, row, chunk);
  }
  return 0;
}

static const double* scan(const double* pw, std::vector<double> (&s)[2]) {
  for (int l = 0; l < fx::kOdLevels; ++l)
    for (int tid = 0; tid < fx::kOdThreads; ++tid) fx::od_scan_step(tid, l, pw, s[l & 1].data(), s[(l + 1) & 1].data());
  return s[fx::kOdLevels & 1].data();
}

template <int DT>
static int overdrive(fx::OdArgs a) {
  using S = typename wa::Elem<DT>::S;
  using C = typename wa::Elem<DT>::C;
  constexpr int NV = fx::kOdSeg * sizeof(S) / 16;
  struct Seg {
    wa::Vec<S> xv[NV];
    C t[fx::kOdSeg], tprev;
  };
  std::vector<Seg> seg(fx::kOdThreads);
  std::vector<double> s[2] = {std::vector<double>(fx::kOdThreads), std::vector<double>(fx::kOdThreads)};
  double pw[fx::kOdLevels + 1];
  fx::od_powers<C>(pw);
  if (a.chunks > 1)
    for (int64_t blk = 0; blk < a.rows * a.chunks; ++blk) {         // overdrive_reduce_kernel
      const int64_t row = blk / a.chunks, chunk = blk - row * a.chunks;
      for (int tid = 0; tid < fx::kOdThreads; ++tid) {
        fx::od_fetch<DT>(tid, a, row, chunk, seg[tid].xv, seg[tid].t, seg[tid].tprev);
        s[0][tid] = fx::od_segment_end(seg[tid].t, seg[tid].tprev, 0.0);
      }
      a.ws[row * a.chunks + chunk] = scan(pw, s)[fx::kOdThreads - 1];
    }
  for (int64_t blk = 0; blk < a.rows * a.chunks; ++blk) {           // overdrive_apply_kernel
    const int64_t row = blk / a.chunks, chunk = blk - row * a.chunks;
    for (int tid = 0; tid < fx::kOdThreads; ++tid)
      fx::od_fetch<DT>(tid, a, row, chunk, seg[tid].xv, seg[tid].t, seg[tid].tprev);
    double y0 = 0.0;
    for (int64_t base = 0; base < chunk; base += fx::kOdThreads) {
      const int n = chunk - base < fx::kOdThreads ? (int)(chunk - base) : fx::kOdThreads;
      for (int tid = 0; tid < n; ++tid) s[0][tid] = a.ws[row * a.chunks + base + tid];
      y0 = fx::od_horner(y0, pw[fx::kOdLevels], s[0].data(), n);
    }
    for (int tid = 0; tid < fx::kOdThreads; ++tid)
      s[0][tid] = fx::od_segment_end(seg[tid].t, seg[tid].tprev, tid == 0 ? y0 : 0.0);
    const double* r = scan(pw, s);
    for (int tid = 0; tid < fx::kOdThreads; ++tid)
      fx::od_write<DT>(tid, a, row, chunk, seg[tid].xv, seg[tid].t, seg[tid].tprev, tid == 0 ? y0 : r[tid - 1]);
  }
  return 0;
}

extern "C" {

int sim_fx_tiles(int which) { return which == 0 ? fx::kRows : (which == 1 ? fx::kTile : fx::kOdChunk); }
int sim_fx_ring_in_lds(int dtype, int64_t L) {
  return dtype == wa::kF64 ? fx::ring_in_lds<double>(L) : fx::ring_in_lds<float>(L);
}

// flanger: 0 phaser (table int32, g = gain_in, decay, gain_out), 1 flanger (table float, g = feedback, in, delay gain);
// general = 0 with a zero feedback gain: the streaming kernel.  Returns < 0 on an unknown dtype.
int sim_fx_delay(int dtype, int flanger, int general, const void* x, void* out, int64_t rows, int64_t T, int64_t sx,
                 const void* table, int64_t M, int64_t L, int channels, const int64_t* cph, double g0, double g1, double g2,
                 int quadratic) {
  fx::DelayArgs a{};
  a.x = x; a.out = out; a.ws = nullptr; a.table = table;
  a.rows = rows; a.T = T; a.sx = sx; a.M = M;
  for (int c = 0; c < channels && c < fx::kMaxChannels; ++c) a.cph[c] = cph ? cph[c] : 0;
  a.g0 = g0; a.g1 = g1; a.g2 = g2;
  a.L = (int32_t)L; a.channels = channels; a.quadratic = quadratic;
  if (flanger && !general && g0 == 0.0) {
    switch (dtype) {
      case wa::kF32: return stream<wa::kF32>(a);
      case wa::kF64: return stream<wa::kF64>(a);
      case wa::kF16: return stream<wa::kF16>(a);
      case wa::kBF16: return stream<wa::kBF16>(a);
      default: return -1;
    }
  }
  switch (dtype) {
    case wa::kF32: return flanger ? delay<wa::kF32, true>(a) : delay<wa::kF32, false>(a);
    case wa::kF64: return flanger ? delay<wa::kF64, true>(a) : delay<wa::kF64, false>(a);
    case wa::kF16: return flanger ? delay<wa::kF16, true>(a) : delay<wa::kF16, false>(a);
    case wa::kBF16: return flanger ? delay<wa::kBF16, true>(a) : delay<wa::kBF16, false>(a);
    default: return -1;
  }
}

// ws: rows * ceil(T / chunk) doubles
int sim_fx_overdrive(int dtype, const void* x, void* out, double* ws, int64_t rows, int64_t T, int64_t sx, double gain,
                     double colour) {
  fx::OdArgs a{};
  a.x = x; a.out = out; a.ws = ws; a.rows = rows; a.T = T; a.sx = sx; a.chunks = fx::od_chunks(T);
  a.gain = gain; a.colour = colour;
  switch (dtype) {
    case wa::kF32: return overdrive<wa::kF32>(a);
    case wa::kF64: return overdrive<wa::kF64>(a);
    case wa::kF16: return overdrive<wa::kF16>(a);
    case wa::kBF16: return overdrive<wa::kBF16>(a);
    default: return -1;
  }
}

}  // extern "C"
