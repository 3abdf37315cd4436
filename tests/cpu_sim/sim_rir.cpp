// CPU replay of the image-source kernel (audio_amd/csrc/rir.h compiled with g++, no GPU): the driver mirrors rir_kernel,
// "all threads run phase X, then __syncthreads()" replaced by a loop over thread ids and the wave ballots by a loop over the
// lanes of each wave, with the launch geometry and the LDS layout of the C ABI.  TEST INFRASTRUCTURE ONLY.
#include <cstdint>
#include <vector>

#include "../../audio_amd/csrc/rir.h"

using namespace aamd;

template <int DT>
static void run(const rir::Args& a) {                                  // rir_kernel
  std::vector<double> smem(rir::lds_doubles(a.order, a.pad));
  std::vector<rir::Lists> lists(2);
  std::vector<rir::Term> term(rir::kThreads);
  double* pw = smem.data();
  double* cs = pw + 6 * rir::pow_rows(a.order);
  for (int64_t blk = 0; blk < a.B * a.M * a.tiles; ++blk) {
    const int64_t row = blk / a.tiles, tile = blk - row * a.tiles;
    const int64_t b = row / a.M, c = row - b * a.M, t0 = tile * rir::kTile;
    for (int tid = 0; tid < rir::kThreads; ++tid) rir::build_powers<DT>(tid, a, b, pw);
    for (int tid = 0; tid < rir::kThreads; ++tid) rir::build_hann(tid, a, cs);
    std::vector<double> acc((size_t)rir::kTile, 0.0);
    bool bad = false;
    int buf = 0;
    for (int64_t i0 = 0; i0 < a.n_img; i0 += rir::kChunk, buf ^= 1) {
      unsigned long long masks[rir::kWaves] = {}, bad_masks[rir::kWaves] = {};
      for (int tid = 0; tid < rir::kThreads; ++tid) {
        term[tid] = rir::Term{};
        if (i0 + tid < a.n_img) term[tid] = rir::image_term<DT>(a, b, c, i0 + tid, t0, pw);
        if (term[tid].meets) masks[tid >> 6] |= 1ull << (tid & 63);
        if (term[tid].bad) bad_masks[tid >> 6] |= 1ull << (tid & 63);
      }
      for (int tid = 0; tid < rir::kThreads; ++tid) rir::list_write(tid, term[tid], masks, lists[buf]);
      const int count = rir::list_slot(rir::kThreads, masks);
      for (int w = 0; w < rir::kWaves; ++w) bad = bad || bad_masks[w] != 0;
      for (int w = 0; w < rir::kWaves; ++w)
        for (int r0 = 0; r0 < count; r0 += 64)
          for (int p = 0; p < rir::kPerLane; ++p) {
            const int32_t n_lo = (int32_t)t0 + p * rir::kThreads + 64 * w;
            unsigned long long hits = 0;                                  // the wave's ballot
            for (int lane = 0; lane < 64; ++lane)
              if (rir::lane_hit(lane, n_lo, a, lists[buf], r0, count)) hits |= 1ull << lane;
            for (int lane = 0; lane < 64; ++lane)
              rir::add_hits(a, n_lo + lane, lists[buf], r0, hits, cs, acc[(size_t)p * rir::kThreads + 64 * w + lane]);
          }
    }
    for (int tid = 0; tid < rir::kThreads; ++tid)
      for (int j = 0; j < rir::kPerLane; ++j)
        rir::store<DT>(a, row, t0 + j * rir::kThreads + tid, acc[(size_t)j * rir::kThreads + tid], bad);
  }
}

extern "C" {

int sim_rir_tiles(int which) {
  return which == 0 ? rir::kTile : (which == 1 ? rir::kChunk : (which == 2 ? rir::kMaxFl : rir::kMaxOrder));
}

// the buffers of aamd_simulate_rir on the host; < 0 on an argument the C ABI refuses
int sim_rir(int dtype, const void* room, const void* source, const void* mic, const void* absorption, const int16_t* lattice,
            int64_t n_img, void* out, int64_t B, int64_t M, int D, int order, int fl, int64_t L, double sample_rate,
            double sound_speed) {
  if ((dtype != rir::kF32 && dtype != rir::kF64) || (D != 2 && D != 3) || order < 0 || fl < 3 || !(fl & 1) || L < 1 || n_img < 1)
    return -1;
  if (order > rir::kMaxOrder || fl > rir::kMaxFl) return -2;
  rir::Args a{};
  a.room = room; a.source = source; a.mic = mic; a.absorption = absorption; a.lattice = lattice; a.out = out;
  a.B = B; a.M = M; a.L = L; a.n_img = n_img; a.tiles = (L + rir::kTile - 1) / rir::kTile;
  a.sample_rate = sample_rate; a.sound_speed = sound_speed;
  a.D = D; a.order = order; a.pad = fl / 2;
  if (dtype == rir::kF64) run<rir::kF64>(a);
  else run<rir::kF32>(a);
  return 0;
}

}  // extern "C"
