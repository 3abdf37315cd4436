// CPU replay of the CTC beam search kernels (audio_amd/csrc/ctc_decoder.h compiled with g++, no GPU): each driver mirrors its
// __global__ kernel with the launch geometry of the C ABI -- "all lanes run a phase, then __syncthreads()" is a loop over
// lanes; the ballot is a loop over 64 frames and the folds over the wave are loops over the lanes' picks.
// TEST INFRASTRUCTURE ONLY.
#include <cstdint>
#include <set>
#include <vector>

#include "../../audio_amd/csrc/ctc_decoder.h"

using namespace aamd;

// prefixes that were appended to a trie a second time: they had left the beam and came back (counted by the driver alone, from
// the hashes of the entries that append a node)
static long g_returned = 0;

template <int DT>
static void row_run(const cd::Args& a) {
  for (int64_t row = 0; row < a.B * a.T; ++row) {
    int Tb;
    if (!cd::len_ok(a, row / a.T, Tb) || row % a.T >= Tb) continue;
    bool skip = false;
    for (int lane = 0; lane < 64; ++lane) skip = cd::row_head<DT>(a, row, lane);
    if (skip) continue;
    cd::RowPick prev = cd::row_none();
    std::vector<cd::RowPick> mine(64, cd::row_none());
    for (int r = 0; r < a.R; ++r) {
      cd::RowPick g = cd::row_none();
      for (int lane = 0; lane < 64; ++lane) {
        if (cd::row_rescan(r, mine[lane], prev)) mine[lane] = cd::row_scan<DT>(a, row, lane, r == 0, prev);
        if (cd::row_before(mine[lane], g)) g = mine[lane];
      }
      cd::row_store(a, row, r, g);
      prev = g;
    }
  }
}

template <int DT>
static void beam_run(const cd::Args& a) {
  constexpr int NT = cd::kBeamThreads;
  std::vector<cd::Shared> shared(1);
  cd::Shared& S = shared[0];
  for (int64_t b = 0; b < a.B; ++b) {
    int Tb;
    if (!cd::len_ok(a, b, Tb)) {
      for (int lane = 0; lane < NT; ++lane) cd::flagged(a, b, lane);
      continue;
    }
    for (int lane = 0; lane < NT; ++lane) cd::beam_init(a, b, lane, S);
    int cur = 0;
    int32_t count = 1;
    std::set<uint64_t> seen;
    std::vector<cd::Rec> rec(NT);
    std::vector<double> g(NT);
    for (int64_t t0 = 0; t0 < Tb; t0 += 64) {
      std::vector<int64_t> frames;
      for (int lane = 0; lane < 64; ++lane)
        if (cd::frame_live(a, b, t0 + lane, Tb)) frames.push_back(t0 + lane);
      for (size_t f = 0; f < frames.size(); ++f) {
        for (int lane = 0; lane < NT; ++lane) {
          rec[lane] = cd::rec_load(a, b, frames[f], lane);
          cd::rec_publish(a, lane, rec[lane], S);
          cd::frame_begin(lane, cur, S);
          g[lane] = cd::gather<DT>(a, b, frames[f], lane, cur, S);
        }
        for (int lane = 0; lane < NT; ++lane) cd::fill(a, b, lane, cur, false, S);
        for (int lane = 0; lane < NT; ++lane) cd::gather_publish(lane, g[lane], S);
        for (int lane = 0; lane < NT; ++lane) cd::fill(a, b, lane, cur, true, S);
        for (int lane = 0; lane < NT; ++lane) cd::select(a, lane, cur, S);
        cur ^= 1;
        for (int k = 0; k < S.n[cur]; ++k)
          if (S.ext[k] && !seen.insert(S.hash[cur][k]).second) ++g_returned;
        int32_t added = 0;
        for (int lane = 0; lane < NT; ++lane) added = cd::append_nodes(a, b, lane, cur, count, S);
        count += added;
      }
    }
    for (int lane = 0; lane < NT; ++lane) cd::finish(a, b, lane, cur, S);
    for (int lane = 0; lane < NT; ++lane) cd::zero_fill(a, b, lane, S);
  }
}

template <int DT>
static void run(const cd::Args& a) {
  row_run<DT>(a);
  beam_run<DT>(a);
}

extern "C" {

long sim_cd_returned_prefixes() { return g_returned; }

int sim_cd_max_beam() { return cd::kMaxBeam; }
int sim_cd_row_threads() { return cd::kRowThreads; }
int sim_cd_beam_threads() { return cd::kBeamThreads; }
int sim_cd_record_slots(int beam) { cd::Args a{}; a.K = beam; a.T = 1; cd::ws_bind(a, nullptr); return a.R; }
int sim_cd_candidates(int beam) { cd::Args a{}; a.K = beam; a.T = 1; cd::ws_bind(a, nullptr); return a.K * a.R2; }
int64_t sim_cd_workspace(int64_t B, int64_t T, int64_t K) { return cd::sizes_ok(B, T, K) ? cd::ws_bytes(B, T, K) : 0; }

// dims: B, T, V
int sim_ctc_beam_search(int dtype, const void* lp, const void* len, int len64, const int64_t* dims, int blank, int beam, int nbest,
                        double thr, void* ws, int32_t* tokens, int32_t* out_len, double* scores) {
  cd::Args a{};
  a.lp = lp; a.len = len;
  a.B = dims[0]; a.T = dims[1]; a.V = dims[2];
  if (!cd::sizes_ok(a.B, a.T, beam) || nbest < 1 || nbest > beam || a.V < 2 || blank < 0 || blank >= a.V) return -2;
  a.blank = blank; a.len64 = len64; a.K = beam; a.N = nbest; a.thr = thr;
  a.tokens = tokens; a.out_len = out_len; a.scores = scores;
  cd::ws_bind(a, ws);
  switch (dtype) {
    case wa::kF32: run<wa::kF32>(a); break;
    case wa::kF64: run<wa::kF64>(a); break;
    case wa::kF16: run<wa::kF16>(a); break;
    default: run<wa::kBF16>(a); break;
  }
  return 0;
}

}  // extern "C"
