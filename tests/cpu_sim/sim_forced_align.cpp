// CPU replay of the forced-alignment kernels (audio_amd/csrc/forced_align.h compiled with g++, no GPU): each driver mirrors
// its __global__ kernel with the launch geometry of the C ABI -- "all threads run a phase, then __syncthreads()" is a loop over
// thread ids; the one-lane shift of a wave reads the previous lane's value of before the step, and the first lane of a wave
// reads the LDS line as the kernel does.  TEST INFRASTRUCTURE ONLY.
#include <cstdint>
#include <vector>

#include "../../audio_amd/csrc/forced_align.h"

using namespace aamd;

template <int DT, int KS, int NT>
static void forward_run(const fa::Args& a) {
  constexpr int WAVES = NT / 64;
  std::vector<fa::Lane<DT, KS>> lanes(NT);
  std::vector<double> last(NT), left(NT);
  for (int64_t b = 0; b < a.B; ++b) {
    double line[2][WAVES];
    fa::Geom g;
    const bool ok = fa::lens_ok(a, b, g);
    int s_bad = 0, s_rep = 0;
    for (int tid = 0; ok && tid < NT; ++tid) {
      int bad, rep;
      fa::scan_labels(a, g, tid, NT, bad, rep);
      s_bad |= bad;
      s_rep += rep;
    }
    if (!ok || s_bad || g.Tb < g.Lb + s_rep) {
      a.info[g.b] = -1;
      continue;
    }
    for (int tid = 0; tid < NT; ++tid) {
      fa::lane_setup<DT, KS>(a, g, tid, lanes[tid]);
      for (int j = 0; j < fa::kPF; ++j) fa::fetch<DT, KS>(a, g, j, j, lanes[tid]);
    }
    auto lefts = [&](int64_t t) {
      for (int tid = 0; tid < NT; ++tid) last[tid] = lanes[tid].alpha[KS - 1];
      for (int tid = 0; tid < NT; ++tid) {
        double l = tid ? last[tid - 1] : 0.0;
        if (WAVES > 1 && (tid & 63) == 0 && tid) l = line[(t & 1) ^ 1][(tid >> 6) - 1];
        left[tid] = tid ? l : fa::neg_inf();
      }
    };
    auto publish = [&](int64_t t) {
      if (WAVES > 1)
        for (int tid = 63; tid < NT; tid += 64) line[t & 1][tid >> 6] = lanes[tid].alpha[KS - 1];
    };
    auto frame = [&](int64_t t, int j) {
      lefts(t);
      for (int tid = 0; tid < NT; ++tid) fa::advance<DT, KS>(a, g, t, j, tid, left[tid], lanes[tid]);
      publish(t);
    };
    for (int tid = 0; tid < NT; ++tid) fa::first_step<DT, KS>(a, g, tid, lanes[tid]);
    publish(0);
    int64_t t0 = 1;
    for (; t0 + fa::kPF <= g.Tb; t0 += fa::kPF)
      for (int j = 0; j < fa::kPF; ++j) frame(t0 + j, (1 + j) % fa::kPF);
    for (int j = 0; j < fa::kPF - 1; ++j)
      if (t0 + j < g.Tb) frame(t0 + j, (1 + j) % fa::kPF);
    lefts(g.Tb);
    for (int tid = 0; tid < NT; ++tid) fa::finish<DT, KS>(a, g, tid, left[tid], lanes[tid]);
  }
}

template <int DT>
static void forward_dt(const fa::Args& a) {
  if (a.nt == 64) forward_run<DT, 4, 64>(a);
  else if (a.ks == 4) forward_run<DT, 4, 256>(a);
  else forward_run<DT, 16, 256>(a);
}

static void backtrack_run(const fa::Args& a) {
  std::vector<uint32_t> tri(fa::kBT * fa::kTriPitch);
  int states[fa::kBT];
  for (int64_t b = 0; b < a.B; ++b) {
    const int fin = a.info[b];
    if (fin < 0) {
      for (int tid = 0; tid < fa::kBtThreads; ++tid) fa::bt_fill(a, b, 0, true, tid);
      continue;
    }
    fa::Geom g;
    fa::lens_ok(a, b, g);
    for (int tid = 0; tid < fa::kBtThreads; ++tid) fa::bt_fill(a, b, g.Tb, false, tid);
    int s = fin;
    for (int64_t t_hi = g.Tb - 1; t_hi >= 0; t_hi -= fa::kBT) {
      for (auto& w : tri) w = 0xffffffffu;                  // what the triangle leaves out would walk as far as it can
      for (int tid = 0; tid < fa::kBtThreads; ++tid) fa::bt_fetch(a, b, t_hi, s, tid, tri.data());
      int st = s;
      const int n = fa::bt_walk(a, t_hi, st, tri.data(), states);
      s = st;
      for (int tid = 0; tid < fa::kBtThreads; ++tid) fa::bt_write(a, b, t_hi, n, states, tid);
    }
  }
}

extern "C" {

int sim_fa_states_per_lane(int64_t L) { int ks, nt; fa::config(L, ks, nt); return ks; }
int sim_fa_threads(int64_t L) { int ks, nt; fa::config(L, ks, nt); return nt; }
int sim_fa_prefetch() { return fa::kPF; }
int sim_fa_backtrack_block() { return fa::kBT; }
int sim_fa_max_l() { return fa::kMaxL; }
int64_t sim_fa_workspace(int64_t B, int64_t T, int64_t L) { return fa::ws_bytes(B, T, L); }

// dims: B, T, C, L
int sim_forced_align(int dtype, const void* lp, const void* targets, int tgt64, const void* in_len, const void* tg_len, int len64,
                     const int64_t* dims, int blank, void* ws, void* paths, void* scores) {
  fa::Args a{};
  a.lp = lp; a.targets = targets; a.in_len = in_len; a.tg_len = tg_len;
  a.B = dims[0]; a.T = dims[1]; a.C = dims[2]; a.L = dims[3];
  if (a.L > fa::kMaxL) return -2;
  a.blank = blank; a.tgt64 = tgt64; a.len64 = len64; a.dtype = dtype;
  a.paths = paths; a.scores = scores;
  fa::ws_bind(a, ws);
  switch (dtype) {
    case wa::kF32: forward_dt<wa::kF32>(a); break;
    case wa::kF64: forward_dt<wa::kF64>(a); break;
    case wa::kF16: forward_dt<wa::kF16>(a); break;
    default: forward_dt<wa::kBF16>(a); break;
  }
  backtrack_run(a);
  return 0;
}

}  // extern "C"
