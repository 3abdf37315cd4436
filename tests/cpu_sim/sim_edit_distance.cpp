// CPU replay of the edit-distance kernel (audio_amd/csrc/edit_distance.h compiled with g++, no GPU): the driver mirrors
// edit_kernel with the launch geometry of the C ABI -- "all threads run a phase, then __syncthreads()" is a loop over thread
// ids; the one-lane shift of a wave reads the previous lane's value of before the step, the first lane of a wave reads the LDS
// line, and the hypothesis tokens come from the ring as the kernel refills it.  What the kernel leaves unwritten (the line before
// the first step, ring slots before their first refill) holds a poison here.  TEST INFRASTRUCTURE ONLY.
#include <cstdint>
#include <vector>

#include "../../audio_amd/csrc/edit_distance.h"

using namespace aamd;

static const uint64_t kPoison = 0xdeadbeefdeadbeefull;

template <int KS, int NT>
static void pair_run(const ed::Args& a, int64_t pair) {
  constexpr int WAVES = NT / 64, RING = 2 * NT;
  uint64_t line[2][WAVES];
  std::vector<int64_t> ring(RING, (int64_t)kPoison), next(NT);
  std::vector<ed::Lane<KS>> lanes(NT);
  std::vector<uint64_t> last(NT), top(NT);
  for (int w = 0; w < WAVES; ++w) line[0][w] = line[1][w] = kPoison;
  ed::Geom g;
  if (!ed::lens_ok(a, pair, g)) {
    ed::write_bad(a, g.pair);
    return;
  }
  if (g.Mb == 0 || g.Nb == 0) {
    ed::write_result(a, g.pair, g.Mb == 0 ? ed::row0_cell(g.Nb) : ed::col0_cell(g.Mb));
    return;
  }
  for (int tid = 0; tid < NT; ++tid) ed::lane_setup<KS>(a, g, tid, lanes[tid]);
  const int total = ed::total_steps(g, KS);
  for (int tid = 0; tid < NT; ++tid) next[tid] = ed::hyp_token(a, g, tid);
  for (int s0 = 0; s0 < total; s0 += NT) {
    for (int tid = 0; tid < NT; ++tid) {
      ring[(s0 + tid) & (RING - 1)] = next[tid];
      next[tid] = ed::hyp_token(a, g, (int64_t)s0 + NT + tid);
    }
    const int s1 = s0 + NT < total ? s0 + NT : total;
    for (int st = s0 + 1; st <= s1; ++st) {
      for (int tid = 0; tid < NT; ++tid) last[tid] = lanes[tid].col[KS - 1];
      for (int tid = 0; tid < NT; ++tid) {
        uint64_t t = (tid & 63) ? last[tid - 1] : last[tid];           // a shift leaves the first lane of a wave its own value
        if (WAVES > 1 && (tid & 63) == 0 && tid) t = line[(st & 1) ^ 1][(tid >> 6) - 1];
        const int j = st - tid;
        if (tid == 0) t = ed::row0_cell(j);
        top[tid] = t;
      }
      for (int tid = 0; tid < NT; ++tid) {
        const int j = st - tid;
        if (ed::active(g, KS, tid, j)) ed::step<KS>(lanes[tid], top[tid], ring[(j - 1) & (RING - 1)]);
      }
      if (WAVES > 1)
        for (int tid = 63; tid < NT; tid += 64) line[st & 1][tid >> 6] = lanes[tid].col[KS - 1];
    }
  }
  for (int tid = 0; tid < NT; ++tid) ed::finish<KS>(a, g, tid, lanes[tid]);
}

extern "C" {

int sim_ed_states_per_lane(int64_t M) { int ks, nt; ed::config(M, ks, nt); return ks; }
int sim_ed_threads(int64_t M) { int ks, nt; ed::config(M, ks, nt); return nt; }
int sim_ed_max_ref() { return ed::kMaxRef; }
int sim_ed_max_hyp() { return ed::kMaxHyp; }

// dims: pairs, pairs per reference, N, M; flags: hyps, refs, hyp_len, ref_len are int64, return_ops
int sim_edit_distance(const void* hyps, const void* refs, const void* hyp_len, const void* ref_len, const int64_t* dims,
                      const int32_t* flags, int32_t* out) {
  ed::Args a{};
  a.hyps = hyps; a.refs = refs; a.hyp_len = hyp_len; a.ref_len = ref_len;
  a.pairs = dims[0]; a.per_ref = dims[1]; a.N = dims[2]; a.M = dims[3];
  if (a.M > ed::kMaxRef || a.N > ed::kMaxHyp) return -2;
  if (a.per_ref < 1 || a.pairs % a.per_ref) return -1;
  a.hyp64 = flags[0]; a.ref64 = flags[1]; a.hlen64 = flags[2]; a.rlen64 = flags[3]; a.ops = flags[4];
  a.out = out;
  int ks, nt;
  ed::config(a.M, ks, nt);
  for (int64_t p = 0; p < a.pairs; ++p) {
    if (nt == 64) pair_run<4, 64>(a, p);
    else if (ks == 4) pair_run<4, 256>(a, p);
    else pair_run<16, 256>(a, p);
  }
  return 0;
}

}  // extern "C"
