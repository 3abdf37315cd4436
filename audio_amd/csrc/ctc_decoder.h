// CTC prefix beam search without a language model (audio_amd.models.decoder: ctc_beam_search, cuda_ctc_decoder).
// log_probs (B, T, V) dense, lengths (B,) int32 / int64 read on the device.  Example b keeps a beam of at most K distinct
// prefixes, each with (pb, pnb), the log mass of its alignments that end in blank / not in blank; the beam starts as
// {(): (0, -inf)}.  A frame with lp[blank] > threshold is skipped entirely.  Every other frame, each prefix l with last token
// e and tot = logaddexp(pb, pnb) gives   l: pb' += tot + lp[blank];   l (not empty): pnb' += pnb + lp[e];
// l + c, c != blank: pnb' += (c == e ? pb : tot) + lp[c]   ("+=" is logaddexp; the same prefix merges), and the new beam is
// the K prefixes with the largest logaddexp(pb', pnb') that is neither -inf nor NaN.  float64 for every input type.
//
// For a fixed parent the score of l + c is monotone in lp[c] except for c == e, so the new beam lies inside
// (the beam) + (each parent x the frame's K + 1 largest non-blank tokens) + (each parent x its own last token): exact, and
// K (K + 2) extensions + K stays = K (K + 3) candidates instead of K V.  (K + 1 tokens because one of them may be e.  When e is
// not among them, pb + lp[e] <= tot + lp[e] <= tot + lp[c] for K + 1 other children of that parent, so l + e is among the K
// best only if rounding makes those sums bit-equal, where the smaller token ranks first: the own-token candidate is there
// for that tie, tests/ctc_decoder_oracle.py own_token_case.)
//
// row     One wave per live frame (b, t), the only full read of log_probs: 16-byte loads with the conversion in the load,
//         scalar head and tail.  Writes the frame's record: the skip flag, lp[blank], and the K + 1 largest non-blank
//         (value, token) pairs in rank order (ties to the smaller id; NaN ranks with -inf; a slot without a token holds -1).
//         Slot r is the best element after slot r - 1: every lane keeps the best of its own share, and only the lane that
//         owned the last winner looks through its share again.  A skipped frame reads lp[blank] only.
// beam    One workgroup of four waves per example.  The beam lives in LDS (nothing indexed at run time lives in registers),
//         in rank order.  The unskipped frames come from a ballot over 64 skip flags; a frame's record is loaded while the
//         frame before it is worked on.  Per frame: one gather lp[t][last token] per prefix (the repeat, the merge into an
//         entry whose parent is in the beam, and the own-token extension all need that one value); candidate p (K + 3) + s
//         (s = 0: p stays, 1 .. K + 1: a record slot, K + 2: p's own last token) belongs to lane (index mod 256).
//         Selection: every candidate counts the candidates that rank before it (score, then parent and token) in one
//         branch-free pass over LDS, and one of rank k < K writes entry k of the new beam -- no rounds, no dependent
//         chain (a lone wave pays the full LDS latency on every step of such a chain).  Prefixes are nodes (parent,
//         token) of a per-example trie in the workspace: a prefix that stays keeps its node, a selected extension appends
//         one -- at most K per unskipped frame, 1 + K T nodes per example.  Candidate (p, c) IS beam entry q when
//         parent[q] == node[p] and token[q] == c; a prefix that left the beam and came back has a second node, so the
//         entries also carry a 64-bit hash of their prefix and of its parent: entries whose hashes and lengths say
//         "child" but whose nodes differ are compared token by token along their parent pointers (rare, and exact).
//         Tail: the N best are the first N entries; each of N lanes walks its parent pointers and writes the tokens in
//         forward order.
//
// No index is formed from a floating value: tokens are the row pass's loop index, node ids a counter, and both are clamped
// where they index memory.  An example with a length outside [0, T] gets lengths -1 and scores NaN, and nothing is indexed
// with that length.  The phase functions are AAMD_HD: tests/cpu_sim/sim_ctc_decoder.cpp replays them with g++.
#pragma once
#include "hd.h"
#include "rnnt_loss.h"      // rnnt::split (head / 16-byte body / tail of a row), rnnt::logaddexp
#include "wave_augment.h"   // wa::Elem, wa::Vec

#if defined(__HIPCC__)
#define AAMD_UNROLL4 _Pragma("unroll 4")                  // short LDS loops of a run-time length: four reads in flight
#else
#define AAMD_UNROLL4
#endif

namespace aamd {
namespace cd {

constexpr int kMaxBeam = 32;
constexpr int kRowThreads = 256;                         // row pass: one wave per frame
constexpr int kBeamThreads = 256;                        // beam pass: one workgroup per example
constexpr int kMaxSlots = kMaxBeam + 1;                  // record slots of a frame
constexpr int kMaxCand = kMaxBeam * (kMaxBeam + 3);      // per parent: the stay, K + 1 record slots, its own last token
constexpr int kOwn = (kMaxCand + kBeamThreads - 1) / kBeamThreads;   // candidates of a lane
constexpr int64_t kMaxFrames = (int64_t)1 << 36;         // B * T: the workspace is counted in int64 bytes
constexpr int64_t kMaxNodes = ((int64_t)1 << 31) - 1;    // 1 + K * T: node ids of the trie are int32
constexpr int32_t kNoTok = 0x7fffffff;
constexpr uint64_t kRootHash = 0x243f6a8885a308d3ull;

AAMD_HD double neg_inf() { return -__builtin_inf(); }
AAMD_HD double nan64() { return __builtin_nan(""); }

struct Node {                        // a prefix: its parent's node and its last token
  int32_t parent, tok;
};

struct Args {
  const void* lp;                    // (B, T, V)
  const void* len;                   // (B,) int32 or int64
  int64_t B, T, V;
  int32_t blank, len64, K, N;
  int32_t R, R2;                     // record slots K + 1; candidates per parent K + 3
  double thr;
  int64_t pool;                      // trie nodes per example: 1 + K T
  // workspace
  Node* nodes;                       // (B, pool)
  double* rec_val;                   // (B, T, R)
  double* rec_lpb;                   // (B, T)
  int32_t* rec_tok;                  // (B, T, R)
  int32_t* rec_skip;                 // (B, T)
  // results
  int32_t* tokens;                   // (B, N, T)
  int32_t* out_len;                  // (B, N)
  double* scores;                    // (B, N)
};

AAMD_HD bool sizes_ok(int64_t B, int64_t T, int64_t K) {
  return B >= 0 && T >= 1 && K >= 1 && K <= kMaxBeam && B < ((int64_t)1 << 31) && T < ((int64_t)1 << 31) &&
         B * T <= kMaxFrames && 1 + K * T <= kMaxNodes;
}
AAMD_HD int64_t pad16(int64_t n) { return (n + 15) / 16 * 16; }
AAMD_HD int64_t ws_bytes(int64_t B, int64_t T, int64_t K) {
  const int64_t R = K + 1, f = B * T;
  return pad16(B * (1 + K * T) * 8) + pad16(f * R * 8 + f * 8) + pad16(f * R * 4) + pad16(f * 4);
}
AAMD_HD void ws_bind(Args& a, void* ws) {
  const int64_t f = a.B * a.T;
  a.R = a.K + 1;
  a.R2 = a.K + 3;
  a.pool = 1 + (int64_t)a.K * a.T;
  uint8_t* w = static_cast<uint8_t*>(ws);
  a.nodes = reinterpret_cast<Node*>(w); w += pad16(a.B * a.pool * 8);
  a.rec_val = reinterpret_cast<double*>(w);
  a.rec_lpb = a.rec_val + f * a.R; w += pad16(f * a.R * 8 + f * 8);
  a.rec_tok = reinterpret_cast<int32_t*>(w); w += pad16(f * a.R * 4);
  a.rec_skip = reinterpret_cast<int32_t*>(w);
}

AAMD_HD bool len_ok(const Args& a, int64_t b, int& Tb) {
  const int64_t tb = a.len64 ? static_cast<const int64_t*>(a.len)[b] : (int64_t) static_cast<const int32_t*>(a.len)[b];
  Tb = (int)tb;
  return tb >= 0 && tb <= a.T;
}

AAMD_HD int64_t node_clamp(const Args& a, int64_t nd) { return nd < 0 ? 0 : (nd >= a.pool ? a.pool - 1 : nd); }

// ---- row pass ------------------------------------------------------------------------------------------------------------------------
struct RowPick {
  double v;
  int32_t tok;
};
AAMD_HD RowPick row_none() { return {neg_inf(), kNoTok}; }
AAMD_HD bool row_before(RowPick x, RowPick y) { return x.v > y.v || (x.v == y.v && x.tok < y.tok); }

// element idx of the row: the best so far of those that rank after prev
AAMD_HD void row_see(const Args& a, int64_t idx, double v, bool first, RowPick prev, RowPick& best) {
  if (!(v == v)) v = neg_inf();
  const RowPick e{v, (int32_t)idx};
  if (idx != a.blank && (first || row_before(prev, e)) && row_before(e, best)) best = e;
}

// lane's share of row (b, t): the best non-blank element that ranks after prev (any, when first)
template <int DT>
AAMD_HD RowPick row_scan(const Args& a, int64_t row, int lane, bool first, RowPick prev) {
  using E = wa::Elem<DT>;
  using S = typename E::S;
  constexpr int VEC = 16 / (int)sizeof(S);
  const S* p = static_cast<const S*>(a.lp) + row * a.V;
  const rnnt::Split sp = rnnt::split(p, a.V, (int)sizeof(S));
  RowPick best = row_none();
  if (lane < sp.h) row_see(a, lane, (double)E::load(p[lane]), first, prev, best);
  const wa::Vec<S>* q = reinterpret_cast<const wa::Vec<S>*>(p + sp.h);
  for (int64_t i = lane; i < sp.nvec; i += 64) {
    const wa::Vec<S> v = q[i];
    AAMD_UNROLL
    for (int k = 0; k < VEC; ++k) row_see(a, sp.h + i * VEC + k, (double)E::load(v.e[k]), first, prev, best);
  }
  const int64_t t0 = sp.h + sp.nvec * VEC;
  if (lane < sp.tail) row_see(a, t0 + lane, (double)E::load(p[t0 + lane]), first, prev, best);
  return best;
}

// lp[blank] and the skip flag of a live row; the same in every lane, lane 0 stores
template <int DT>
AAMD_HD bool row_head(const Args& a, int64_t row, int lane) {
  using E = wa::Elem<DT>;
  const double lpb = (double)E::load(static_cast<const typename E::S*>(a.lp)[row * a.V + a.blank]);
  const bool skip = lpb > a.thr;
  if (lane == 0) {
    a.rec_lpb[row] = lpb;
    a.rec_skip[row] = skip ? 1 : 0;
  }
  return skip;
}
// slot r: every lane looks through its share for slot 0; afterwards only the lane that owned the last winner does, and nobody
// once the row has run out of tokens
AAMD_HD bool row_rescan(int r, RowPick mine, RowPick prev) { return r == 0 || (prev.tok != kNoTok && mine.tok == prev.tok); }
AAMD_HD void row_store(const Args& a, int64_t row, int r, RowPick g) {
  a.rec_val[row * a.R + r] = g.v;
  a.rec_tok[row * a.R + r] = g.tok == kNoTok ? -1 : g.tok;
}
AAMD_HD int64_t row_blocks(int64_t rows) {
  const int64_t n = (rows + kRowThreads / 64 - 1) / (kRowThreads / 64);
  return n < (1 << 20) ? n : (1 << 20);
}

#if defined(__HIPCC__)
template <int DT>
__global__ __launch_bounds__(kRowThreads) void row_kernel(Args a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t rows = a.B * a.T;
  for (int64_t r0 = (int64_t)blockIdx.x * (kRowThreads / 64); r0 < rows; r0 += (int64_t)gridDim.x * (kRowThreads / 64)) {
    const int64_t row = r0 + wave;                          // everything below is the same in every lane of the wave
    if (row >= rows) continue;
    int Tb;
    if (!len_ok(a, row / a.T, Tb) || row % a.T >= Tb) continue;
    if (row_head<DT>(a, row, lane)) continue;
    RowPick prev = row_none(), mine = row_none();
    for (int r = 0; r < a.R; ++r) {
      if (row_rescan(r, mine, prev)) mine = row_scan<DT>(a, row, lane, r == 0, prev);
      RowPick g = mine;
      AAMD_UNROLL
      for (int o = 32; o; o >>= 1) {
        const RowPick x{__shfl_xor(g.v, o), __shfl_xor(g.tok, o)};
        if (row_before(x, g)) g = x;
      }
      if (lane == 0) row_store(a, row, r, g);
      prev = g;
    }
  }
}
#endif

// ---- beam pass -----------------------------------------------------------------------------------------------------------------------
struct Shared {                      // [2]: the beam of this frame and the one being selected
  double pb[2][kMaxBeam], pnb[2][kMaxBeam], tot[2][kMaxBeam];
  int32_t node[2][kMaxBeam], par[2][kMaxBeam], last[2][kMaxBeam], len[2][kMaxBeam];
  uint64_t hash[2][kMaxBeam], phash[2][kMaxBeam];           // of the prefix and of its parent: what equal prefixes share
  int32_t n[2];
  int32_t ext[kMaxBeam];             // entry k of the new beam is an extension: it appends a node
  double glast[kMaxBeam];            // lp[t][last token] of every prefix
  double stay_pb[kMaxBeam], stay_pnb[kMaxBeam];
  double top_val[kMaxSlots];         // the frame's record
  int32_t top_tok[kMaxSlots];
  double lpb;
  double cand[kMaxCand];             // scores; -inf: not a candidate
  int64_t key[kMaxCand];             // parent << 32 | token + 1 (0: the stay): the order among equal scores
  int32_t out_len[kMaxBeam];
};

struct Rec {                         // lane r holds slot r
  double val, lpb;
  int32_t tok;
};
AAMD_HD Rec rec_load(const Args& a, int64_t b, int64_t t, int lane) {
  const int64_t row = b * a.T + t;
  Rec r;
  r.lpb = a.rec_lpb[row];
  r.val = lane < a.R ? a.rec_val[row * a.R + lane] : neg_inf();
  r.tok = lane < a.R ? a.rec_tok[row * a.R + lane] : -1;
  return r;
}
AAMD_HD void rec_publish(const Args& a, int lane, const Rec& r, Shared& S) {
  if (lane < a.R) {
    S.top_val[lane] = r.val;
    S.top_tok[lane] = r.tok >= 0 && r.tok < a.V ? r.tok : -1;
  }
  if (lane == 0) S.lpb = r.lpb;
}
AAMD_HD bool frame_live(const Args& a, int64_t b, int64_t t, int Tb) { return t < Tb && a.rec_skip[b * a.T + t] == 0; }

AAMD_HD void beam_init(const Args& a, int64_t b, int lane, Shared& S) {
  if (lane) return;
  S.pb[0][0] = 0.0; S.pnb[0][0] = neg_inf(); S.tot[0][0] = 0.0;
  S.node[0][0] = 0; S.par[0][0] = -1; S.last[0][0] = -1; S.len[0][0] = 0;
  S.n[0] = 1;
  a.nodes[b * a.pool] = Node{-1, -1};
  S.hash[0][0] = kRootHash; S.phash[0][0] = 0;
}

// lp[t][last token] of prefix `lane`
template <int DT>
AAMD_HD double gather(const Args& a, int64_t b, int64_t t, int lane, int cur, const Shared& S) {
  using E = wa::Elem<DT>;
  if (lane >= S.n[cur]) return neg_inf();
  const int32_t e = S.last[cur][lane];
  if (e < 0 || e >= a.V) return neg_inf();
  return (double)E::load(static_cast<const typename E::S*>(a.lp)[(b * a.T + t) * a.V + e]);
}
AAMD_HD void gather_publish(int lane, double g, Shared& S) {
  if (lane < kMaxBeam) S.glast[lane] = g;
}

AAMD_HD double kept(double score) { return score > neg_inf() ? score : neg_inf(); }      // NaN and -inf are never kept

// the hash of prefix + c from the prefix's (splitmix64's finisher)
AAMD_HD uint64_t hash_next(uint64_t h, int32_t c) {
  uint64_t z = h + 0x9e3779b97f4a7c15ull * (uint64_t)(uint32_t)(c + 1);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// Do nodes x and y spell one prefix of the same length?  A prefix that left the beam and came back has a second node; only
// then (the hashes agree, the nodes differ) is this walk taken.
AAMD_HD bool same_prefix(const Args& a, int64_t b, int64_t x, int64_t y) {
  const Node* nodes = a.nodes + b * a.pool;
  for (int64_t steps = 0; x != y && steps < a.pool; ++steps) {
    if (x < 0 || y < 0) return false;
    const Node nx = nodes[node_clamp(a, x)], ny = nodes[node_clamp(a, y)];
    if (nx.tok != ny.tok) return false;
    x = nx.parent;
    y = ny.parent;
  }
  return x == y;
}

// Is entry q the prefix of entry p plus token c?  The hashes and lengths sift (no branch: the LDS reads of the loops that call
// this stay in flight); sure: the nodes say so too.
AAMD_HD int child_maybe(const Shared& S, int cur, int q, int p, int32_t c) {
  return (int)(S.phash[cur][q] == S.hash[cur][p]) & (int)(S.last[cur][q] == c) & (int)(S.len[cur][q] == S.len[cur][p] + 1);
}
AAMD_HD int child_sure(const Shared& S, int cur, int q, int p) { return (int)(S.par[cur][q] == S.node[cur][p]); }

// is (p, c) an entry of the beam already?  Its mass went into that entry.
AAMD_HD bool in_beam(const Args& a, int64_t b, const Shared& S, int cur, int n, int p, int32_t c) {
  int hit = 0, maybe = 0;
  AAMD_UNROLL4
  for (int q = 0; q < n; ++q) {
    const int m = child_maybe(S, cur, q, p, c);
    hit |= m & child_sure(S, cur, q, p);
    maybe |= m;
  }
  if (!hit && maybe)
    for (int q = 0; q < n; ++q)
      if (child_maybe(S, cur, q, p, c) && same_prefix(a, b, S.par[cur][q], S.node[cur][p])) hit = 1;
  return hit != 0;
}
// the entry that is the parent of entry p, or -1
AAMD_HD int parent_in_beam(const Args& a, int64_t b, const Shared& S, int cur, int n, int p) {
  const int32_t e = S.last[cur][p];
  int from = -1, maybe = 0;
  AAMD_UNROLL4
  for (int q = 0; q < n; ++q) {
    const int m = child_maybe(S, cur, p, q, e);
    from = m & child_sure(S, cur, p, q) ? q : from;
    maybe |= m;
  }
  if (from < 0 && maybe)
    for (int q = 0; q < n; ++q)
      if (child_maybe(S, cur, p, q, e) && same_prefix(a, b, S.par[cur][p], S.node[cur][q])) from = q;
  return from;
}

// the token of candidate slot s of parent p: -1 for the stay
AAMD_HD int32_t cand_tok(const Args& a, const Shared& S, int cur, int p, int s) {
  return s == 0 ? -1 : (s <= a.R ? S.top_tok[s - 1] : S.last[cur][p]);
}

// the lane's candidates: own == false the record slots, own == true the stay and the parent's own last token
AAMD_HD void fill(const Args& a, int64_t b, int lane, int cur, bool own, Shared& S) {
  const int n = S.n[cur];
  for (int i = lane; i < n * a.R2; i += kBeamThreads) {
    const int p = i / a.R2, s = i % a.R2;
    if (own != (s == 0 || s == a.R2 - 1)) continue;
    const int32_t e = S.last[cur][p];
    if (s == 0) {
      const double g = S.glast[p];
      const double pb = S.tot[cur][p] + S.lpb;
      double pnb = e >= 0 ? S.pnb[cur][p] + g : neg_inf();
      const int from = parent_in_beam(a, b, S, cur, n, p);   // the parent, when the beam holds it, extends into this entry
      if (from >= 0) pnb = rnnt::logaddexp(pnb, (S.last[cur][from] == e ? S.pb[cur][from] : S.tot[cur][from]) + g);
      S.stay_pb[p] = pb;
      S.stay_pnb[p] = pnb;
      S.cand[i] = kept(rnnt::logaddexp(pb, pnb));
      S.key[i] = (int64_t)p << 32;
      continue;
    }
    const int32_t c = cand_tok(a, S, cur, p, s);
    bool ok = c >= 0;
    double v;
    if (s <= a.R) {
      v = S.top_val[s - 1];
    } else {                                                 // the record's slots serve it when it is among them
      v = S.glast[p];
      int other = 1;
      AAMD_UNROLL4
      for (int r = 0; r < a.R; ++r) other &= (int)(S.top_tok[r] != c);
      ok = ok && other;
    }
    ok = ok && !in_beam(a, b, S, cur, n, p, c);
    S.cand[i] = ok ? kept((c == e ? S.pb[cur][p] : S.tot[cur][p]) + v) : neg_inf();
    S.key[i] = ((int64_t)p << 32) | (int64_t)(c + 1);
  }
}

// candidate idx, of rank k among all candidates, becomes entry k of the new beam; an extension's node is found afterwards
AAMD_HD void take(const Args& a, int cur, int idx, double score, int k, Shared& S) {
  const int nw = cur ^ 1, p = idx / a.R2, s = idx % a.R2;
  S.tot[nw][k] = score;
  if (s == 0) {
    S.pb[nw][k] = S.stay_pb[p]; S.pnb[nw][k] = S.stay_pnb[p];
    S.node[nw][k] = S.node[cur][p]; S.par[nw][k] = S.par[cur][p]; S.last[nw][k] = S.last[cur][p]; S.len[nw][k] = S.len[cur][p];
    S.hash[nw][k] = S.hash[cur][p]; S.phash[nw][k] = S.phash[cur][p];
    S.ext[k] = 0;
  } else {
    const int32_t c = cand_tok(a, S, cur, p, s);
    S.pb[nw][k] = neg_inf(); S.pnb[nw][k] = score;
    S.node[nw][k] = -1; S.par[nw][k] = S.node[cur][p]; S.last[nw][k] = c; S.len[nw][k] = S.len[cur][p] + 1;
    S.hash[nw][k] = hash_next(S.hash[cur][p], c); S.phash[nw][k] = S.hash[cur][p];
    S.ext[k] = 1;
  }
}

AAMD_HD void lds_max(int32_t* p, int32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMax(p, v);
#else
  *p = v > *p ? v : *p;
#endif
}

// The lane's candidates (OWN of them, in registers under compile-time indices) count the candidates that rank before them
// (score, then key: a strict order; the keys are read only where scores are bit-equal): one pass over the candidates, every
// lane reading the same LDS words, eight at a time so that the reads are in flight together, no dependent chain.  One of
// rank k < K is entry k of the new beam; n of the new beam is 1 + the largest rank taken.
template <int OWN>
AAMD_HD void select_own(const Args& a, int lane, int cur, Shared& S) {
  constexpr int STEP = 8;
  const int nc = S.n[cur] * a.R2;
  double mine[OWN];
  int rank[OWN], same[OWN];                                 // candidates with a larger score; with the same score (itself too)
  AAMD_UNROLL
  for (int c = 0; c < OWN; ++c) {
    const int i = lane + c * kBeamThreads;
    mine[c] = i < nc ? S.cand[i] : neg_inf();
    rank[c] = same[c] = 0;
  }
  for (int j0 = 0; j0 < nc; j0 += STEP) {
    double sc[STEP];
    AAMD_UNROLL
    for (int u = 0; u < STEP; ++u) sc[u] = j0 + u < nc ? S.cand[j0 + u] : neg_inf();     // kMaxCand is a multiple of STEP
    AAMD_UNROLL
    for (int u = 0; u < STEP; ++u) {
      AAMD_UNROLL
      for (int c = 0; c < OWN; ++c) {
        rank[c] += (int)(sc[u] > mine[c]);
        same[c] += (int)(sc[u] == mine[c]);
      }
    }
  }
  AAMD_UNROLL
  for (int c = 0; c < OWN; ++c) {
    if (mine[c] > neg_inf() && same[c] > 1 && rank[c] < a.K) {                           // an exact tie: the keys order it
      const int64_t key = S.key[lane + c * kBeamThreads];
      for (int j = 0; j < nc; ++j) rank[c] += (int)(S.cand[j] == mine[c]) & (int)(S.key[j] < key);
    }
    if (mine[c] > neg_inf() && rank[c] < a.K) {
      take(a, cur, lane + c * kBeamThreads, mine[c], rank[c], S);
      lds_max(&S.n[cur ^ 1], rank[c] + 1);
    }
  }
}
AAMD_HD void select(const Args& a, int lane, int cur, Shared& S) {
  static_assert(kOwn == 5 && kMaxCand % 8 == 0, "select() lists the instantiations");
  const int own = (S.n[cur] * a.R2 + kBeamThreads - 1) / kBeamThreads;         // the same in every lane
  if (own <= 1) select_own<1>(a, lane, cur, S);
  else if (own == 2) select_own<2>(a, lane, cur, S);
  else if (own == 3) select_own<3>(a, lane, cur, S);
  else if (own == 4) select_own<4>(a, lane, cur, S);
  else select_own<5>(a, lane, cur, S);
}

AAMD_HD void frame_begin(int lane, int cur, Shared& S) {
  if (lane == 0) S.n[cur ^ 1] = 0;
}
// The extensions among the entries of the new beam append the nodes count, count + 1, ... in the order of their ranks (at most K
// per unskipped frame, so the pool of 1 + K T holds them).  Returns how many: the same in every lane.
AAMD_HD int32_t append_nodes(const Args& a, int64_t b, int lane, int nw, int32_t count, Shared& S) {
  const int n = S.n[nw];
  int32_t before = 0, all = 0;
  AAMD_UNROLL4
  for (int k = 0; k < n; ++k) {
    before += k < lane ? S.ext[k] : 0;
    all += S.ext[k];
  }
  if (lane < n && S.ext[lane]) {
    const int32_t id = count + before;
    S.node[nw][lane] = id;
    if (id >= 0 && id < a.pool) a.nodes[b * a.pool + id] = Node{S.par[nw][lane], S.last[nw][lane]};
  }
  return all;
}

// lane h < N: hypothesis h (the beam is in rank order)
AAMD_HD void finish(const Args& a, int64_t b, int lane, int cur, Shared& S) {
  if (lane >= a.N) return;
  const int64_t o = b * a.N + lane;
  int32_t L = -1;
  double score = neg_inf();
  if (lane < S.n[cur]) {
    L = S.len[cur][lane];
    L = L < 0 ? 0 : (L > a.T ? (int32_t)a.T : L);
    score = S.tot[cur][lane];
    int64_t nd = S.node[cur][lane];
    for (int32_t d = L - 1; d >= 0; --d) {
      nd = node_clamp(a, nd);                               // no value of the workspace takes the walk out of the pool
      const Node x = a.nodes[b * a.pool + nd];
      a.tokens[o * a.T + d] = x.tok;
      nd = x.parent;
    }
  }
  a.out_len[o] = L;
  a.scores[o] = score;
  S.out_len[lane] = L < 0 ? 0 : L;
}
// all lanes: zeros beyond each length
AAMD_HD void zero_fill(const Args& a, int64_t b, int lane, const Shared& S) {
  for (int h = 0; h < a.N; ++h)
    for (int64_t t = (int64_t)S.out_len[h] + lane; t < a.T; t += kBeamThreads) a.tokens[(b * a.N + h) * a.T + t] = 0;
}
// a flagged example: -1 / NaN / zeros
AAMD_HD void flagged(const Args& a, int64_t b, int lane) {
  if (lane < a.N) {
    a.out_len[b * a.N + lane] = -1;
    a.scores[b * a.N + lane] = nan64();
  }
  for (int64_t e = lane; e < (int64_t)a.N * a.T; e += kBeamThreads) a.tokens[b * a.N * a.T + e] = 0;
}

#if defined(__HIPCC__)
template <int DT>
__global__ __launch_bounds__(kBeamThreads) void beam_kernel(Args a) {
  __shared__ Shared S;
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  int Tb;
  if (!len_ok(a, b, Tb)) {                                  // the same in every lane
    flagged(a, b, lane);
    return;
  }
  beam_init(a, b, lane, S);
  int cur = 0;
  int32_t count = 1;                                        // nodes of the trie; the same in every lane
  __syncthreads();
  for (int64_t t0 = 0; t0 < Tb; t0 += 64) {
    unsigned long long mask = __ballot(frame_live(a, b, t0 + (lane & 63), Tb));      // the same in every wave
    Rec rec{};
    if (mask) rec = rec_load(a, b, t0 + __builtin_ctzll(mask), lane);
    while (mask) {                                          // every lane meets every barrier: mask is the workgroup's
      const int64_t t = t0 + __builtin_ctzll(mask);
      mask &= mask - 1;
      rec_publish(a, lane, rec, S);
      frame_begin(lane, cur, S);
      if (mask) rec = rec_load(a, b, t0 + __builtin_ctzll(mask), lane);
      const double g = gather<DT>(a, b, t, lane, cur, S);
      __syncthreads();
      fill(a, b, lane, cur, false, S);
      gather_publish(lane, g, S);
      __syncthreads();
      fill(a, b, lane, cur, true, S);
      __syncthreads();
      select(a, lane, cur, S);
      __syncthreads();
      cur ^= 1;
      count += append_nodes(a, b, lane, cur, count, S);
      __syncthreads();
    }
  }
  finish(a, b, lane, cur, S);
  __syncthreads();
  zero_fill(a, b, lane, S);
}
#endif

}  // namespace cd
}  // namespace aamd
