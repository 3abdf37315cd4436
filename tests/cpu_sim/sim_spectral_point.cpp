// CPU replay of the spectral-centroid and pointwise kernels (audio_amd/csrc/spectral_feat.h and wave_pointwise.h compiled
// with g++, no GPU): each driver mirrors its __global__ kernel -- the loop over workgroups and thread ids, the wave's
// shuffle tree as the same additions on an array -- with the launch geometry and the argument checks of the C ABI.
// TEST INFRASTRUCTURE ONLY.
#include <cstdint>
#include <vector>

#include "../../audio_amd/csrc/spectral_feat.h"
#include "../../audio_amd/csrc/wave_pointwise.h"

using namespace aamd;

template <int DT>
static void centroid(const sf::CentArgs& a, bool lines) {               // centroid_kernel<DT, LINES>
  const int64_t items = a.rows * a.frames;
  if (!lines) {
    for (int64_t q = 0; q < (items + sf::kThreads - 1) / sf::kThreads * sf::kThreads; ++q) {
      double num, den;
      sf::frame_strided(a, q, num, den);
      if (q < items) sf::store_result<DT>(a, q, num, den);
    }
    return;
  }
  const int P = a.lanes, per_block = sf::kThreads / P;
  std::vector<double> num(P), den(P);
  for (int64_t blk = 0; blk < (items + per_block - 1) / per_block; ++blk)
    for (int g = 0; g < per_block; ++g) {
      const int64_t q = blk * per_block + g;
      for (int lane = 0; lane < P; ++lane) sf::lane_partial(a, q, lane, num[lane], den[lane]);
      for (int s = P >> 1; s > 0; s >>= 1)
        for (int lane = 0; lane < P; ++lane) sf::tree_step(num.data(), den.data(), lane, s);
      if (q < items) sf::store_result<DT>(a, q, num[0], den[0]);
    }
}

template <int OP, int DIN, int DOUT>
static int pointwise(const pw::Args& a) {                               // pointwise_kernel<OP, DIN, DOUT>
  for (int64_t blk = 0; blk < a.rows * a.chunks; ++blk) {
    const int64_t row = blk / a.chunks, chunk = blk - row * a.chunks;
    for (int tid = 0; tid < pw::kThreads; ++tid) pw::chunk_thread<OP, DIN, DOUT>(tid, a, row, chunk);
  }
  return 0;
}

template <int OP>
static int pointwise_float(int dtype, const pw::Args& a) {
  switch (dtype) {
    case wa::kF32: return pointwise<OP, wa::kF32, wa::kF32>(a);
    case wa::kF64: return pointwise<OP, wa::kF64, wa::kF64>(a);
    case wa::kF16: return pointwise<OP, wa::kF16, wa::kF16>(a);
    case wa::kBF16: return pointwise<OP, wa::kBF16, wa::kBF16>(a);
    default: return -1;
  }
}

extern "C" {

int sim_spectral_tiles(int which) { return which == 0 ? sf::kThreads : (which == 1 ? sf::kVec : (which == 2 ? sf::kMaxLanes : 0)); }
int sim_spectral_lanes(int64_t n_freq) { return n_freq < 1 ? 0 : sf::lanes_for(n_freq); }
int sim_pointwise_tiles(int which) { return which == 0 ? pw::kThreads : (which == 1 ? pw::kChunk : (which == 2 ? pw::kBatch : 0)); }

// the arguments of aamd_spectral_centroid without the stream; < 0 on a bad argument
int sim_spectral_centroid(int out_dtype, const float* mag, const float* freqs, void* out, int64_t rows, int64_t frames,
                          int64_t n_freq, int64_t sr, int64_t st, int64_t sk) {
  if (rows < 0 || frames < 0 || n_freq < 1 || sr < 0 || st < 0 || sk < 0) return -2;
  if (rows == 0 || frames == 0) return 0;
  if (((uintptr_t)freqs & 15) || ((uintptr_t)mag & 3)) return -3;
  sf::CentArgs a{};
  a.m = mag; a.freqs = freqs; a.out = out; a.rows = rows; a.frames = frames; a.n_freq = n_freq; a.sr = sr; a.st = st; a.sk = sk;
  const bool lines = sk == 1 || n_freq == 1;
  a.lanes = lines ? sf::lanes_for(n_freq) : 1;
  switch (out_dtype) {
    case wa::kF32: centroid<wa::kF32>(a, lines); break;
    case wa::kF16: centroid<wa::kF16>(a, lines); break;
    case wa::kBF16: centroid<wa::kBF16>(a, lines); break;
    default: return -1;
  }
  return 0;
}

// the arguments of aamd_pointwise without the stream; < 0 on a bad argument
int sim_pointwise(int op, int dtype, const void* x, void* out, int64_t rows, int64_t L, int64_t sx, double p0, double p1,
                  int flag, const void* table, int64_t n_in, int64_t n_out) {
  if (op < 0 || op >= pw::kOps || dtype < 0 || dtype >= pw::kTypes || rows < 0 || L < 0 || sx < 0) return -2;
  if (dtype > wa::kBF16 && op != pw::kMuDecode) return -2;
  if (op == pw::kFade && (n_in < 0 || n_out < 0 || n_in > L || n_out > L)) return -2;
  if (rows == 0 || L == 0) return 0;
  pw::Args a{};
  a.x = x; a.out = out; a.rows = rows; a.L = L; a.sx = rows > 1 ? sx : 0; a.chunks = pw::n_chunks(L);
  a.p0 = p0; a.p1 = p1; a.flag = flag;
  switch (op) {
    case pw::kScale: return pointwise_float<pw::kScale>(dtype, a);
    case pw::kContrast: return pointwise_float<pw::kContrast>(dtype, a);
    case pw::kDbToAmp: return pointwise_float<pw::kDbToAmp>(dtype, a);
    case pw::kMuEncode: return pointwise_float<pw::kMuEncode>(dtype, a);
    case pw::kMuDecode:
      switch (dtype) {
        case pw::kI64: return pointwise<pw::kMuDecode, pw::kI64, wa::kF32>(a);
        case pw::kI32: return pointwise<pw::kMuDecode, pw::kI32, wa::kF32>(a);
        case pw::kI16: return pointwise<pw::kMuDecode, pw::kI16, wa::kF32>(a);
        case pw::kI8: return pointwise<pw::kMuDecode, pw::kI8, wa::kF32>(a);
        case pw::kU8: return pointwise<pw::kMuDecode, pw::kU8, wa::kF32>(a);
        default: return pointwise_float<pw::kMuDecode>(dtype, a);
      }
    default:
      a.n_in = n_in; a.n_out = n_out; a.table = table;
      return pointwise_float<pw::kFade>(dtype, a);
  }
}

}  // extern "C"
