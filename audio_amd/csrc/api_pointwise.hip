// Pointwise waveform ops of the C ABI (csrc/wave_pointwise.h): exported constants and the one entry point of the family.
#include "api_common.h"
#include "wave_pointwise.h"

using namespace aamd;

namespace {

int elem_size(int32_t dtype) {
  switch (dtype) {
    case AAMD_SA_F64: case AAMD_PW_I64: return 8;
    case AAMD_SA_F32: case AAMD_PW_I32: return 4;
    case AAMD_SA_F16: case AAMD_SA_BF16: case AAMD_PW_I16: return 2;
    default: return 1;
  }
}

template <int OP, int DIN, int DOUT>
int run(const pw::Args& a, hipStream_t s) {
  return launch(pw::pointwise_kernel<OP, DIN, DOUT>, a.rows * a.chunks, pw::kThreads, 0, s, a);
}

// the four floating types, result in the input's type
template <int OP>
int run_float(int32_t dtype, const pw::Args& a, hipStream_t s) {
  switch (dtype) {
    case AAMD_SA_F32: return run<OP, wa::kF32, wa::kF32>(a, s);
    case AAMD_SA_F64: return run<OP, wa::kF64, wa::kF64>(a, s);
    case AAMD_SA_F16: return run<OP, wa::kF16, wa::kF16>(a, s);
    default: return run<OP, wa::kBF16, wa::kBF16>(a, s);
  }
}

}  // namespace

extern "C" {

int32_t aamd_pointwise_tiles(int32_t which) {
  static_assert(pw::kScale == AAMD_PW_SCALE && pw::kContrast == AAMD_PW_CONTRAST && pw::kDbToAmp == AAMD_PW_DB_TO_AMPLITUDE &&
                    pw::kMuEncode == AAMD_PW_MU_ENCODE && pw::kMuDecode == AAMD_PW_MU_DECODE && pw::kFade == AAMD_PW_FADE,
                "the header's op codes are the kernels'");
  static_assert(pw::kI64 == AAMD_PW_I64 && pw::kI32 == AAMD_PW_I32 && pw::kI16 == AAMD_PW_I16 && pw::kI8 == AAMD_PW_I8 &&
                    pw::kU8 == AAMD_PW_U8, "the header's element codes are the kernels'");
  return which == 0 ? pw::kThreads : (which == 1 ? pw::kChunk : (which == 2 ? pw::kBatch : 0));
}

int aamd_pointwise(int32_t op, int32_t dtype, const void* x, void* out, int64_t rows, int64_t length, int64_t row_stride,
                   double p0, double p1, int32_t flag, const void* table, int64_t n_in, int64_t n_out, void* stream) {
  DeviceScope dev_scope_(x);
  AAMD_CHECK_ARG(op >= 0 && op < pw::kOps, "pointwise: unknown op");
  AAMD_CHECK_ARG(dtype >= AAMD_SA_F32 && dtype < pw::kTypes, "pointwise: unknown element type");
  AAMD_CHECK_ARG(dtype <= AAMD_SA_BF16 || op == AAMD_PW_MU_DECODE, "pointwise: integer input is served by mu_decode only");
  AAMD_CHECK_ARG(rows >= 0 && length >= 0 && row_stride >= 0, "pointwise: bad sizes");
  AAMD_CHECK_ARG(rows < (1ll << 31) && length < (1ll << 40), "pointwise: too many rows or samples");
  if (op == AAMD_PW_FADE)
    AAMD_CHECK_ARG(n_in >= 0 && n_out >= 0 && n_in <= length && n_out <= length, "pointwise: a fade is longer than the signal");
  if (rows == 0 || length == 0) return AAMD_OK;
  AAMD_CHECK_ARG(x && out, "null buffer");
  const int out_size = op == AAMD_PW_MU_ENCODE ? 8 : (dtype > AAMD_SA_BF16 ? 4 : elem_size(dtype));
  AAMD_CHECK_ARG(((uintptr_t)x & (uintptr_t)(elem_size(dtype) - 1)) == 0 && ((uintptr_t)out & (uintptr_t)(out_size - 1)) == 0,
                 "pointwise: a buffer is not aligned to its element");
  pw::Args a{};
  a.x = x; a.out = out; a.rows = rows; a.L = length; a.sx = rows > 1 ? row_stride : 0; a.chunks = pw::n_chunks(length);
  a.p0 = p0; a.p1 = p1; a.flag = flag;
  AAMD_CHECK_ARG(rows * a.chunks < (1ll << 31), "pointwise: too many workgroups");
  hipStream_t s = (hipStream_t)stream;
  switch (op) {
    case AAMD_PW_SCALE: return run_float<pw::kScale>(dtype, a, s);
    case AAMD_PW_CONTRAST: return run_float<pw::kContrast>(dtype, a, s);
    case AAMD_PW_DB_TO_AMPLITUDE: return run_float<pw::kDbToAmp>(dtype, a, s);
    case AAMD_PW_MU_ENCODE:
      AAMD_CHECK_ARG(p0 >= 1.0, "pointwise: mu-law needs at least two quantization channels");
      return run_float<pw::kMuEncode>(dtype, a, s);
    case AAMD_PW_MU_DECODE:
      AAMD_CHECK_ARG(p0 >= 1.0, "pointwise: mu-law needs at least two quantization channels");
      switch (dtype) {
        case AAMD_PW_I64: return run<pw::kMuDecode, pw::kI64, wa::kF32>(a, s);
        case AAMD_PW_I32: return run<pw::kMuDecode, pw::kI32, wa::kF32>(a, s);
        case AAMD_PW_I16: return run<pw::kMuDecode, pw::kI16, wa::kF32>(a, s);
        case AAMD_PW_I8: return run<pw::kMuDecode, pw::kI8, wa::kF32>(a, s);
        case AAMD_PW_U8: return run<pw::kMuDecode, pw::kU8, wa::kF32>(a, s);
        default: return run_float<pw::kMuDecode>(dtype, a, s);
      }
    default:
      a.n_in = n_in; a.n_out = n_out; a.table = table;
      AAMD_CHECK_ARG(n_in + n_out == 0 || (table && ((uintptr_t)table & (uintptr_t)(elem_size(dtype) - 1)) == 0),
                     "pointwise: the fade table is missing or misaligned");
      return run_float<pw::kFade>(dtype, a, s);
  }
}

}  // extern "C"
