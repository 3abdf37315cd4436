// CTC prefix beam search of the C ABI (csrc/ctc_decoder.h): exported constants, workspace query, row pass + beam pass.
#include "api_common.h"
#include "ctc_decoder.h"

using namespace aamd;

namespace {

template <int DT>
int search_launch(const cd::Args& a, hipStream_t s) {
  const int rc = launch(cd::row_kernel<DT>, cd::row_blocks(a.B * a.T), cd::kRowThreads, 0, s, a);
  if (rc != AAMD_OK) return rc;
  return launch(cd::beam_kernel<DT>, a.B, cd::kBeamThreads, 0, s, a);
}

}  // namespace

extern "C" {

int32_t aamd_ctc_decoder_max_beam(void) { return cd::kMaxBeam; }
int32_t aamd_ctc_decoder_row_threads(void) { return cd::kRowThreads; }
int32_t aamd_ctc_decoder_beam_threads(void) { return cd::kBeamThreads; }
int32_t aamd_ctc_decoder_record_slots(int32_t beam) { return beam + 1; }
int32_t aamd_ctc_decoder_candidates(int32_t beam) { return beam * (beam + 3); }
int64_t aamd_ctc_decoder_max_frames(void) { return cd::kMaxFrames; }
int64_t aamd_ctc_decoder_max_nodes(void) { return cd::kMaxNodes; }

int64_t aamd_ctc_decoder_workspace(int64_t batch, int64_t max_t, int64_t vocab, int64_t beam) {
  if (vocab < 2 || !cd::sizes_ok(batch, max_t, beam)) return 0;
  return cd::ws_bytes(batch, max_t, beam);
}

int aamd_ctc_beam_search(int32_t dtype, const void* log_probs, const void* lengths, int32_t lengths_int64, int64_t batch,
                         int64_t max_t, int64_t vocab, int32_t blank, int32_t beam, int32_t nbest, double threshold,
                         void* workspace, int32_t* tokens, int32_t* token_lengths, double* scores, void* stream) {
  DeviceScope dev_scope_(log_probs);
  static_assert(cd::kMaxBeam == AAMD_CTC_DECODER_MAX_BEAM, "the header's limit is the beam kernel's");
  AAMD_CHECK_ARG(dtype >= AAMD_SA_F32 && dtype <= AAMD_SA_BF16, "ctc_beam_search: unknown element type");
  AAMD_CHECK_ARG(batch >= 0 && max_t >= 1 && vocab >= 2, "ctc_beam_search: bad sizes (vocab >= 2, max_t >= 1)");
  AAMD_CHECK_ARG(beam >= 1 && nbest >= 1 && nbest <= beam, "ctc_beam_search: 1 <= nbest <= beam");
  if (beam > AAMD_CTC_DECODER_MAX_BEAM)
    return fail(AAMD_EUNSUPPORTED, "audio_amd: ctc_beam_search: the beam kernel serves beam_size <= 32");
  if (max_t >= (1ll << 31) || vocab >= (1ll << 31) || batch >= (1ll << 31))
    return fail(AAMD_EUNSUPPORTED, "audio_amd: ctc_beam_search: batch, max_t and vocab must be below 2^31");
  if (!cd::sizes_ok(batch, max_t, beam))
    return fail(AAMD_EUNSUPPORTED, "audio_amd: ctc_beam_search: batch * max_t <= 2^36 and beam * max_t < 2^31 - 1 "
                                   "(node ids of the prefix trie are 32-bit)");
  AAMD_CHECK_ARG(blank >= 0 && blank < vocab, "ctc_beam_search: blank must lie in [0, vocab)");
  if (batch == 0) return AAMD_OK;
  AAMD_CHECK_ARG(log_probs && lengths && workspace && tokens && token_lengths && scores, "null buffer");
  const int es = dtype == AAMD_SA_F64 ? 8 : (dtype == AAMD_SA_F32 ? 4 : 2);
  AAMD_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "ctc_beam_search: workspace must be 16-byte aligned");
  AAMD_CHECK_ARG(((uintptr_t)log_probs & (uintptr_t)(es - 1)) == 0, "ctc_beam_search: log_probs is not aligned to its element");
  cd::Args a{};
  a.lp = log_probs; a.len = lengths;
  a.B = batch; a.T = max_t; a.V = vocab;
  a.blank = blank; a.len64 = lengths_int64 ? 1 : 0; a.K = beam; a.N = nbest; a.thr = threshold;
  a.tokens = tokens; a.out_len = token_lengths; a.scores = scores;
  cd::ws_bind(a, workspace);
  hipStream_t s = (hipStream_t)stream;
  switch (dtype) {
    case AAMD_SA_F32: return search_launch<wa::kF32>(a, s);
    case AAMD_SA_F64: return search_launch<wa::kF64>(a, s);
    case AAMD_SA_F16: return search_launch<wa::kF16>(a, s);
    default: return search_launch<wa::kBF16>(a, s);
  }
}

}  // extern "C"
