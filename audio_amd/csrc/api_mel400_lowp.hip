// n_fft = 400 mel entry points that read the waveform as it is stored: int16 PCM (mono, interleaved stereo), half, bfloat16.
// Owns the melspec400_kernel instantiations with a non-float input type.
#include "api_common.h"
#include "mel400_launch.h"

using namespace aamd;

namespace {

// what the mono and the stereo PCM entry share once their arguments are checked: mel rows, or (mean given) the RNN-T features
template <typename TIn>
int launch_pcm(const StftGeom& g, const MelBandsDev& mb, const TIn* wav, const float* window, const float* twiddle, float* out,
               float gain, const float* mean, const float* invstddev, int64_t out_frames, hipStream_t s) {
  if (!mel400_eligible(g, mb) || (g.hop != 160 && g.hop != 200))
    return fail(AAMD_EUNSUPPORTED, "audio_amd: int16 PCM input is served by the n_fft = 400, hop 160 / 200 kernel only");
  if (mean == nullptr) return launch_fft400<m400::EPI400_MEL>(g, mb, wav, window, twiddle, out, m400::Epi400{}, s);
  AAMD_CHECK_ARG(out_frames >= g.n_frames, "out_frames must be >= n_frames");
  m400::Epi400 epi{};
  epi.gain = gain; epi.mean = mean; epi.invstd = invstddev; epi.out_frames = out_frames;
  return launch_fft400<m400::EPI400_MEL_NORM>(g, mb, wav, window, twiddle, out, epi, s);
}

}  // namespace

extern "C" {

int aamd_melspectrogram_pcm16_f32(const int16_t* wav, const float* window, const float* twiddle,
                                  const aamd_mel_bands* bands, float* out, const aamd_stft_desc* desc, float gain,
                                  const float* mean, const float* invstddev, int64_t out_frames, void* stream) {
  DeviceScope dev_scope_(wav);
  StftGeom g;
  MelBandsDev mb;
  int rc = mel_prologue(desc, bands, wav && window && twiddle && out, true, g, mb,
                        [&] { return (mean == nullptr) == (invstddev == nullptr) ? nullptr : "mean and invstddev come together"; });
  if (rc != AAMD_OK) return rc;
  return launch_pcm(g, mb, wav, window, twiddle, out, gain, mean, invstddev, out_frames, (hipStream_t)stream);
}

// Reduced-precision waveforms (the reference takes any floating dtype, functional/functional.py:1413-1414 and every
// transform's forward; a half / bfloat16 pipeline hands such tensors over): read as they are, converted to float in the gather
// of the radix-20x20 kernel -- half the input bytes, no separate cast pass.  Arithmetic and output stay float32 (the host
// casts the result to the input dtype, which is what the reference returns).  n_fft = 400, hop 160 / 200 only; every other
// shape takes the host's cast + the float kernels.
int aamd_melspectrogram_lowp_f32(const void* wav, int32_t wav_dtype, const float* window, const float* twiddle,
                                 const aamd_mel_bands* bands, float* out, const aamd_stft_desc* desc, void* stream) {
  DeviceScope dev_scope_(wav);
  StftGeom g;
  MelBandsDev mb;
  int rc = mel_prologue(desc, bands, wav && window && twiddle && out, true, g, mb, [&] {
    return wav_dtype == AAMD_DTYPE_F16 || wav_dtype == AAMD_DTYPE_BF16 ? nullptr : "wav_dtype: AAMD_DTYPE_F16 or AAMD_DTYPE_BF16";
  });
  if (rc != AAMD_OK) return rc;
  if (!mel400_eligible(g, mb) || (g.hop != 160 && g.hop != 200))
    return fail(AAMD_EUNSUPPORTED, "audio_amd: half / bfloat16 input is read directly by the n_fft = 400, hop 160 / 200 kernel only");
  hipStream_t s = (hipStream_t)stream;
  const m400::Epi400 epi{};
  if (wav_dtype == AAMD_DTYPE_F16)
    return launch_fft400<m400::EPI400_MEL>(g, mb, static_cast<const _Float16*>(wav), window, twiddle, out, epi, s);
  return launch_fft400<m400::EPI400_MEL>(g, mb, static_cast<const __bf16*>(wav), window, twiddle, out, epi, s);
}

int aamd_melspectrogram_pcm16_interleaved_f32(const int16_t* pcm, int32_t channels, const float* window, const float* twiddle,
                                              const aamd_mel_bands* bands, float* out, const aamd_stft_desc* desc,
                                              float gain, const float* mean, const float* invstddev, int64_t out_frames,
                                              void* stream) {
  if (channels == 1)
    return aamd_melspectrogram_pcm16_f32(pcm, window, twiddle, bands, out, desc, gain, mean, invstddev, out_frames, stream);
  if (channels != 2)
    return fail(AAMD_EUNSUPPORTED, "audio_amd: interleaved PCM is read directly for 1 or 2 channels only (transpose first)");
  DeviceScope dev_scope_(pcm);
  StftGeom g;
  MelBandsDev mb;
  int rc = mel_prologue(desc, bands, pcm && window && twiddle && out, true, g, mb, [&] {
    if (g.rows % 2 != 0) return "rows must be clips * channels";
    return (mean == nullptr) == (invstddev == nullptr) ? nullptr : "mean and invstddev come together";
  }, [&] { return reinterpret_cast<uintptr_t>(pcm) % 4 == 0 ? nullptr : "interleaved stereo PCM must be 4-byte aligned"; });
  if (rc != AAMD_OK) return rc;
  const m400::PcmStereo* w2 = reinterpret_cast<const m400::PcmStereo*>(pcm);      // one (L, R) word per sample time
  return launch_pcm(g, mb, w2, window, twiddle, out, gain, mean, invstddev, out_frames, (hipStream_t)stream);
}

}  // extern "C"
