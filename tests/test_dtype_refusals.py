"""The type-generic entry points of the C ABI refuse an element-type code they do not serve before anything is launched:
the return code and the aamd_last_error text of each, called with that code, null buffers and zero sizes (no GPU here).
The launchers share one dispatch and one element-size vocabulary (csrc/api_common.h); every refusal below is the entry
point's own and its text is part of the ABI."""
import ctypes
import os

import pytest

from audio_amd import _lib

AAMD_EINVAL = -1
F64 = 1          # AAMD_SA_F64
UNKNOWN = 99

# (entry point, index of its element-type argument, code passed, text after "audio_amd: ")
REFUSALS = [
    ("aamd_spec_augment_iid", 8, UNKNOWN, "spec_augment: unknown element type"),
    ("aamd_spec_augment_shared", 8, UNKNOWN, "spec_augment: unknown element type"),
    ("aamd_add_noise_lp", 15, UNKNOWN, "add_noise: the low-precision entry takes AAMD_SA_F16 or AAMD_SA_BF16"),
    ("aamd_add_noise_lp", 15, F64, "add_noise: the low-precision entry takes AAMD_SA_F16 or AAMD_SA_BF16"),
    ("aamd_preemphasis_lp", 6, UNKNOWN, "preemphasis: the low-precision entry takes AAMD_SA_F16 or AAMD_SA_BF16"),
    ("aamd_preemphasis_lp", 6, F64, "preemphasis: the low-precision entry takes AAMD_SA_F16 or AAMD_SA_BF16"),
    ("aamd_beamform_psd", 0, UNKNOWN, "beamform: unknown element type"),
    ("aamd_beamform_weights", 0, UNKNOWN, "beamform: unknown element type"),
    ("aamd_beamform_apply", 0, UNKNOWN, "beamform: unknown element type"),
    ("aamd_rnnt_loss_forward", 0, UNKNOWN, "rnnt_loss: unknown element type"),
    ("aamd_rnnt_loss_backward", 0, UNKNOWN, "rnnt_loss: unknown element type"),
    ("aamd_forced_align", 0, UNKNOWN, "forced_align: unknown element type"),
    ("aamd_overdrive", 0, UNKNOWN, "overdrive: unknown element type"),
    ("aamd_phaser", 0, UNKNOWN, "phaser: unknown element type"),
    ("aamd_flanger", 0, UNKNOWN, "flanger: unknown element type"),
    ("aamd_ctc_beam_search", 0, UNKNOWN, "ctc_beam_search: unknown element type"),
    ("aamd_inverse_mel", 0, UNKNOWN, "inverse_mel: float32, float16 or bfloat16 elements"),
    ("aamd_inverse_mel", 0, F64, "inverse_mel: float32, float16 or bfloat16 elements"),
    ("aamd_vad_measure", 0, UNKNOWN, "vad: unknown element type"),
    ("aamd_spectral_centroid", 0, UNKNOWN, "spectral_centroid: the result is float32, float16 or bfloat16"),
    ("aamd_spectral_centroid", 0, F64, "spectral_centroid: the result is float32, float16 or bfloat16"),
    ("aamd_pointwise", 1, UNKNOWN, "pointwise: unknown element type"),
    ("aamd_simulate_rir", 0, UNKNOWN, "simulate_rir: the element type must be float32 or float64"),
    ("aamd_ray_trace", 0, UNKNOWN, "ray_trace: the element type must be float32 or float64"),
    ("aamd_oscillator_bank", 0, UNKNOWN, "oscillator_bank: the element type must be float32, float64, float16 or bfloat16"),
    ("aamd_filter_waveform", 0, UNKNOWN, "filter_waveform: the element type must be float32, float64, float16 or bfloat16"),
    ("aamd_oscillator_bank_grad", 0, UNKNOWN,
     "oscillator_bank_grad: the element type must be float32, float64, float16 or bfloat16"),
    ("aamd_filter_waveform_grad", 0, UNKNOWN,
     "filter_waveform_grad: the element type must be float32, float64, float16 or bfloat16"),
    ("aamd_sinc_impulse_response", 0, UNKNOWN, "sinc_impulse_response: the element type must be float32 or float64"),
    ("aamd_frequency_impulse_response", 0, UNKNOWN, "frequency_impulse_response: the element type must be float32 or float64"),
    ("aamd_extend_pitch", 0, UNKNOWN, "extend_pitch: the element type must be float32, float64, float16 or bfloat16"),
    ("aamd_dense_fbank", 0, UNKNOWN, "dense_fbank: float32, float16 or bfloat16 elements"),
    ("aamd_dense_fbank", 0, F64, "dense_fbank: float32, float16 or bfloat16 elements"),
    ("aamd_stoi", 0, UNKNOWN, "stoi: unknown element type"),
    ("aamd_sdr", 0, UNKNOWN, "sdr: unknown element type"),
    ("aamd_si_sdr", 0, UNKNOWN, "si_sdr: unknown element type"),
    ("aamd_si_sdr_grad", 0, UNKNOWN, "si_sdr_grad: unknown element type"),
    ("aamd_pit_forward", 0, UNKNOWN, "pit_forward: unknown element type"),
    ("aamd_pit_assign", 0, UNKNOWN, "pit_assign: the matrix must be float32 or float64"),
    ("aamd_pit_grad", 0, UNKNOWN, "pit_grad: unknown element type"),
]


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libaudio_amd.so not built yet (python -m audio_amd._build)")
    return _lib.lib()


@pytest.mark.parametrize("name,index,code,text", REFUSALS, ids=lambda v: str(v) if isinstance(v, int) else v.split(":")[0])
def test_unserved_element_type_is_refused(L, name, index, code, text):
    _, argtypes = _lib._SIGS[name]
    args = [0.0 if t is ctypes.c_double else 0 if t in (ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64) else None
            for t in argtypes]
    assert argtypes[index] is ctypes.c_int32
    args[index] = code
    assert getattr(L, name)(*args) == AAMD_EINVAL
    assert L.aamd_last_error().decode() == "audio_amd: " + text


def test_size_queries_by_element_type(L):
    """The queries that size something from the element type do not refuse: an unknown code counts as a two-byte storage
    type with float32 arithmetic, except where the query itself returns 0 for it."""
    codes = (0, 1, 2, 3, UNKNOWN)        # AAMD_SA_F32, F64, F16, BF16
    assert [L.aamd_rnnt_team_width(d, 40) for d in codes] == [16, 32, 8, 8, 8]
    assert [L.aamd_rnnt_team_width(d, 100) for d in codes] == [32, 64, 16, 16, 16]
    assert [L.aamd_stoi_workspace(d, 2, 40000) for d in codes] == [82472, 156872, 82472, 82472, 82472]
    # flanger (effect 2) with a 4000-sample ring: one ring per row in the compute type
    assert [L.aamd_effects_workspace(2, d, 4, 1000, 4000) for d in codes] == [1024000, 2048000, 1024000, 1024000, 0]
