"""Seeded differential fuzzing of the stand-alone spectrogram-domain ops on the device -- AmplitudeToDB (db_group_kernel),
MelScale (mel_scale_lds_kernel in both LDS regimes, mel_scale_kernel), TimeStretch / phase_vocoder (phase_vocoder_kernel),
GriffinLim (the 400 fast path, the power-of-two and the generic STFT / iSTFT kernels) and the MFCC tail (both DCT kernels) --
against tests/specdomain_oracle.py in float64, which tests/test_specdomain_oracle.py pins on the reference's stored outputs.
tests/test_gpu_fuzz.py and tests/test_gpu_fuzz_backward.py sweep the large kernels; these small ones rested on a few fixtures
that never reach the thresholds of their launch geometry (a dB group below / at / above one 8192-element chunk, a misaligned
base, the raised-LDS and the no-LDS MelScale launches, a ragged 16-frame tile, n_in of 1 or 2, n_out == 1, the zero pad read).

Every draw is a function of its seed alone (_draw_*), so the tests WITHOUT the gpu mark check, on any machine, that the
draws cover what they are meant to cover (test_draws_cover_the_gaps), that the clamped shares of the dB draws are what a
top_db test needs (test_db_clamped_share) and that the inputs and bars BITE: the oracle perturbed the way a kernel would
plausibly be wrong misses the bar of its own seed by at least 10 x (test_bite_*).  Every device case prints its figure before
asserting it ("[fuzz-specdomain] <family> seed=... err=... bar=... err/bar=..."; run with -s).

Bars (none is derived from the product's output):
  dB        1e-4 peak-relative, TOL["AmplitudeToDB"] of tests/test_gpu_parity.py
  MelScale  2e-5 peak-relative, the forward fuzz's bar for mel outputs
  vocoder   magnitudes 1e-5 (test_phase_vocoder_vs_reference); complex values max(2e-5, 4 x the float32 oracle's distance
            from the float64 oracle), the yardstick rule of test_fuzz_inverse_spectrogram_vs_aten_istft
  GriffinLim min(2e-3, max(2e-5, 4 x the float32 oracle's distance from the float64 oracle))
  MFCC tail 2e-3 * max(1, peak / 80) absolute, the forward fuzz's bar for MFCC

Measured without a device, with the seed bases below (oracle only): the dB clamped shares (test_db_clamped_share's docstring),
the vocoder and GriffinLim yardsticks (test_vocoder_yardsticks, test_griffinlim_yardsticks), the bite table (BITE_MEASURED).
Measured on an MI355X: MEASURED_DEVICE.

The vocoder's magnitudes come closest to their bar (0.70 x at n_in = 120, rate 1.3): the kernel's time steps are
float(t * rate) with the product in float64, torch.arange's vectorised float32 evaluation (base + k * float(rate)) differs from
that by one ulp of the time step on some frames -- 7.6e-6 at t ~ 100 -- and the interpolation weight alpha with it.  The CPU
replay of the kernel (tests/cpu_sim) gives the same 0.70 x; the frames chosen agree on every draw.

A NaN element: csrc/db_mfcc.h keeps it (torch.clamp does; fmax did not) and takes the group maximum over the group's OTHER
elements, where the reference's amax() turns the whole group into NaN -- README "Contract".
test_db_special_values_in_one_group states both halves.
"""
import math
import warnings

import numpy as np
import pytest
import torch

from conftest import peak_rel_err
import specdomain_oracle as SO

# seed bases, disjoint from tests/test_gpu_fuzz.py (1000 .. 7000) and tests/test_gpu_fuzz_backward.py (11260 .. 16020); chosen on
# the CPU so that the draws cover what test_draws_cover_the_gaps lists
BASE = dict(db=21000, mel=22002, vocoder=23000, griffinlim=24000)
DB_SEEDS, MEL_SEEDS, VOC_SEEDS, GL_SEEDS = 24, 16, 16, 8

# family -> (worst err / bar, its seed or case) on an MI355X with the bases above, from the "[fuzz-specdomain]" lines of one
# device run of this file (102 device cases, all passed)
MEASURED_DEVICE = {"dB": (0.002, 23), "MelScale": (0.096, 13), "vocoder |.|": (0.698, 3), "vocoder": (0.559, 13),
                   "GriffinLim": (0.293, 3), "MFCC tail": (0.066, "160x40")}

_WORST = {}


def _rng(seed):
    return np.random.default_rng(seed)


def _note(family, seed, what, err, bar):
    ratio = err / bar
    _WORST[family] = max(_WORST.get(family, 0.0), ratio)
    print(f"[fuzz-specdomain] {family} seed={seed} {what}: err={err:.3e} bar={bar:.3e} err/bar={ratio:.3f} "
          f"(worst so far {_WORST[family]:.3f})")
    return ratio


def _np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from audio_amd import _lib
    _lib.lib()
    return torch.device("cuda", 0)


# --------------------------------------------------------------------------- #
# 1. amplitude_to_DB                                                          #
# --------------------------------------------------------------------------- #

# (C, F, T) of one cut-off group: 1, 3, 4, 5 elements (shorter than one float4 / one head), one element under, at and over one
# and two kDbChunk = 8192 chunks, odd sizes in between
DB_GROUPS = [(1, 1, 1), (1, 3, 1), (1, 2, 2), (1, 1, 5), (1, 1, 8191), (1, 64, 128), (3, 1, 2731), (2, 17, 241), (1, 99, 101),
             (3, 5, 823), (2, 64, 128), (5, 29, 113)]
DB_GROUP_SIZES = [1, 3, 4, 5, 8191, 8192, 8193, 8194, 9999, 12345, 16384, 16385]
DB_LAYOUTS = ["contiguous", "misaligned", "frame_major", "slice"]


def _draw_db(seed):
    r = _rng(BASE["db"] + seed)
    C, Fq, T = DB_GROUPS[seed % len(DB_GROUPS)]
    n_groups = int(r.choice([1, 3, 5, 7]))
    if n_groups == 1:
        lead = [None, (), (1,), (1, 1)][int(r.integers(0 if C == 1 else 1, 4))]      # rank 2 only has C = 1
    else:
        lead = [(n_groups,), (n_groups, 1), (1, n_groups)][int(r.integers(0, 3))]
    shape = (Fq, T) if lead is None else tuple(lead) + (C, Fq, T)
    stype = str(r.choice(["power", "magnitude"]))
    top_db = [None, 20.0, 40.0, 80.0][int(r.integers(0, 4))]
    if C * Fq * T == 1 and top_db is not None:
        # pinned: a group of ONE element is its own maximum, so a cut-off from the wrong group only shows when top_db is under
        # the 30 dB between neighbouring groups (test_bite_db: 0 x the bar at 80 dB)
        stype, top_db = "power", 20.0
    return dict(shape=shape, group=C * Fq * T, n_groups=n_groups, stype=stype, top_db=top_db, layout=str(r.choice(DB_LAYOUTS)))


def _db_values(cfg, seed):
    """randn^2 with decades between neighbouring groups: group k times 10^((3 k mod 7) - 3), so that a cut-off taken from the wrong
    group misses by tens of dB.  float32, contiguous, CPU."""
    g = torch.Generator().manual_seed(BASE["db"] + seed)
    x = torch.randn(cfg["n_groups"], cfg["group"], generator=g).pow(2)
    gain = torch.tensor([10.0 ** ((3 * k) % 7 - 3) for k in range(cfg["n_groups"])])
    return (x * gain[:, None]).reshape(cfg["shape"])


def _db_args(cfg):
    return (10.0 if cfg["stype"] == "power" else 20.0), 1e-10, 0.0, cfg["top_db"]


def _db_layout(x, layout):
    """The same values on the device in one of the four layouts."""
    if layout == "contiguous":
        return x.cuda()
    if layout == "misaligned":                # base one float past a 16-byte boundary: the all-scalar route of db_group_kernel
        big = torch.empty(x.numel() + 8, device="cuda")
        v = big.flatten()[1:1 + x.numel()].view(x.shape)
        v.copy_(x)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v
    if layout == "frame_major":               # what Spectrogram / MelScale return: (..., F, T) view of (..., T, F) memory
        return x.cuda().transpose(-1, -2).contiguous().transpose(-1, -2)
    big = torch.zeros(x.shape[:-1] + (2 * x.shape[-1] + 1,), device="cuda")
    v = big[..., 1::2]
    v.copy_(x)
    return v


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(DB_SEEDS))
def test_fuzz_amplitude_to_db_vs_oracle(seed, dev):
    import audio_amd.functional as F
    import audio_amd.transforms as T
    cfg = _draw_db(seed)
    x = _db_values(cfg, seed)
    ref = SO.amplitude_to_db(x, *_db_args(cfg))
    xd = _db_layout(x, cfg["layout"])
    assert torch.equal(xd.cpu(), x), cfg
    with torch.no_grad():
        got = T.AmplitudeToDB(cfg["stype"], cfg["top_db"])(xd)
        fn = F.amplitude_to_DB(xd, *_db_args(cfg))
    assert got.shape == ref.shape and got.dtype == torch.float32, cfg
    assert torch.equal(got, fn), cfg
    if cfg["layout"] in ("contiguous", "misaligned"):
        assert got.is_contiguous(), cfg
    if cfg["layout"] == "frame_major":        # memory order kept (strides of size-1 dimensions carry no information)
        keep = [i for i, n in enumerate(got.shape) if n > 1]
        assert [got.stride(i) for i in keep] == [xd.stride(i) for i in keep], (cfg, got.stride(), xd.stride())
    e = peak_rel_err(_np(got), ref.numpy())
    _note("dB", seed, str(cfg), e, 1e-4)
    assert e <= 1e-4, (cfg, e)


SPECIALS = {"with_inf": [0.0, -1.0, 1e-40, 1e-10, math.inf, math.nan, 1.0, 250.0],
            "finite": [0.0, -1.0, 1e-40, 1e-10, 3e-3, math.nan, 1.0, 250.0]}


@pytest.mark.gpu
@pytest.mark.parametrize("values", sorted(SPECIALS))
@pytest.mark.parametrize("top_db", [None, 80.0, 20.0])
@pytest.mark.parametrize("layout", ["contiguous", "misaligned"])           # the float4 body and the scalar route
def test_db_special_values_in_one_group(values, top_db, layout, dev):
    """0, a negative value, a subnormal, amin itself, +inf and NaN in ONE cut-off group.  A NaN element comes out NaN
    (torch.clamp keeps it; the kernel's fmax() returned amin's -100 dB until this test) and -- the product's contract, not the
    reference's -- does NOT poison the group: the cut-off is the maximum over the other elements, every other element is what
    the reference gives for the group without the NaN.  With +inf in the group the cut-off is +inf and every other element
    becomes +inf, as in the reference."""
    import audio_amd.functional as F
    x = torch.tensor(SPECIALS[values], dtype=torch.float32).repeat(3).reshape(4, 6)          # 24 elements: body and tail
    for mult in (10.0, 20.0):
        exp = SO.amplitude_to_db(x, mult, 1e-10, 0.0, top_db, nan_poisons_group=False)
        with torch.no_grad():
            got = F.amplitude_to_DB(_db_layout(x, layout), mult, 1e-10, 0.0, top_db).cpu()
        assert torch.equal(torch.isnan(got), torch.isnan(x)), (values, top_db, mult, got)
        np.testing.assert_allclose(got.numpy(), exp.numpy(), rtol=0, atol=1e-4 * 100.0, equal_nan=True)
        if top_db is not None:                # which of the two group rules holds: the reference's would be all-NaN here
            assert bool(torch.isnan(SO.amplitude_to_db(x, mult, 1e-10, 0.0, top_db)).all())
            assert not bool(torch.isnan(got).all())


@pytest.mark.gpu
@pytest.mark.parametrize("n_mels,n_mfcc", [(40, 13), (23, 13)])            # the matrix-core kernel, the scalar kernel
def test_mfcc_tail_keeps_a_nan_in_its_db_modes(n_mels, n_mfcc, dev):
    """aamd_mfcc_dct_f32 with a NaN mel value: log_mode 0 (dB in the tail) and log_mode 2 (dB values in, top_db clamp in the
    tail) give a NaN frame, as torch.clamp / torch.max + matmul do; the other frames are untouched."""
    import audio_amd.functional as F
    from audio_amd import _host
    g = torch.Generator().manual_seed(n_mels)
    mel = torch.randn(19, n_mels, generator=g).pow(2)
    mel[7, 5] = math.nan
    dct = _host.create_dct(n_mfcc, n_mels, "ortho").contiguous()
    db = SO.amplitude_to_db(mel, 10.0, 1e-10, 0.0, None)
    gmax = torch.where(torch.isnan(db), torch.full_like(db, -math.inf), db).amax().reshape(1)
    want0 = db @ dct.double()
    want2 = torch.max(db, gmax - 30.0) @ dct.double()
    with torch.no_grad():
        got0 = F._mfcc_dct_launch(mel.cuda(), dct.cuda(), 0, None, 1, -1.0).cpu()
        got2 = F._mfcc_dct_launch(db.float().cuda(), dct.cuda(), 2, gmax.float().cuda(), 19, 30.0).cpu()
    for got, want in ((got0, want0), (got2, want2)):
        assert bool(torch.isnan(got[7]).all()) and int(torch.isnan(got).sum()) == n_mfcc
        np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=0, atol=2e-3, equal_nan=True)


# --------------------------------------------------------------------------- #
# 2. MelScale                                                                 #
# --------------------------------------------------------------------------- #

K_MS_VEC = 16                                 # csrc/db_mfcc.h kMsVec


def ms_lds_bytes(n_mels, max_width, n_freq):
    """csrc/db_mfcc.h ms_lds_floats() * sizeof(float)"""
    return 4 * (n_mels * (max_width | 1) + 2 * n_mels + K_MS_VEC * (n_freq | 1))


def _regime(lds):
    return 1 if lds <= 48 * 1024 else 2 if lds <= 96 * 1024 else 3


def _draw_mel(seed):
    r = _rng(BASE["mel"] + seed)
    bank = str(r.choice(["mel", "mel", "mel", "dense", "empty_columns"]))
    n_freq = int(r.choice([33, 201, 257, 513, 1025, 2049]))
    n_mels = int(r.choice([1, 13, 40, 80, 128]))
    sr = int(r.choice([8000, 16000, 44100]))
    f_min = float(r.choice([0.0, 60.0, 300.0]))
    f_max = [None, sr / 2.0, sr / 4.0][int(r.integers(0, 3))]
    norm = [None, "slaney"][int(r.integers(0, 2))]
    scale = str(r.choice(["htk", "slaney"]))
    if bank == "empty_columns":               # 128 bands on 101 bins: the low bands fall between two bins (width == 0)
        n_freq, n_mels, sr, f_min, f_max = 101, 128, 16000, 0.0, None
    T = int(r.choice([1, 15, 16, 17, 37]))
    lead = [(), (2,), (2, 3)][int(r.integers(0, 3))]
    return dict(bank=bank, n_freq=n_freq, n_mels=n_mels, sr=sr, f_min=f_min, f_max=f_max, norm=norm, scale=scale, T=T,
                lead=lead, frame_major=bool(r.random() < 0.5))


def _mel_bank(cfg, seed):
    from audio_amd import _host
    if cfg["bank"] == "dense":                # a user filterbank without a zero: max_width == n_freq
        g = torch.Generator().manual_seed(BASE["mel"] + seed)
        return torch.rand(cfg["n_freq"], cfg["n_mels"], generator=g) + 0.01
    f_max = cfg["f_max"] if cfg["f_max"] is not None else float(cfg["sr"] // 2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")       # "At least one mel filterbank has all zero values": drawn on purpose
        return _host.melscale_fbanks(cfg["n_freq"], cfg["f_min"], f_max, cfg["n_mels"], cfg["sr"], cfg["norm"], cfg["scale"])


def _mel_lds(cfg, seed):
    from audio_amd import _host
    fb = _mel_bank(cfg, seed)
    _, width, _, max_width = _host.mel_band_table(fb.numpy())
    return ms_lds_bytes(fb.shape[1], max_width, fb.shape[0]), width, max_width


def _mel_spec(cfg, seed):
    g = torch.Generator().manual_seed(BASE["mel"] + 100 + seed)
    return torch.randn(*cfg["lead"], cfg["n_freq"], cfg["T"], generator=g).pow(2)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(MEL_SEEDS))
def test_fuzz_mel_scale_vs_oracle(seed, dev):
    import audio_amd.functional as F
    import audio_amd.transforms as T
    cfg = _draw_mel(seed)
    fb = _mel_bank(cfg, seed)
    spec = _mel_spec(cfg, seed)
    ref = SO.mel_scale(spec, fb)
    xd = spec.cuda()
    if cfg["frame_major"]:
        xd = xd.transpose(-1, -2).contiguous().transpose(-1, -2)
    fbd = fb.cuda()
    lds, _, max_width = _mel_lds(cfg, seed)
    assert F._mel_bands(fbd, dev).max_width == max_width, cfg              # the regime below is the one the launch takes
    with torch.no_grad():
        got = F.mel_scale(xd, fbd)
        if cfg["bank"] == "mel":              # the module builds the same bank
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                m = T.MelScale(cfg["n_mels"], cfg["sr"], cfg["f_min"], cfg["f_max"], cfg["n_freq"], cfg["norm"],
                               cfg["scale"]).cuda()
            assert torch.equal(m.fb.cpu(), fb), cfg
            assert torch.equal(m(xd), got), cfg
    assert got.shape == ref.shape and got.dtype == torch.float32, cfg
    e = peak_rel_err(_np(got), ref.numpy())
    _note("MelScale", seed, f"regime {_regime(lds)} ({lds} B) {cfg}", e, 2e-5)
    assert e <= 2e-5, (cfg, lds, e)


# --------------------------------------------------------------------------- #
# 3. phase vocoder                                                            #
# --------------------------------------------------------------------------- #

def _draw_vocoder(seed):
    r = _rng(BASE["vocoder"] + seed)
    n_freq = int(r.choice([1, 33, 201, 255, 256, 257]))
    n_in = int(r.choice([1, 2, 9, 57, 120]))
    rate = [0.5, 0.7, 0.9, 1.3, 2.0, 2.5, 3.0, float(n_in + 1)][int(r.integers(0, 8))]
    lead = [(), (2,), (2, 2), (1, 2, 2)][int(r.integers(0, 4))]
    hop = int(r.choice([1, 2, 4, 16, 160]))
    return dict(n_freq=n_freq, n_in=n_in, rate=rate, lead=lead, hop=hop, frame_major=bool(r.random() < 0.5))


def _vocoder_inputs(cfg, seed):
    g = torch.Generator().manual_seed(BASE["vocoder"] + seed)
    shape = tuple(cfg["lead"]) + (cfg["n_freq"], cfg["n_in"])
    spec = torch.complex(torch.randn(shape, generator=g), torch.randn(shape, generator=g))
    pa = torch.linspace(0, math.pi * cfg["hop"], cfg["n_freq"])[..., None]
    return spec, pa


def _vocoder_refs(cfg, seed):
    """(float64 oracle, complex bar): max(2e-5, 4 x the float32 oracle's distance from the float64 oracle)."""
    spec, pa = _vocoder_inputs(cfg, seed)
    ref = SO.phase_vocoder(spec.to(torch.complex128), cfg["rate"], pa)
    ref32 = SO.phase_vocoder(spec, cfg["rate"], pa)
    d32 = peak_rel_err(ref32.to(torch.complex128).numpy(), ref.numpy())
    return ref, max(2e-5, 4.0 * d32), d32, peak_rel_err(ref32.abs().double().numpy(), ref.abs().numpy())


def _vocoder_reads_the_pad(cfg):
    """Some output frame interpolates between the last input frame and the zero pad (i0 + 1 == n_in with alpha > 0)."""
    ts = torch.arange(0, cfg["n_in"], cfg["rate"], dtype=torch.float32)
    return bool(((ts.long() + 1 == cfg["n_in"]) & (ts % 1.0 > 0)).any())


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(VOC_SEEDS))
def test_fuzz_phase_vocoder_vs_oracle(seed, dev):
    import audio_amd.functional as F
    import audio_amd.transforms as T
    cfg = _draw_vocoder(seed)
    spec, pa = _vocoder_inputs(cfg, seed)
    ref, bar, _, _ = _vocoder_refs(cfg, seed)
    xd = spec.cuda()
    if cfg["frame_major"]:
        xd = xd.transpose(-1, -2).contiguous().transpose(-1, -2)
    with torch.no_grad():
        got = F.phase_vocoder(xd, cfg["rate"], pa.cuda())
        if cfg["n_freq"] > 1:                 # the module builds the same phase_advance (n_freq = 1 divides by zero in its n_fft)
            t = T.TimeStretch(hop_length=cfg["hop"], n_freq=cfg["n_freq"], fixed_rate=cfg["rate"]).cuda()
            assert torch.equal(t.phase_advance.cpu(), pa), cfg
            assert torch.equal(t(xd), got), cfg
    assert got.shape == ref.shape and got.dtype == torch.complex64 and got.is_contiguous(), (cfg, got.shape, ref.shape)
    assert got.shape[-1] == math.ceil(cfg["n_in"] / cfg["rate"]), cfg
    em = peak_rel_err(np.abs(_np(got)), np.abs(ref.numpy()))
    _note("vocoder |.|", seed, str(cfg), em, 1e-5)
    assert em <= 1e-5, (cfg, em)
    e = peak_rel_err(_np(got), ref.numpy())
    _note("vocoder", seed, str(cfg), e, bar)
    assert e <= bar, (cfg, e, bar)


# --------------------------------------------------------------------------- #
# 4. Griffin-Lim                                                              #
# --------------------------------------------------------------------------- #

GL_FRAMES = 30


def _draw_griffinlim(seed):
    r = _rng(BASE["griffinlim"] + seed)
    n_fft = [400, 512, 200, 96][seed % 4]     # the 400 fast path, the power-of-two kernel, the generic kernel (twice)
    hop = int(r.choice([n_fft // 4, n_fft // 2]))
    power = float(r.choice([1.0, 2.0]))
    n_iter = int(r.choice([2, 4]))
    momentum = float(r.choice([0.0, 0.99]))
    use_length = bool(r.random() < 0.5)
    lead = [(2,), (2, 2)][int(r.integers(0, 2))]
    length = hop * (GL_FRAMES - 1) + hop // 3 if use_length else None
    return dict(n_fft=n_fft, hop=hop, power=power, n_iter=n_iter, momentum=momentum, length=length, lead=lead)


def _griffinlim_spec(cfg, seed):
    """|STFT|^power of clipped noise plus a floor of 1e-3 of its peak: no bin is weak, so the 1 / |angles| step does not
    amplify rounding without bound.  float32, (lead, n_fft / 2 + 1, 30)."""
    g = torch.Generator().manual_seed(BASE["griffinlim"] + seed)
    x = (0.5 * torch.randn(*cfg["lead"], cfg["hop"] * (GL_FRAMES - 1), generator=g, dtype=torch.float64)).clamp_(-1, 1)
    w = torch.hann_window(cfg["n_fft"], dtype=torch.float64)
    s = torch.stft(x.reshape(-1, x.shape[-1]), cfg["n_fft"], cfg["hop"], cfg["n_fft"], w, True, "reflect", False, True,
                   return_complex=True).abs().pow(cfg["power"])
    s = s.reshape(tuple(cfg["lead"]) + s.shape[-2:])
    assert s.shape[-1] == GL_FRAMES
    return (s + 1e-3 * s.max()).float()


def _griffinlim_refs(cfg, seed, bite=None):
    spec = _griffinlim_spec(cfg, seed)
    args = (cfg["n_fft"], cfg["hop"], cfg["n_fft"], cfg["power"], cfg["n_iter"], cfg["momentum"], cfg["length"])
    ref = SO.griffinlim(spec, torch.hann_window(cfg["n_fft"], dtype=torch.float64), *args)
    if bite is not None:
        return ref, SO.griffinlim(spec, torch.hann_window(cfg["n_fft"], dtype=torch.float64), *args, bite=bite)
    ref32 = SO.griffinlim(spec, torch.hann_window(cfg["n_fft"]), *args, dtype=torch.float32)
    d32 = peak_rel_err(ref32.double().numpy(), ref.numpy())
    return ref, min(2e-3, max(2e-5, 4.0 * d32)), d32


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(GL_SEEDS))
def test_fuzz_griffinlim_vs_oracle(seed, dev):
    import audio_amd.transforms as T
    cfg = _draw_griffinlim(seed)
    spec = _griffinlim_spec(cfg, seed)
    ref, bar, _ = _griffinlim_refs(cfg, seed)
    with torch.no_grad():
        t = T.GriffinLim(n_fft=cfg["n_fft"], hop_length=cfg["hop"], power=cfg["power"], n_iter=cfg["n_iter"],
                         momentum=cfg["momentum"], length=cfg["length"], rand_init=False).cuda()
        got = t(spec.cuda())
    assert got.shape == ref.shape and got.dtype == torch.float32, (cfg, got.shape, ref.shape)
    e = peak_rel_err(_np(got), ref.numpy())
    _note("GriffinLim", seed, str(cfg), e, bar)
    assert e <= bar, (cfg, e, bar)


# --------------------------------------------------------------------------- #
# 5. MFCC tail                                                                #
# --------------------------------------------------------------------------- #

# (n_mels, n_mfcc): aamd_mfcc_dct_f32 takes the scalar kernel for n_mels > 128 (132, 160) and n_mfcc > 64 (65, 80) -- the forward
# fuzz only ever took it for n_mels % 4 != 0 -- and the matrix-core kernel at its small end (20 x 20 with a ragged coefficient
# tile, 4 x 1)
MFCC_TAIL_CASES = [(132, 13), (160, 40), (128, 65), (128, 80), (20, 20), (4, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("lead", [(2,), (2, 2)], ids=["2d", "3d"])
@pytest.mark.parametrize("log_mels", [False, True])
@pytest.mark.parametrize("n_mels,n_mfcc", MFCC_TAIL_CASES)
def test_mfcc_tail_shapes_vs_oracle(n_mels, n_mfcc, log_mels, lead, dev):
    """T.MFCC on its two-kernel path (fused = False: the mel kernel, then aamd_mfcc_dct_f32 -- the kernel this test is about)
    against mfcc_tail of the float64 mel spectrogram; top_db = 80 with one cut-off per (C, n_mels, T) block of a 3-D input.
    Row 1 is 60 dB under row 0, and the tail of row 0 is digital silence, so the cut-off is at work."""
    import audio_amd.transforms as T
    from oracle import torch_cpu_ref as R
    n_fft, hop = (400, 200) if n_mels in (132, 128, 4) else (512, 128)
    g = torch.Generator().manual_seed(n_mels * 100 + n_mfcc)
    x = (0.5 * torch.randn(*lead, 2300, generator=g)).clamp_(-1, 1)
    x.reshape(-1, 2300)[1] *= 1e-3
    x.reshape(-1, 2300)[0, 1500:] = 0.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")       # 132 / 160 bands on 201 / 257 bins leave empty bands: part of the case
        m = T.MFCC(sample_rate=16000, n_mfcc=n_mfcc, log_mels=log_mels,
                   melkwargs=dict(n_fft=n_fft, hop_length=hop, n_mels=n_mels)).cuda()
    m.fused = False
    with torch.no_grad():
        got = m(x.cuda())
    w = torch.hann_window(n_fft, dtype=torch.float64)
    mel64 = R.mel_spectrogram(x.double(), w, m.MelSpectrogram.mel_scale.fb.cpu().double(), n_fft, hop)
    ref = SO.mfcc_tail(mel64, m.dct_mat.cpu().double(), log_mels, 80.0)
    assert got.shape == ref.shape and got.dtype == torch.float32
    if not log_mels:
        db = SO.amplitude_to_db(mel64, 10.0, 1e-10, 0.0, None)
        assert bool((db < SO.amplitude_to_db(mel64, 10.0, 1e-10, 0.0, 80.0)).any())     # the clamp is exercised
    err = float(np.abs(_np(got) - ref.numpy()).max())
    bar = 2e-3 * max(1.0, float(ref.abs().max()) / 80.0)
    _note("MFCC tail", f"{n_mels}x{n_mfcc}", f"log_mels={log_mels} lead={lead}", err, bar)
    assert err <= bar, (n_mels, n_mfcc, log_mels, lead, err, bar)


# --------------------------------------------------------------------------- #
# no device: coverage of the draws, clamped shares, yardsticks, bite          #
# --------------------------------------------------------------------------- #

def test_draws_cover_the_gaps():
    """The seed bases were chosen so that the draws reach what the fixtures never had; checked here so that a change of a
    base or of a draw cannot silently lose one."""
    db = [_draw_db(s) for s in range(DB_SEEDS)]
    assert sorted({c["group"] for c in db}) == DB_GROUP_SIZES
    assert [c["group"] for c in db[:len(DB_GROUPS)]] == [a * b * c for a, b, c in DB_GROUPS]
    assert {len(c["shape"]) for c in db} == {2, 3, 4, 5}
    assert {c["n_groups"] for c in db} == {1, 3, 5, 7}
    assert {c["layout"] for c in db} == set(DB_LAYOUTS)
    assert {c["top_db"] for c in db} == {None, 20.0, 40.0, 80.0} and {c["stype"] for c in db} == {"power", "magnitude"}
    assert any(c["layout"] == "frame_major" and c["top_db"] is not None and c["n_groups"] > 1 for c in db)
    assert any(c["layout"] == "misaligned" and c["group"] > 8192 for c in db)
    assert any(c["n_groups"] > 2 and c["group"] < 8192 for c in db) and any(c["n_groups"] > 2 and c["group"] > 8192 for c in db)
    for c in db:
        n = 1
        for d in c["shape"]:
            n *= d
        assert n == c["group"] * c["n_groups"], c

    mel = [_draw_mel(s) for s in range(MEL_SEEDS)]
    regimes = {}
    for s, c in enumerate(mel):
        lds, width, max_width = _mel_lds(c, s)
        regimes.setdefault(_regime(lds), []).append(s)
        if c["bank"] == "dense":
            assert max_width == c["n_freq"]
        if c["bank"] == "empty_columns":
            assert int((width == 0).sum()) > 0
    assert all(len(regimes.get(k, [])) >= 2 for k in (1, 2, 3)), regimes
    assert regimes == MEL_REGIME_SEEDS, regimes
    assert {c["bank"] for c in mel} == {"mel", "dense", "empty_columns"}
    assert {c["T"] for c in mel} >= {1, 15, 16, 17, 37} and {c["lead"] for c in mel} == {(), (2,), (2, 3)}
    assert {c["n_freq"] for c in mel} >= {33, 201, 257, 513, 1025, 2049}
    assert {c["n_mels"] for c in mel} >= {1, 13, 40, 80, 128}
    assert {c["norm"] for c in mel} == {None, "slaney"} and {c["frame_major"] for c in mel} == {True, False}

    voc = [_draw_vocoder(s) for s in range(VOC_SEEDS)]
    assert {c["n_in"] for c in voc} == {1, 2, 9, 57, 120}
    assert {c["n_freq"] for c in voc} == {1, 33, 201, 255, 256, 257}
    assert {c["lead"] for c in voc} == {(), (2,), (2, 2), (1, 2, 2)} and {c["frame_major"] for c in voc} == {True, False}
    assert {c["hop"] for c in voc} == {1, 2, 4, 16, 160}
    assert any(c["rate"] == c["n_in"] + 1 for c in voc)                     # n_out == 1
    whole = [float(c["n_in"] / c["rate"]).is_integer() for c in voc]
    assert any(whole) and not all(whole)
    assert sum(_vocoder_reads_the_pad(c) for c in voc) >= 4
    chains = [int(np.prod(c["lead"], dtype=np.int64)) * c["n_freq"] for c in voc]
    assert any(n < 256 for n in chains) and any(n % 256 for n in chains if n > 256) and any(n % 256 == 0 for n in chains)

    gl = [_draw_griffinlim(s) for s in range(GL_SEEDS)]
    assert {c["n_fft"] for c in gl} == {400, 512, 200, 96}
    assert {c["momentum"] for c in gl} == {0.0, 0.99} and {c["length"] is None for c in gl} == {True, False}
    assert {c["power"] for c in gl} == {1.0, 2.0} and {c["n_iter"] for c in gl} == {2, 4} and {c["lead"] for c in gl} == {(2,), (2, 2)}
    assert {c["hop"] * 4 // c["n_fft"] for c in gl} == {1, 2}
    assert any(c["n_fft"] in (200, 96) and c["momentum"] == 0.0 for c in gl)
    assert any(c["n_fft"] in (200, 96) and c["length"] is None for c in gl)


# MelScale regimes of the suite's seeds (<= 48 KiB, 48 .. 96 KiB: the raised-LDS launch, > 96 KiB: mel_scale_kernel)
MEL_REGIME_SEEDS = {1: [1, 2, 5, 8, 9, 10, 11, 12, 14], 2: [3, 15], 3: [0, 4, 6, 7, 13]}


def _db_shares():
    pooled = {}
    for s in range(DB_SEEDS):
        c = _draw_db(s)
        if c["top_db"] is None:
            continue
        x = _db_values(c, s)
        mult, amin, dbm, _ = _db_args(c)
        clamped = SO.amplitude_to_db(x, mult, amin, dbm, None) < SO.amplitude_to_db(x, mult, amin, dbm, c["top_db"])
        a = pooled.setdefault((c["stype"], c["top_db"]), [0, 0])
        a[0] += int(clamped.sum())
        a[1] += clamped.numel()
    return {k: v[0] / v[1] for k, v in pooled.items()}


def test_db_clamped_share():
    """The share of elements under their group's cut-off, from the oracle alone, pooled over the suite's draws per (stype,
    top_db): a top_db test needs both sides of the clamp populated.  Measured with the bases above:
        power      top_db 20: 32.0 %   40: 3.24 %   80: 0.031 %      (per draw 30.6 .. 32.9 %, 3.2 .. 3.4 %, 0.024 .. 0.041 %)
        magnitude  top_db 20: 79.6 %   40: 31.9 %   80: 3.23 %       (per draw 78 .. 81 %, 31.4 .. 33.2 %, 3.1 .. 3.3 %)
    20 log10 doubles the spread of 10 log10, so "magnitude" at top_db is "power" at top_db / 2 and takes that row's range;
    magnitude at 20 dB (= power at 10 dB) has no such row: 60 .. 90 % around the measured 79.6 %.  Groups of 1 .. 5 elements
    contribute next to nothing to the pooled shares (a group of one element is never clamped)."""
    share = _db_shares()
    print("[fuzz-specdomain] dB clamped share", share)
    assert 0.10 <= share[("power", 20.0)] <= 0.50 and 0.10 <= share[("magnitude", 40.0)] <= 0.50, share
    assert 0.01 <= share[("power", 40.0)] <= 0.10 and 0.01 <= share[("magnitude", 80.0)] <= 0.10, share
    assert 0.0 < share[("power", 80.0)] <= 0.01, share
    assert 0.60 <= share[("magnitude", 20.0)] <= 0.90, share


def test_vocoder_yardsticks():
    """float32 oracle against float64 oracle per seed: the distance grows with the accumulated phase, so the large-hop draws
    check magnitudes and frame selection and the small-hop draws the phase -- at least half of the seeds must have a complex
    bar under 1e-4.  Measured: 7.5e-8 (n_in 2, hop 16) .. 1.84e-4 (n_freq 201, n_in 57, rate 0.7, hop 16), 1.05e-4 at
    (256, 120) with hop 16, 4.8e-5 at (201, 120) with hop 4; 12 of the 16 bars are under 1e-4 (seeds 3, 9, 10, 15 are not).
    Magnitudes of the float32 oracle stay within 1.2e-7 of the float64 ones (asserted: 1e-6)."""
    bars, mags = [], []
    for s in range(VOC_SEEDS):
        _, bar, d32, m32 = _vocoder_refs(_draw_vocoder(s), s)
        print(f"[fuzz-specdomain] vocoder yardstick seed={s} d32={d32:.2e} bar={bar:.2e} |.| d32={m32:.2e}")
        bars.append(bar)
        mags.append(m32)
    assert sum(b < 1e-4 for b in bars) >= VOC_SEEDS // 2, bars
    assert max(mags) <= 1e-6, mags


def test_griffinlim_yardsticks():
    """float32 oracle against float64 oracle per seed; every bar must stay under the 2e-3 of the fixture test without the cap
    having to act, or the inputs are too ill-conditioned to test anything.  Measured: 9.7e-7 .. 4.6e-6 (the floor of 1e-3 of
    the peak keeps every bin strong), so 4 x is under 2e-5 and every seed's bar is 2e-5."""
    for s in range(GL_SEEDS):
        _, bar, d32 = _griffinlim_refs(_draw_griffinlim(s), s)
        print(f"[fuzz-specdomain] GriffinLim yardstick seed={s} d32={d32:.2e} bar={bar:.2e}")
        assert 4.0 * d32 <= 2e-3, (s, d32)


def _bite_db(kind):
    worst = math.inf
    for s in range(DB_SEEDS):
        c = _draw_db(s)
        if c["top_db"] is None or c["n_groups"] < 2:
            continue                          # one group, or no cut-off: the perturbation is the identity
        x = _db_values(c, s)
        ref = SO.amplitude_to_db(x, *_db_args(c))
        bad = SO.amplitude_to_db(x, *_db_args(c), bite=kind)
        worst = min(worst, peak_rel_err(bad.numpy(), ref.numpy()) / 1e-4)
    return worst


def _bite_mel():
    worst = math.inf
    for s in range(MEL_SEEDS):
        c = _draw_mel(s)
        fb, spec = _mel_bank(c, s), _mel_spec(c, s)
        worst = min(worst, peak_rel_err(SO.mel_scale(spec, fb, bite="band_start").numpy(), SO.mel_scale(spec, fb).numpy()) / 2e-5)
    return worst


def _bite_vocoder(kind):
    worst = math.inf
    for s in range(VOC_SEEDS):
        c = _draw_vocoder(s)
        if kind == "no_pad" and not _vocoder_reads_the_pad(c):
            continue                          # no frame of this draw touches the pad with a non-zero weight
        if kind in ("no_readd", "floor_wrap") and (c["n_freq"] == 1 or math.ceil(c["n_in"] / c["rate"]) < 2):
            continue                          # phase_advance = 0, or no second output frame: the identity
        spec, pa = _vocoder_inputs(c, s)
        ref, bar, _, _ = _vocoder_refs(c, s)
        bad = SO.phase_vocoder(spec.to(torch.complex128), c["rate"], pa, bite=kind)
        if kind == "no_pad":
            ratio = peak_rel_err(bad.abs().numpy(), ref.abs().numpy()) / 1e-5
        else:
            ratio = peak_rel_err(bad.numpy(), ref.numpy()) / bar
        worst = min(worst, ratio)
    return worst


def _bite_griffinlim():
    worst = math.inf
    for s in range(GL_SEEDS):
        c = _draw_griffinlim(s)
        if c["momentum"] == 0.0:
            continue
        _, bar, _ = _griffinlim_refs(c, s)
        ref, bad = _griffinlim_refs(c, s, bite="raw_momentum")
        worst = min(worst, peak_rel_err(bad.numpy(), ref.numpy()) / bar)
    return worst


# smallest (perturbed oracle - oracle) / bar over the seeds a perturbation applies to, measured on the CPU with the bases above
BITE_MEASURED = {
    "dB: group one element too long": 1.66e3,                   # over the 14 seeds with top_db and more than one group
    "dB: cut-off of the neighbouring group": 1.78e3,            # the same 14 seeds
    "MelScale: one band start one bin too high": 98.2,          # all 16 seeds; the smallest is the single 255-bin band of seed 5
    "vocoder: frame i0 + 1 == n_in read without the zero pad": 1.03e4,       # magnitudes, the 8 seeds whose last frame needs the pad
    "vocoder: first term of the running sum dropped": 2.67e3,   # all 16 seeds
    "vocoder: phase_advance not added back after the wrap": 2.46e3,          # seeds with n_freq > 1 and a second output frame
    "vocoder: floor in place of round-half-even in the wrap": 0.0,           # an invariance: see
                                                                             # test_vocoder_wrap_rule_cannot_be_seen_in_the_output
    "GriffinLim: momentum not scaled by 1 / (1 + m)": 2.17e3,   # the 4 seeds with momentum 0.99
}


def test_bite_db():
    for kind in ("group_size", "neighbour_cut"):
        w = _bite_db(kind)
        print(f"[fuzz-specdomain] bite dB {kind}: smallest err/bar {w:.3g}")
        assert w >= 10.0, (kind, w)


def test_bite_mel_scale():
    w = _bite_mel()
    print(f"[fuzz-specdomain] bite MelScale band_start: smallest err/bar {w:.3g}")
    assert w >= 10.0, w


def test_bite_vocoder():
    for kind in ("no_pad", "drop_first", "no_readd"):
        w = _bite_vocoder(kind)
        print(f"[fuzz-specdomain] bite vocoder {kind}: smallest err/bar {w:.3g}")
        assert w >= 10.0, (kind, w)


def test_vocoder_wrap_rule_cannot_be_seen_in_the_output():
    """floor in place of round-half-even in `phase - 2 pi round(phase / 2 pi)` moves a phase step by a whole multiple of 2 pi,
    and the step only ever enters the output through cos / sin of the running sum: the float64 oracle with either rule gives
    the same values to rounding (3e-11 x the bar at worst), whatever the input.  No draw can make this perturbation bite, so it
    is stated as what it is -- an invariance -- and "no_readd" (phase_advance not added back after the wrap, the other way to
    get that line wrong) stands in for it in test_bite_vocoder."""
    w = 0.0
    for s in range(VOC_SEEDS):
        c = _draw_vocoder(s)
        spec, pa = _vocoder_inputs(c, s)
        ref = SO.phase_vocoder(spec.to(torch.complex128), c["rate"], pa)
        bad = SO.phase_vocoder(spec.to(torch.complex128), c["rate"], pa, bite="floor_wrap")
        w = max(w, peak_rel_err(bad.numpy(), ref.numpy()))
    print(f"[fuzz-specdomain] vocoder floor_wrap: largest distance {w:.3g}")
    assert w <= 1e-9, w


def test_bite_griffinlim():
    w = _bite_griffinlim()
    print(f"[fuzz-specdomain] bite GriffinLim raw_momentum: smallest err/bar {w:.3g}")
    assert w >= 10.0, w
