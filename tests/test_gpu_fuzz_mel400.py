"""Every instantiation of the n_fft = 400 kernel (csrc/melspec400.h, dispatched by csrc/mel400_launch.h) in LONG-RUN launches
against float64 ATen: epilogue (MEL, MEL_DB, SPEC, MEL_NORM, MFCC with its fix-up launch) x hop (100, 160, 200) x input type
(float, int16 mono, interleaved stereo, half, bfloat16) x NR (4, 8) x SIG (0, kSigHtk80, kSigSlaney80) x AR (packed, scalar).

Why: the launch gives each workgroup `tiles_per_block = ceil(n_tiles / blocks)` tiles with `blocks = min(cu_count,
ceil(n_tiles / 12))` rounded down to a multiple of 8, so a wave runs more than about two tiles only when
n_tiles > 12 * cu_count -- 18 000 frames on 256 CUs.  Every other comparison of this kernel with an independent reference stays
under 200 tiles; what only matters beyond that (claim() from the LDS queue, the prefetch of the next tile while the current
one is in phase B, tile_next's kCarry stepping across row boundaries in rows of >= 16 tiles, the division path in shorter rows
and in the stereo / MFCC instantiations, runs cut short at the end of the launch, the XCD remap) was covered by
self-consistency at full size only, which cannot see an error that both arms share.  Non-float inputs were only ever compared
with the float arm of the same kernel.

launch_split() is a host mirror of launch_fft400_nr's arithmetic and of the kernel's `tin_hi`; every device run ASSERTS the
regime it claims with the device's own CU count (a device with another count fails loudly, it does not pass vacuously), and the
mirror's n_frames against the product's output shape.  Regimes (shapes for 256 CUs, the smallest that reach the code):

  long        490 rows of 19 tiles: tiles_per_block 37, kCarry stepping live, runs end inside rows (37 % 19 != 0)
  short       rows of 2 / 5 / 15 tiles, tiles_per_block 37: the division path, many row boundaries per run
  one         ONE clip of 9 234 tiles
  two_tile    7 rows of 19 tiles: ceil(n_tiles / 12) = 12, 8 workgroups of 17 tiles (the regime of the older tests, forced)
  few_blocks  3 rows of 19 tiles: 5 workgroups, no XCD remap
  boundary    40 rows of (6 k + 5) hop + 200 + d samples, d in {-1, 0, 1}: whether the last interior tile is staged

n_frames % 6 cycles through {0, 1, 5}; layouts: contiguous and 16-byte aligned, a row-strided view with an aligned start (rows
staged, row_stride != length), a misaligned start (every tile through gather_global).  Every case runs `long` plus two more
regimes (test_draws_cover_the_gaps lists what the 44 cases pin).

Reference: the stored waveform widened EXACTLY to float64 (int16 x 2^-15, half.double()), torch.stft in float64 on the device
with the module's own window, |X|^2 x the normalisation, x fb.double(); oracle.torch_cpu_ref.amplitude_to_db and the DCT for
MFCC; pipelines.piecewise_linear_log and the statistics in float64 for MEL_NORM -- the construction of tests/test_gpu_fuzz.py.

Bars (none is new, none is derived from the product's output):
  linear outputs   2e-5 peak-relative (test_fuzz_melspectrogram_and_mfcc_vs_aten) -- PER WAVEFORM ROW against that row's own
                   peak: rows carry gains 1, 1e-3, 1e-3, 1, 1e-2, 1e-2, 1 and a whole-tensor peak lets a mis-addressed tile in a
                   quiet row pass (test_bite_whole_tensor_metric_misses_a_quiet_row).  The error is scale-invariant.
  MFCC             2e-3 * max(1, |ref|max / 80) absolute, the same test's bar for dB / cepstral features
  MEL_NORM         the rule of tests/test_gpu_parity.py::_assert_rnnt_features_close
  half / bfloat16  module output within one rounding of the checked float32 output (test_low_precision._within_one_rounding)
A failure names (row, tile in row, global tile, mirrored workgroup and hardware block, position in the run, staged or not) of
the worst element.

Two things the issue's examples did not foresee, kept as cases: the 80-mel banks with f_min = 20 and with sample_rate 22 050
HAVE the table signature 0x4221 of the HTK bank (the signature is the four rounds' chunk counts), so at hop 160 they run the
kSigHtk80 instantiation with OTHER weights ("mel-htk80sig-fmin20"); f_min = 300 (0x3221) is the 80-mel bank with neither
signature.

Device-free tests: the draws' coverage, the share of frames under the top_db cut-off in the MFCC draws (from the reference
alone), and bite tests with oracle/dsp_oracle.py: the float32-rounded reference passes the per-row bar, four plausible
addressing faults miss it by >= 10 x (BITE_MEASURED).

Measured on an MI355X (256 CUs): MEASURED_DEVICE; wall time of the whole file FILE_SECONDS.  No case found the kernel wrong.
That the DEVICE cases bite, beyond the device-free bite tests, was checked once by hand with a library built from a deliberately
wrong tile_next (the carry loop not advancing `in_off` when it enters a row whose number is a multiple of 64 -- an in-bounds
read of the previous row's samples): every `long` run of the float cases tried (mel-htk80-h160, its scalar twin, mel-23-h100,
mel-128-h160) failed with err / bar > 1e10; three named row 64, tile 0 in the row, global tile 1 216, workgroup 32, position 32
of a run of 37 -- the first tile a wave reaches by the carry across that row boundary -- and the fourth a tile of row 449 at
position 33 of its run, one row after such a boundary (the offset stays one row behind for the rest of the wave's run).
"""
import math
import warnings

import numpy as np
import pytest
import torch

FRAMES_PER_TILE, WAVES_PER_BLOCK, CARRY_MIN_TILES = 6, 12, 16      # csrc/melspec400.h kFramesPerWave, kWavesPerBlock, kCarryMinTiles
N_FFT, PAD = 400, 200
SIG_HTK80, SIG_SLANEY80 = 0x4221, 0x4211                           # csrc/melspec400.h kSigHtk80, kSigSlaney80
CU_DESIGN = 256
LINEAR_BAR = 2e-5

# measured on an MI355X (256 CUs), one run of this file (44 cases, 186 figures, all passed): family -> (worst err / bar, its case,
# regime, layout), from the "[fuzz-mel400]" lines (run with -s)
MEASURED_DEVICE = {"MEL": (0.020, "mel-40-h200", "short", "strided"), "SPEC": (0.020, "spec-p1.0-h100", "short", "contiguous"),
                   "MFCC": (0.048, "mfcc-fused-16-h160-3d", "long", "misaligned"),
                   "MEL_DB": (0.048, "meldb-80x13-h160-3d", "long", "contiguous"),
                   "MEL_NORM": (0.013, "rnnt-float-80-h160", "short", "misaligned"),
                   "MEL_NORM strong": (0.077, "rnnt-int16-80-h160", "short", "strided"),
                   "MEL pcm": (0.016, "pcm-int16-128-h160", "short", "misaligned"),
                   "MEL lowp": (0.015, "f16-80-h160", "short", "contiguous")}
# the 44 device cases together: 18.1 s of pytest wall time (0.5 s a case, 2.3 s for the first, which loads the library) -- 4.7 % on
# top of the 386 s the device suite took without them (404 s with them, 1 226 tests)
FILE_SECONDS = 18.1


# --------------------------------------------------------------------------- #
# 1. the host mirror of the launch arithmetic                                 #
# --------------------------------------------------------------------------- #

def launch_split(rows, length, hop, cu_count, aligned=True):
    """csrc/mel400_launch.h launch_fft400_nr + the `tin_hi` block of melspec400_kernel, for `rows` rows of `length` samples
    (stereo: rows = clips * 2, length in sample times).  `aligned`: the launch's in_aligned (16-byte base and row stride)."""
    n_frames = 1 + length // hop                                   # centre, reflect, pad = 0
    tiles_per_row = -(-n_frames // FRAMES_PER_TILE)
    n_tiles = rows * tiles_per_row
    need = -(-n_tiles // WAVES_PER_BLOCK)
    blocks = min(cu_count, need)
    if blocks >= 8:
        blocks -= blocks % 8
    blocks = max(blocks, 1)
    tiles_per_block = -(-n_tiles // blocks)
    tin_hi = 0
    if aligned and length >= N_FFT - PAD:
        last = min((length - (N_FFT - PAD)) // hop - (FRAMES_PER_TILE - 1), n_frames - FRAMES_PER_TILE)
        if last >= FRAMES_PER_TILE:
            tin_hi = last // FRAMES_PER_TILE
    return dict(rows=rows, length=length, hop=hop, n_frames=n_frames, tiles_per_row=tiles_per_row, n_tiles=n_tiles, need=need,
                blocks=blocks, tiles_per_block=tiles_per_block, tin_hi=tin_hi)


def locate(s, row, frame):
    """Where the launch computes (row, frame): tile in row, global tile, the workgroup's number after the XCD remap (`lb`), the
    hardware block that carries it, the tile's position in that workgroup's run."""
    tin = frame // FRAMES_PER_TILE
    t = row * s["tiles_per_row"] + tin
    lb, pos = divmod(t, s["tiles_per_block"])
    nb = s["blocks"]
    block = (lb % (nb >> 3)) * 8 + lb // (nb >> 3) if nb % 8 == 0 else lb
    return dict(row=row, frame=frame, tile_in_row=tin, tile=t, workgroup=lb, hw_block=block, pos_in_run=pos,
                run_length=s["tiles_per_block"], staged=1 <= tin <= s["tin_hi"])


def in_regime(name, s, k=None, d=None):
    """The condition a run of regime `name` asserts on the mirror's split."""
    long_run = s["tiles_per_block"] >= 36
    if name == "long":
        return long_run and s["tiles_per_row"] >= CARRY_MIN_TILES and s["rows"] > 1 and s["tiles_per_block"] % s["tiles_per_row"] != 0
    if name == "short":
        return long_run and 2 <= s["tiles_per_row"] < CARRY_MIN_TILES and s["tiles_per_block"] % s["tiles_per_row"] != 0
    if name == "one":
        return long_run and s["rows"] == 1 and s["tiles_per_row"] >= CARRY_MIN_TILES
    if name == "two_tile":
        return 9 <= s["need"] <= 15 and s["blocks"] == 8 and 13 <= s["tiles_per_block"] <= 23
    if name == "few_blocks":
        return s["blocks"] < 8
    if name == "boundary":            # tin_hi = k from d = 0 on, k - 1 one sample earlier
        return s["rows"] >= 16 and s["blocks"] % 8 == 0 and s["tin_hi"] == (k if d >= 0 else k - 1)
    raise KeyError(name)


# --------------------------------------------------------------------------- #
# 2. the cases and their draws                                                #
# --------------------------------------------------------------------------- #

def _bank(n_mels=80, sr=16000, f_min=0.0, norm=None, mel_scale="htk"):
    return dict(n_mels=n_mels, sr=sr, f_min=f_min, norm=norm, mel_scale=mel_scale)


HTK80, SLANEY80 = _bank(), _bank(norm="slaney", mel_scale="slaney")


def _c(cid, epi, hop, tin="float", bank=None, **kw):
    return dict(id=cid, epi=epi, hop=hop, tin=tin, bank=bank, **kw)


CASES = [
    # float MEL: the banks
    _c("mel-htk80-h160", "MEL", 160, bank=HTK80),
    _c("mel-htk80-h160-scalar", "MEL", 160, bank=HTK80, scalar=True),
    _c("mel-slaney80-h160", "MEL", 160, bank=SLANEY80),
    _c("mel-80-fmin300-h160", "MEL", 160, bank=_bank(f_min=300.0)),
    _c("mel-htk80sig-fmin20-h160", "MEL", 160, bank=_bank(f_min=20.0)),
    _c("mel-80-sr22050-h200", "MEL", 200, bank=_bank(sr=22050)),
    _c("mel-htk80-h100", "MEL", 100, bank=HTK80),
    _c("mel-htk80-h200", "MEL", 200, bank=HTK80),
    _c("mel-23-h100", "MEL", 100, bank=_bank(23)),
    _c("mel-40-h200", "MEL", 200, bank=_bank(40)),
    _c("mel-128-h160", "MEL", 160, bank=_bank(128)),
    _c("mel-160-h200", "MEL", 200, bank=_bank(160)),
    _c("mel-128-h100", "MEL", 100, bank=_bank(128)),
    _c("mel-80-hamming320-normalized-h160", "MEL", 160, bank=HTK80, win_length=320, hamming=True, normalized=True),
    # SPEC
    *[_c(f"spec-p{p}-h{h}", "SPEC", h, power=p) for h in (100, 160, 200) for p in (2.0, 1.0, None)],
    # MFCC: the fused kernel + fix-up launch (80 mels, n_mfcc % 4 == 0); (B, L) = one cut-off, (B, 1, L) = one per item
    _c("mfcc-fused-4-h100-2d", "MFCC", 100, bank=HTK80, n_mfcc=4, fused=True, lead3d=False),
    _c("mfcc-fused-16-h160-3d", "MFCC", 160, bank=HTK80, n_mfcc=16, fused=True, lead3d=True),
    _c("mfcc-fused-40-h200-2d", "MFCC", 200, bank=SLANEY80, n_mfcc=40, fused=True, lead3d=False),
    _c("mfcc-fused-40-h160-2d", "MFCC", 160, bank=SLANEY80, n_mfcc=40, fused=True, lead3d=False),
    # MEL_DB: the two-kernel path (n_mfcc = 13 is not served by the fused kernel, nor are 40 mels)
    _c("meldb-80x13-h160-3d", "MEL_DB", 160, bank=HTK80, n_mfcc=13, fused="auto", lead3d=True),
    _c("meldb-40x20-h200-2d", "MEL_DB", 200, bank=_bank(40), n_mfcc=20, fused="auto", lead3d=False),
    _c("meldb-40x13-h100-2d", "MEL_DB", 100, bank=_bank(40), n_mfcc=13, fused="auto", lead3d=False),
    # MEL_NORM: RNNTFeatureExtractor
    _c("rnnt-float-80-h160", "MEL_NORM", 160, bank=HTK80),
    _c("rnnt-float-80-h200", "MEL_NORM", 200, bank=HTK80),
    _c("rnnt-int16-80-h160", "MEL_NORM", 160, "int16", HTK80),
    _c("rnnt-int16-128-h200", "MEL_NORM", 200, "int16", _bank(128)),
    _c("rnnt-stereo-80-h160", "MEL_NORM", 160, "stereo", HTK80, others=0),
    _c("rnnt-stereo-128-h200", "MEL_NORM", 200, "stereo", _bank(128), others=2),
    # plain mel from PCM: the C entry with mean == NULL (no Python wrapper)
    _c("pcm-int16-80-h200", "MEL", 200, "int16", HTK80),
    _c("pcm-int16-128-h160", "MEL", 160, "int16", _bank(128)),
    _c("pcm-stereo-80-h200", "MEL", 200, "stereo", HTK80, others=4),
    _c("pcm-stereo-160-h160", "MEL", 160, "stereo", _bank(160), others=0),
    # half / bfloat16: F._melspectrogram_lowp (float32 out) and the module
    _c("f16-80-h160", "MEL", 160, "f16", HTK80),
    _c("f16-128-h200", "MEL", 200, "f16", _bank(128)),
    _c("bf16-80-h200", "MEL", 200, "bf16", SLANEY80, others=1),
    _c("bf16-128-h160", "MEL", 160, "bf16", _bank(128)),
]
CASE_IDS = [c["id"] for c in CASES]
LAYOUTS = ("contiguous", "strided", "misaligned")
# the two regimes a case runs besides `long`, by case index % 5 (or the case's own `others`)
OTHERS = (("short", "two_tile"), ("one", "boundary"), ("short", "few_blocks"), ("one", "two_tile"), ("short", "boundary"))
FRAMES_MOD = {0: 0, 1: 5, 5: 1}       # n_frames % 6 -> frames missing from the row's last tile
BOUNDARY_K = 4
SEED_BASE = 40400                     # disjoint from the other fuzz files' bases


def _rows_frames(regime, variant):
    """(rows, n_frames) of a regime for CU_DESIGN CUs; `variant` picks n_frames % 6 and the short rows' tile count."""
    short = FRAMES_MOD[(0, 1, 5)[variant % 3]]
    if regime == "long":
        return 490, 19 * 6 - short
    if regime == "short":
        tpr = (2, 5, 15)[(variant // 3) % 3]
        return -(-9300 // tpr), tpr * 6 - short
    if regime == "one":
        return 1, 9234 * 6 - short
    if regime == "two_tile":
        return 7, 19 * 6 - short
    if regime == "few_blocks":
        return 3, 19 * 6 - short
    raise KeyError(regime)


def _draw_runs(idx):
    """The runs of case `idx`, a function of the index alone: dict(regime, layout, rows, length, seed[, k, d])."""
    case = CASES[idx]
    hop = case["hop"]
    runs = []

    def add(regime, j):
        variant = idx + j
        layout = LAYOUTS[(idx + idx // 3 + j) % 3]
        if regime == "boundary":
            for d in (-1, 0, 1):      # always the strided view: an aligned start whatever the length
                runs.append(dict(regime=regime, layout="strided", rows=40, k=BOUNDARY_K, d=d,
                                 length=(6 * BOUNDARY_K + 5) * hop + 200 + d, seed=SEED_BASE + 100 * idx + 10 * j + d + 1))
            return
        rows, n_frames = _rows_frames(regime, variant)
        if case["tin"] == "stereo":
            rows += rows % 2          # (clip, channel) pairs
        length = (n_frames - 1) * hop + 8 * (1 + variant % 5)       # a multiple of 8: a contiguous batch is 16-byte aligned
        runs.append(dict(regime=regime, layout=layout, rows=rows, length=length, seed=SEED_BASE + 100 * idx + 10 * j))

    add("long", 0)
    for j, regime in enumerate(OTHERS[case.get("others", idx % 5)]):
        add(regime, j + 1)
    return runs


def _elem_bytes(tin):
    return {"float": 4, "stereo": 4}.get(tin, 2)


def _run_split(case, run, cu_count, aligned=None):
    if aligned is None:               # what the layout gives by construction (the device test asserts it on the pointers)
        aligned = run["layout"] != "misaligned"
        if run["layout"] == "contiguous" and run["rows"] > 1:
            aligned = run["length"] % (16 // _elem_bytes(case["tin"])) == 0
    return launch_split(run["rows"], run["length"], case["hop"], cu_count, aligned)


def _filterbank(bank):
    from audio_amd import _host
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")       # 160 bands on 201 bins leave empty bands: part of the case
        return _host.melscale_fbanks(N_FFT // 2 + 1, bank["f_min"], float(bank["sr"] // 2), bank["n_mels"], bank["sr"],
                                     bank["norm"], bank["mel_scale"])


def _table_sig(bank):
    """aamd_mel_bands.table_sig as the host computes it (the chunk counts do not depend on the layout search's length)."""
    from audio_amd import _host
    lo, width, weights, max_width = _host.mel_band_table(_filterbank(bank).numpy())
    image, _ = _host.mel400_table_image(lo, width, weights, max_width, iters=1)
    return _host.mel400_table_signature(image, bank["n_mels"], max_width)


def instantiation(case):
    """(EPI, H, TIn, NR, SIG, AR) as launch_fft400 / launch_fft400_h / launch_fft400_nr choose them."""
    epi, hop, tin, bank = case["epi"], case["hop"], case["tin"], case["bank"]
    if epi == "SPEC":
        return (epi, hop // 20, tin, 8, 0, "legacy")
    nr = 4 if bank["n_mels"] <= 80 else 8
    sig, ar = 0, "legacy"
    if nr == 4 and hop == 160 and tin == "float" and epi in ("MEL", "MFCC") and bank["n_mels"] == 80:
        s = _table_sig(bank)
        if s in (SIG_HTK80, SIG_SLANEY80):
            sig = s
        if sig == SIG_HTK80 and epi == "MEL":
            ar = "scalar" if case.get("scalar") else "packed"
    return (epi, hop // 20, tin, nr, sig, ar)


# --------------------------------------------------------------------------- #
# 3. waveforms                                                                #
# --------------------------------------------------------------------------- #

GAINS = (1.0, 1e-3, 1e-3, 1.0, 1e-2, 1e-2, 1.0)
N_BASE = 11_400_000
_BASE = []


def _noise(n, seed):
    """n samples of ONE seeded noise buffer from a seed-dependent offset: generated once per process, shared by every run."""
    if not _BASE:
        _BASE.append(torch.randn(N_BASE + 65536, generator=torch.Generator().manual_seed(SEED_BASE)))
    assert n <= N_BASE, n
    off = (seed * 7919) % 65536
    return _BASE[0][off:off + n]


def _wave(rows, length, seed, silence=False):
    """float32 (rows, length): clipped noise at 0.5, row r times GAINS[r % 7] (a quiet PAIR, so that a tile taken from the
    neighbouring row can stay under a whole-tensor bar); `silence`: two rows in seven, both of gain 1 (the silence of a 1e-3 row
    is not 80 dB under that row's own peak), are digitally silent from a quarter of their length on, a single row in 16 passages
    of 1 / 128 of its length each."""
    x = (0.5 * _noise(rows * length, seed)).clamp_(-1, 1).view(rows, length)
    if rows > 1:
        x *= torch.tensor([GAINS[r % len(GAINS)] for r in range(rows)])[:, None]
        if silence:
            x[[r for r in range(rows) if r % len(GAINS) in (0, 3)], length // 4:] = 0.0
    elif silence:
        for k in range(16):
            a = k * (length // 16) + length // 64
            x[0, a:a + length // 128] = 0.0
    return x


def _store(x, tin):
    """The waveform as the input type stores it (CPU, planar rows), and the factor that widens it exactly."""
    if tin == "float":
        return x, 1.0
    if tin in ("int16", "stereo"):
        pcm = (x * 30000.0).round().to(torch.int16)
        if x.shape[0] >= 4:           # full scale in two rows of gain 1
            pcm[0, :50] = 32767
            pcm[3, -7:] = -32768
        return pcm, 1.0 / 32768.0
    return x.to(torch.float16 if tin == "f16" else torch.bfloat16), 1.0


def _layout(q, layout, step=1):
    """The same values on the device: contiguous, a row-strided view with an aligned start, or `step` elements past a 16-byte
    boundary."""
    rows, n = q.shape
    if layout == "contiguous":
        v = q.cuda()
    elif layout == "strided":
        buf = torch.zeros(rows, (n + 15) // 8 * 8 + 8, dtype=q.dtype, device="cuda")
        v = buf[:, :n]
        v.copy_(q)
        assert v.stride(0) != n and v.stride(0) % 8 == 0
    else:
        flat = torch.zeros(rows * n + 16, dtype=q.dtype, device="cuda")
        v = flat[step:step + rows * n].view(rows, n)
        v.copy_(q)
        assert v.data_ptr() % 16 != 0 and v.is_contiguous()
    assert layout == "misaligned" or v.data_ptr() % 16 == 0
    return v


# --------------------------------------------------------------------------- #
# 4. the reference and the checks (torch, on whatever device the tensors are) #
# --------------------------------------------------------------------------- #

SLAB_FRAMES = 20000


def _window64(case, device):
    wl = case.get("win_length", N_FFT)
    w = torch.hamming_window(wl, dtype=torch.float64) if case.get("hamming") else torch.hann_window(wl, dtype=torch.float64)
    return w.to(device)


def _spectrum64(x64, w64, hop, normalized=False):
    """(rows, L) float64 -> complex (rows, T, 201): torch.stft with the window as given (aten pads it to n_fft, centred)."""
    X = torch.stft(x64, N_FFT, hop, w64.shape[0], w64, True, "reflect", False, True, return_complex=True).transpose(1, 2)
    return X / w64.pow(2).sum().sqrt() if normalized else X


def _slabs(rows, n_frames):
    step = max(1, SLAB_FRAMES // n_frames)
    return [(a, min(rows, a + step)) for a in range(0, rows, step)]


def _mel64(x64, w64, hop, fb64, normalized=False):
    """(rows, T, n_mels) float64, the float64 spectrum held one slab of rows at a time."""
    n_frames = 1 + x64.shape[1] // hop
    return torch.cat([_spectrum64(x64[a:b], w64, hop, normalized).abs().pow(2) @ fb64 for a, b in _slabs(x64.shape[0], n_frames)])


def row_errors(got, ref):
    """got, ref: (rows, T, C) -> per row max|got - ref| / max|ref of that row|, and the frame of each row's worst element."""
    if ref.is_complex():
        got, ref = torch.view_as_real(got).flatten(2), torch.view_as_real(ref).flatten(2)
    d = (got.double() - ref).abs().flatten(1)
    e, where = d.max(1)
    peak = ref.abs().flatten(1).amax(1)
    rel = torch.where(peak > 0, e / peak.clamp_min(1e-300), e)
    return rel, where // ref.shape[2]


def whole_tensor_error(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max())


class _Rows:
    """Per-row errors of one run, gathered slab by slab."""

    def __init__(self):
        self.rel, self.frame = [], []

    def add(self, got, ref):
        rel, frame = row_errors(got, ref)
        self.rel.append(rel)
        self.frame.append(frame)

    def worst(self):
        rel, frame = torch.cat(self.rel), torch.cat(self.frame)
        r = int(rel.argmax())
        return float(rel[r]), r, int(frame[r])


_WORST = {}


def _note(family, cid, run, what, err, bar, where):
    ratio = err / bar
    _WORST[family] = max(_WORST.get(family, 0.0), ratio)
    print(f"[fuzz-mel400] {family} {cid} {run['regime']}/{run['layout']} rows={run['rows']} L={run['length']} {what}: "
          f"err={err:.3e} bar={bar:.3e} err/bar={ratio:.3f} (worst so far {_WORST[family]:.3f}) at {where}")


def assert_rows_close(rows_or_pair, s, family, cid, run, what, bar=LINEAR_BAR):
    """The linear bar, per waveform row against that row's own peak."""
    if not isinstance(rows_or_pair, _Rows):
        acc = _Rows()
        acc.add(*rows_or_pair)
        rows_or_pair = acc
    err, r, f = rows_or_pair.worst()
    where = locate(s, r, f)
    _note(family, cid, run, what, err, bar, where)
    assert err <= bar, (cid, run, what, err, bar, where, s)


def _assert_abs_close(got, ref, bar, s, family, cid, run, what):
    d = (got.double() - ref).abs()
    i = int(d.argmax())
    r, f = i // (ref.shape[1] * ref.shape[2]), i // ref.shape[2] % ref.shape[1]
    where = locate(s, r, f)
    _note(family, cid, run, what, float(d.max()), bar, where)
    assert float(d.max()) <= bar, (cid, run, what, float(d.max()), bar, where, s)


def rnnt_reference(mel64, mean, invstd):
    """((plog(mel * GAIN) - mean) * invstddev, the element-wise bar, the elements within 0.5 % of plog's two break points, the
    well-conditioned elements) -- tests/test_gpu_parity.py::_assert_rnnt_features_close for any hop and batch."""
    from audio_amd.pipelines import GAIN, piecewise_linear_log
    y = mel64 * GAIN
    ref = (piecewise_linear_log(y) - mean) * invstd
    e, ee = math.e, math.e ** math.e
    ye = y.clamp_min(e)
    dplog = torch.where(y <= e, torch.full_like(y, 1.0 / e), torch.where(y <= ee, 1.0 / (ye * e), 1.0 / ye))
    peak = mel64.amax(-1, keepdim=True)
    tol = 2e-4 + invstd * GAIN * dplog * 2e-6 * peak
    near = ((y / e - 1).abs() < 5e-3) | ((y / ee - 1).abs() < 5e-3)
    strong = (mel64 > 1e-5 * peak) & ~near
    return ref, tol, near, strong


def _assert_rnnt_close(got, mel64, mean, invstd, s, cid, run, what):
    T = mel64.shape[1]
    assert got.shape[1] >= T and not bool(got[:, T:].any()), (cid, run, "right padding")
    ref, tol, near, strong = rnnt_reference(mel64, mean, invstd)
    d = (got[:, :T].double() - ref).abs()
    ratio = torch.where(near, torch.zeros_like(d), d / tol)
    i = int(ratio.argmax())
    where = locate(s, i // (T * ref.shape[2]), i // ref.shape[2] % T)
    _note("MEL_NORM", cid, run, what, float(ratio.max()), 1.0, where)
    assert float(ratio.max()) <= 1.0, (cid, run, what, float(ratio.max()), where, s)
    ds = torch.where(strong, d, torch.zeros_like(d))
    i = int(ds.argmax())
    where = locate(s, i // (T * ref.shape[2]), i // ref.shape[2] % T)
    _note("MEL_NORM strong", cid, run, what, float(ds.max()), 2e-4, where)
    assert float(ds.max()) <= 2e-4, (cid, run, what, float(ds.max()), where, s)


def silence_share(mel64, per_item):
    """(share of frames whose every band lies under the top_db = 80 cut-off, share of elements under it), from the float64 mel
    spectrogram (rows, T, n_mels) alone; one cut-off for the batch or one per row."""
    db = 10.0 * torch.log10(mel64.clamp_min(1e-10))
    top = db.amax(dim=(1, 2), keepdim=True) if per_item else db.amax()
    under = db < top - 80.0
    return float(under.all(-1).double().mean()), float(under.double().mean())


SHARE_RANGE = (0.08, 0.30)


def mfcc_reference(mel64, dct64, lead3d):
    from oracle import torch_cpu_ref as R
    m = mel64.transpose(1, 2)                 # (B, n_mels, T): one cut-off; (B, 1, n_mels, T): one per item
    db = R.amplitude_to_db(m[:, None] if lead3d else m)
    return db.reshape(m.shape).transpose(1, 2) @ dct64


# --------------------------------------------------------------------------- #
# 5. the device tests                                                         #
# --------------------------------------------------------------------------- #

@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from audio_amd import _lib
    _lib.lib()
    return torch.device("cuda", 0)


def _mel_kwargs(case):
    b = case["bank"]
    kw = dict(sample_rate=b["sr"], n_fft=N_FFT, hop_length=case["hop"], n_mels=b["n_mels"], f_min=b["f_min"], norm=b["norm"],
              mel_scale=b["mel_scale"])
    if case.get("win_length"):
        kw.update(win_length=case["win_length"], window_fn=torch.hamming_window if case.get("hamming") else torch.hann_window,
                  normalized=bool(case.get("normalized")))
    return kw


def _stats(n_mels):
    g = torch.Generator().manual_seed(n_mels)
    return dict(mean=(5.0 + 10.0 * torch.rand(n_mels, generator=g)).tolist(),
                invstddev=(0.2 + 0.3 * torch.rand(n_mels, generator=g)).tolist())


def _pcm_plain_mel(v, mel, chans):
    """aamd_melspectrogram_pcm16_f32 / _interleaved_f32 with mean == NULL: the plain mel spectrogram of int16 PCM, frame-major
    (rows, T, n_mels).  v: (rows, L) int16, or (clips, T, 2); a row stride is passed on as it is."""
    import ctypes as C
    import audio_amd.functional as F
    from audio_amd import _lib
    sp, d = mel.spectrogram, v.device
    window = sp.window.to(device=d, dtype=torch.float32)
    if chans == 2:
        clips, n_time = v.shape[0], v.shape[1]
        probe = torch.empty((2 * clips, n_time), dtype=torch.float32, device="meta")
        desc = F._stft_desc(probe, 0, window, N_FFT, sp.hop_length, 2.0, False, True, "reflect", True)
        assert v.stride(2) == 1 and v.stride(1) == 2 and v.stride(0) % 2 == 0 and v.data_ptr() % 4 == 0
        desc.row_stride = v.stride(0) // 2 if clips > 1 else n_time
    else:
        desc = F._stft_desc(v, 0, window, N_FFT, sp.hop_length, 2.0, False, True, "reflect", True)
    desc.scale = desc.scale / 32768.0
    bands = F._mel_bands(mel.mel_scale.fb, d)
    out = torch.empty((desc.rows, desc.n_frames, bands.n_mels), dtype=torch.float32, device=d)
    L = _lib.lib()
    tail = (F._padded_window(window, N_FFT).data_ptr(), F._twiddles(N_FFT, d).data_ptr(), C.byref(bands.struct), out.data_ptr(),
            C.byref(desc), 1.0, None, None, 0, _lib.current_stream(d))
    with torch.cuda.device(d):
        if chans == 2:
            _lib.check(L.aamd_melspectrogram_pcm16_interleaved_f32(v.data_ptr(), 2, *tail))
        else:
            _lib.check(L.aamd_melspectrogram_pcm16_f32(v.data_ptr(), *tail))
    return out


def _frame_major(y, rows):
    """A module's (..., C, T) output as (rows, T, C)."""
    return y.reshape((rows,) + tuple(y.shape[-2:])).transpose(1, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(len(CASES)), ids=CASE_IDS)
def test_fuzz_mel400_instantiations_in_long_runs_vs_float64(idx, dev):
    import audio_amd.functional as F
    import audio_amd.transforms as T
    from audio_amd import _lib
    from audio_amd.pipelines import RNNTFeatureExtractor
    from test_low_precision import _within_one_rounding
    case = CASES[idx]
    epi, hop, tin, bank = case["epi"], case["hop"], case["tin"], case["bank"]
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    inst = instantiation(case)
    # the modules of this case, and that the launch takes the instantiation the case is listed for
    mel = fe = mod = None
    if epi == "SPEC":
        mod = T.Spectrogram(n_fft=N_FFT, hop_length=hop, power=case["power"]).cuda()
    elif epi in ("MFCC", "MEL_DB"):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            mod = T.MFCC(sample_rate=bank["sr"], n_mfcc=case["n_mfcc"], melkwargs={k: v for k, v in _mel_kwargs(case).items()
                                                                                   if k != "sample_rate"}).cuda()
        mod.fused = case["fused"]
        mel = mod.MelSpectrogram
    elif epi == "MEL_NORM":
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            fe = RNNTFeatureExtractor(_stats(bank["n_mels"]), sample_rate=bank["sr"], n_mels=bank["n_mels"], hop_length=hop).cuda()
        mel = fe.mel
    else:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            mel = T.MelSpectrogram(**_mel_kwargs(case)).cuda()
    if mel is not None:
        assert torch.equal(mel.mel_scale.fb.cpu(), _filterbank(bank)), case
        bands = F._mel_bands(mel.mel_scale.fb, dev)
        assert bands.n_mels <= 160 and bands.max_width <= 62, case       # served by the n_fft = 400 kernel
        want_sig = _table_sig(bank)
        assert int(bands.table_sig) == want_sig, (case, hex(int(bands.table_sig)), hex(want_sig))
        assert inst[4] in (0, want_sig)
        fb64 = mel.mel_scale.fb.double()
    w64 = (mod if epi == "SPEC" else mel.spectrogram).window.double()       # the module's own window
    assert w64.shape[0] == case.get("win_length", N_FFT) and float((w64.cpu() - _window64(case, "cpu")).abs().max()) < 1e-6
    normalized = bool(case.get("normalized"))
    chans = 2 if tin == "stereo" else 1

    for run in _draw_runs(idx):
        rows, length = run["rows"], run["length"]
        x = _wave(rows, length, run["seed"], silence=epi in ("MFCC", "MEL_DB"))
        q, widen = _store(x, tin)
        if chans == 2:                # rows (clip, channel) -> interleaved (clips, time * 2)
            q = q.view(rows // 2, 2, length).transpose(1, 2).reshape(rows // 2, 2 * length)
        v = _layout(q, run["layout"], step=2 if chans == 2 else 1)
        assert torch.equal(v.cpu(), q)
        elems16 = 16 // v.element_size()
        aligned = v.data_ptr() % 16 == 0 and (v.stride(0) if v.shape[0] > 1 else v.shape[1]) % elems16 == 0
        assert aligned == (run["layout"] != "misaligned"), (case, run)
        s = launch_split(rows, length, hop, cu, aligned)
        assert in_regime(run["regime"], s, run.get("k"), run.get("d")), (case["id"], run, s, f"{cu} CUs")
        assert (s["tin_hi"] > 0) == (aligned and s["n_frames"] >= 2 * FRAMES_PER_TILE), (run, s)      # rows with an interior tile
        T_ = s["n_frames"]
        if chans == 2:
            v3 = v.unflatten(1, (length, 2))
            x64 = v3.permute(0, 2, 1).reshape(rows, length).double() * widen
        else:
            x64 = v.double() * widen
        what = f"inst={inst}"

        with torch.no_grad():
            if epi == "SPEC":
                got = _frame_major(mod(v), rows)
                assert got.shape == (rows, T_, 201), (got.shape, s)
                acc = _Rows()
                for a, b in _slabs(rows, T_):
                    X = _spectrum64(x64[a:b], w64, hop)
                    if case["power"] is None:
                        acc.add(got[a:b], X)
                    else:             # in the power-spectrum domain, as tests/test_gpu_fuzz.py compares
                        acc.add(got[a:b].double().pow(2.0 / case["power"]), X.abs().pow(2))
                assert_rows_close(acc, s, "SPEC", case["id"], run, what)
                continue

            m64 = _mel64(x64, w64, hop, fb64, normalized)
            assert m64.shape == (rows, T_, bank["n_mels"])

            if epi in ("MFCC", "MEL_DB"):
                xin = v[:, None] if case["lead3d"] else v
                got = _frame_major(mod(xin), rows)
                rep = mod.fused_report()
                assert rep["path"] == ("fused" if epi == "MFCC" else "two-kernel"), (case, rep)
                assert got.shape == (rows, T_, case["n_mfcc"]), (got.shape, s)
                ref = mfcc_reference(m64, mod.dct_mat.double(), case["lead3d"])
                share = silence_share(m64, case["lead3d"])
                print(f"[fuzz-mel400] {case['id']} {run['regime']}: frames under the cut-off {share[0]:.3f}, elements "
                      f"{share[1]:.3f}, fix-up share {rep['redone_share']}")
                assert SHARE_RANGE[0] <= share[0] <= SHARE_RANGE[1], share
                _assert_abs_close(got, ref, 2e-3 * max(1.0, float(ref.abs().max()) / 80.0), s, epi, case["id"], run, what)
            elif epi == "MEL_NORM":
                if chans == 2:
                    if run["layout"] == "strided":       # (features() copies a strided interleaved batch: the launch sees it contiguous)
                        assert not v3.is_contiguous()
                    got = fe.features(v3, channels_first=False).reshape(rows, T_ + fe.right_padding, bank["n_mels"])
                else:
                    got = fe(v)
                assert got.shape == (rows, T_ + fe.right_padding, bank["n_mels"]), (got.shape, s)
                _assert_rnnt_close(got, m64, fe.mean.double(), fe.invstddev.double(), s, case["id"], run, what)
            elif tin in ("int16", "stereo"):
                got = _pcm_plain_mel(v3 if chans == 2 else v, mel, chans)
                assert got.shape == m64.shape, (got.shape, s)
                assert_rows_close((got, m64), s, "MEL pcm", case["id"], run, what)
            elif tin in ("f16", "bf16"):
                direct = F._melspectrogram_lowp(v, 0, mel.spectrogram.window, mel.mel_scale.fb, N_FFT, hop, N_FFT, 2.0, False,
                                                True, "reflect")
                assert direct is not None and direct.dtype == torch.float32, case      # read as stored, n_mels > 80 included
                assert direct.shape == m64.shape, (direct.shape, s)
                assert_rows_close((direct, m64), s, "MEL lowp", case["id"], run, what)
                y = mel(v)
                assert y.dtype == v.dtype
                assert _within_one_rounding(_frame_major(y, rows), direct, tin), (case, run)
            else:
                if case.get("scalar"):
                    with _lib.kernel_policy(_lib.POLICY_MEL400_SCALAR):
                        got = _frame_major(mel(v), rows)
                else:
                    got = _frame_major(mel(v), rows)
                assert got.shape == m64.shape, (got.shape, s)
                assert_rows_close((got, m64), s, "MEL", case["id"], run, what)


# --------------------------------------------------------------------------- #
# 6. no device: coverage of the draws, the silence share, bite                #
# --------------------------------------------------------------------------- #

def test_launch_split_by_hand():
    """The mirror on shapes worked out by hand from csrc/mel400_launch.h (256 CUs)."""
    s = launch_split(490, 113 * 160 + 8, 160, 256)           # 114 frames = 19 tiles; 9 310 tiles; ceil(9310 / 256) = 37
    assert (s["n_frames"], s["tiles_per_row"], s["n_tiles"], s["blocks"], s["tiles_per_block"]) == (114, 19, 9310, 256, 37)
    assert s["tin_hi"] == 17                                  # last = (18088 - 200) // 160 - 5 = 106 -> 106 // 6
    s = launch_split(7, 113 * 160 + 8, 160, 256)             # 133 tiles: need 12 -> 8 workgroups of 17
    assert (s["need"], s["blocks"], s["tiles_per_block"]) == (12, 8, 17)
    s = launch_split(3, 113 * 160 + 8, 160, 256)             # 57 tiles: 5 workgroups (no remap) of 12
    assert (s["blocks"], s["tiles_per_block"]) == (5, 12)
    s = launch_split(100, 113 * 160 + 8, 160, 256)           # 1 900 tiles: need 159 -> 152 workgroups of 13
    assert (s["blocks"], s["tiles_per_block"]) == (152, 13)
    assert launch_split(3, 5003, 160, 256, aligned=False)["tin_hi"] == 0
    # the XCD remap is a bijection, and hardware block b carries workgroup (b & 7) * (nb >> 3) + (b >> 3)
    s = launch_split(490, 113 * 160 + 8, 160, 256)
    seen = {}
    for t in range(0, s["n_tiles"], s["tiles_per_block"]):
        w = locate(s, t // s["tiles_per_row"], (t % s["tiles_per_row"]) * 6)
        assert w["tile"] == t and w["pos_in_run"] == 0
        assert (w["hw_block"] & 7) * (s["blocks"] >> 3) + (w["hw_block"] >> 3) == w["workgroup"]
        seen[w["hw_block"]] = w["workgroup"]
    assert len(seen) == -(-s["n_tiles"] // s["tiles_per_block"])


def test_draws_cover_the_gaps():
    """What the cases pin, with the mirror at 256 CUs; a change of a case or of a draw cannot silently lose one."""
    insts = {c["id"]: instantiation(c) for c in CASES}
    runs = {c["id"]: _draw_runs(i) for i, c in enumerate(CASES)}
    by_id = {c["id"]: c for c in CASES}
    splits = {cid: [(r, _run_split(by_id[cid], r, CU_DESIGN)) for r in rs] for cid, rs in runs.items()}
    assert 40 <= len(CASES) <= 48 and len(set(CASE_IDS)) == len(CASES)
    # every run is in the regime it claims; every case runs `long` and at least one other regime
    for cid, rs in splits.items():
        for r, s in rs:
            assert in_regime(r["regime"], s, r.get("k"), r.get("d")), (cid, r, s)
            assert r["length"] > N_FFT and r["rows"] * r["length"] <= N_BASE
            if by_id[cid]["tin"] == "stereo":
                assert r["rows"] % 2 == 0
        assert rs[0][0]["regime"] == "long" and len({r["regime"] for r, _ in rs}) >= 2, cid
    every = [(cid, r, s) for cid, rs in splits.items() for r, s in rs]
    # gap: every regime
    assert {r["regime"] for _, r, _ in every} == {"long", "short", "one", "two_tile", "few_blocks", "boundary"}
    # gap: every (epilogue, hop, input type) that exists
    have = {(i[0], i[1] * 20, i[2]) for i in insts.values()}
    want = {(e, h, "float") for e in ("MEL", "SPEC", "MFCC", "MEL_DB") for h in (100, 160, 200)}
    want |= {("MEL_NORM", h, t) for h in (160, 200) for t in ("float", "int16", "stereo")}
    want |= {("MEL", h, t) for h in (160, 200) for t in ("int16", "stereo", "f16", "bf16")}
    assert have == want, (sorted(want - have), sorted(have - want))
    # gap: both NR, all three SIG, both AR
    assert {i[3] for i in insts.values() if i[0] != "SPEC"} == {4, 8}
    assert {i[4] for i in insts.values()} == {0, SIG_HTK80, SIG_SLANEY80}
    assert {i[5] for i in insts.values()} == {"legacy", "packed", "scalar"}
    assert insts["mel-80-fmin300-h160"][3:5] == (4, 0) and insts["mel-htk80sig-fmin20-h160"][4] == SIG_HTK80
    assert insts["mfcc-fused-16-h160-3d"][4] == SIG_HTK80 and insts["mfcc-fused-40-h160-2d"][4] == SIG_SLANEY80
    for t in ("int16", "stereo", "f16", "bf16"):              # gap: non-float inputs with n_mels > 80
        assert {i[3] for i in insts.values() if i[2] == t} == {4, 8}, t
    assert {by_id[c]["bank"]["n_mels"] for c in by_id if by_id[c]["epi"] == "MEL" and by_id[c]["tin"] == "float"} \
        >= {23, 40, 80, 128, 160}
    assert any(c.get("hamming") and c.get("normalized") and c.get("win_length", N_FFT) < N_FFT for c in CASES)
    assert {(c["hop"], c["power"]) for c in CASES if c["epi"] == "SPEC"} == {(h, p) for h in (100, 160, 200) for p in (2.0, 1.0, None)}
    assert {(c["n_mfcc"], c["hop"]) for c in CASES if c["epi"] == "MFCC"} >= {(4, 100), (16, 160), (40, 200)}
    assert {c["lead3d"] for c in CASES if c["epi"] == "MFCC"} == {True, False} == {c["lead3d"] for c in CASES if c["epi"] == "MEL_DB"}
    # gap: n_frames % 6 in {0, 1, 5} in the long-run regimes, rows of < 16 and >= 16 tiles, runs that end inside rows
    for regime in ("long", "short", "one"):
        assert {s["n_frames"] % 6 for _, r, s in every if r["regime"] == regime} == {0, 1, 5}, regime
    assert {s["tiles_per_row"] for _, r, s in every if r["regime"] == "short"} == {2, 5, 15}
    assert all(s["tiles_per_block"] % s["tiles_per_row"] != 0 for _, r, s in every if r["regime"] in ("long", "short", "one"))
    for cid in by_id:
        if by_id[cid]["tin"] == "stereo":                     # the stereo instantiation in rows of >= 16 and of < 16 tiles
            assert {s["tiles_per_row"] >= CARRY_MIN_TILES for _, s in splits[cid]} == {True, False}, cid
    # gap: all three layouts in every long-run regime, per input type in `long`; staged and unstaged
    for regime in ("long", "short", "one"):
        assert {r["layout"] for _, r, _ in every if r["regime"] == regime} == set(LAYOUTS), regime
    for t in ("float", "int16", "stereo", "f16", "bf16"):
        lay = {r["layout"] for cid, r, _ in every if by_id[cid]["tin"] == t}
        assert lay == set(LAYOUTS), (t, lay)
    assert all(s["tin_hi"] == 0 for _, r, s in every if r["layout"] == "misaligned")
    assert all(s["tin_hi"] > 0 for _, r, s in every if r["layout"] != "misaligned" and s["tiles_per_row"] >= 3)
    # gap: both sides of tin_hi at the boundary lengths, in a many-row batch, at every hop
    for hop in (100, 160, 200):
        b = {r["d"]: s for cid, r, s in every if r["regime"] == "boundary" and by_id[cid]["hop"] == hop}
        assert sorted(b) == [-1, 0, 1] and b[-1]["tin_hi"] == BOUNDARY_K - 1 and b[0]["tin_hi"] == b[1]["tin_hi"] == BOUNDARY_K
        assert all(s["rows"] == 40 and s["tiles_per_row"] > BOUNDARY_K for s in b.values())
    assert {by_id[cid]["tin"] for cid, r, _ in every if r["regime"] == "boundary"} >= {"float", "int16", "f16", "bf16", "stereo"}
    print("[fuzz-mel400] gaps pinned: 6 regimes; (epilogue, hop, input type) x", len(want), "; NR 4 / 8 per input type; SIG 0 / "
          "0x4221 / 0x4211; AR packed / scalar; n_frames % 6 in {0, 1, 5} per long-run regime; rows of 2 / 5 / 15 / 19 / 9234 "
          "tiles; 3 layouts per long-run regime and per input type; runs ending inside rows; tin_hi = k - 1 / k at d = -1 / 0, 1")


def test_mfcc_draws_silence_share():
    """The share of frames that lie wholly under the top_db = 80 cut-off, from the float64 reference alone, for every run of the
    MFCC / MEL_DB cases: both sides of the clamp are populated, and the fix-up list of the fused kernel is long (the tiles of
    those frames, spread over two rows in seven = over every workgroup; on the device the fix-up pass redid 21 .. 56 % of the
    tiles in the many-row runs, 12.5 % in the single row).  Measured: 0.203 .. 0.213 in rows of >= 5 tiles, 0.163 in the rows of
    2 tiles, 0.245 in the batch of 3 rows, 0.124 in the single row (16 passages); asserted: SHARE_RANGE."""
    for idx, case in enumerate(CASES):
        if case["epi"] not in ("MFCC", "MEL_DB"):
            continue
        fb64, w64 = _filterbank(case["bank"]).double(), _window64(case, "cpu")
        for run in _draw_runs(idx):
            x64 = _wave(run["rows"], run["length"], run["seed"], silence=True).double()
            frames, elems = silence_share(_mel64(x64, w64, case["hop"], fb64), case["lead3d"])
            print(f"[fuzz-mel400] silence share {case['id']} {run['regime']} rows={run['rows']} L={run['length']}: "
                  f"frames {frames:.3f} elements {elems:.3f}")
            assert SHARE_RANGE[0] <= frames <= SHARE_RANGE[1], (case["id"], run, frames)
            assert elems >= frames


# (perturbed reference - reference) / bar, measured on the CPU with the shape below
BITE_MEASURED = {"float32-rounded reference": 0.0023, "tile from the neighbouring row": 3.29e4, "tile shifted by one frame": 3.53e4,
                 "first tile = last tile of the previous row": 2.81e4, "int16 sample from the wrong half-word": 904,
                 "half sample from the wrong half-word": 912, "quiet-row tile, whole-tensor metric": 0.028}
BITE_ROWS, BITE_FRAMES, BITE_HOP = 6, 19 * 6 - 1, 160


def _bite_reference(tin="float"):
    """(stored waveform widened, float64 mel spectrogram (rows, T, 80), the mirror's split) of a few_blocks-sized batch."""
    from oracle import dsp_oracle as O
    length = (BITE_FRAMES - 1) * BITE_HOP + 8
    q, widen = _store(_wave(BITE_ROWS, length, SEED_BASE + 7), tin)
    x = q.double().numpy() * widen
    fb = _filterbank(HTK80).double().numpy()
    return x, _bite_mel(x, fb), launch_split(BITE_ROWS, length, BITE_HOP, CU_DESIGN)


def _bite_mel(x, fb=None):
    from oracle import dsp_oracle as O
    fb = _filterbank(HTK80).double().numpy() if fb is None else fb
    return torch.from_numpy(np.ascontiguousarray(np.swapaxes(O.mel_spectrogram(x, O.hann_window(N_FFT), fb, N_FFT, BITE_HOP), -1, -2)))


def _bite_factor(got, ref):
    return float(row_errors(got, ref)[0].max()) / LINEAR_BAR


def test_bite_reference_rounded_to_float32_passes():
    x, ref, s = _bite_reference()
    assert ref.shape == (BITE_ROWS, s["n_frames"], 80) and s["n_frames"] == BITE_FRAMES
    f = _bite_factor(ref.float(), ref)
    print(f"[fuzz-mel400] bite: float32-rounded reference err/bar {f:.3g}")
    assert f <= 0.01
    assert_rows_close((ref.float(), ref), s, "bite", "rounded", dict(regime="few_blocks", layout="-", rows=BITE_ROWS, length=0), "-")


@pytest.mark.parametrize("fault", ["tile_from_neighbouring_row", "tile_shifted_one_frame", "first_tile_is_previous_rows_last"])
def test_bite_addressing_faults(fault):
    """One tile of six frames wrong, the way a run-boundary or row-boundary slip of the tile loop would leave it; in the QUIET row
    of the pair (gain 1e-3), so the fault is as small as the draws make it."""
    x, ref, s = _bite_reference()
    got = ref.float().clone()
    row, tin = 2, 7                   # rows 1, 2 carry the gain 1e-3
    f0 = tin * FRAMES_PER_TILE
    if fault == "tile_from_neighbouring_row":
        got[row, f0:f0 + 6] = ref[row - 1, f0:f0 + 6].float()
    elif fault == "tile_shifted_one_frame":
        got[row, f0:f0 + 6] = ref[row, f0 + 1:f0 + 7].float()
    else:
        last = (s["tiles_per_row"] - 1) * FRAMES_PER_TILE
        n = s["n_frames"] - last
        got[row, :n] = ref[row - 1, last:].float()
    f = _bite_factor(got, ref)
    print(f"[fuzz-mel400] bite {fault}: err/bar {f:.3g}")
    assert f >= 10.0, (fault, f)
    with pytest.raises(AssertionError):
        assert_rows_close((got, ref), s, "bite", fault, dict(regime="few_blocks", layout="-", rows=BITE_ROWS, length=0), "-")


@pytest.mark.parametrize("tin", ["int16", "f16"])
def test_bite_sample_from_the_wrong_half_word(tin):
    """One 16-bit sample of one staging piece replaced by its neighbour in the same 32-bit word, in a quiet row."""
    x, ref, s = _bite_reference(tin)
    bad = x.copy()
    n = 40 * BITE_HOP + 6             # an even sample at the centre of frame 40
    bad[2, n] = x[2, n + 1]
    assert bad[2, n] != x[2, n]
    f = _bite_factor(_bite_mel(bad).float(), ref)
    print(f"[fuzz-mel400] bite wrong half-word ({tin}): err/bar {f:.3g}")
    assert f >= 10.0, (tin, f)


def test_bite_whole_tensor_metric_misses_a_quiet_row():
    """Why the bar is applied per row: a tile of a 1e-3 row taken from the other 1e-3 row is 1e-6 of the batch's peak."""
    x, ref, s = _bite_reference()
    got = ref.float().clone()
    got[2, 42:48] = ref[1, 42:48].float()
    whole = whole_tensor_error(got, ref) / LINEAR_BAR
    per_row = _bite_factor(got, ref)
    print(f"[fuzz-mel400] bite quiet row: whole-tensor err/bar {whole:.3g}, per-row err/bar {per_row:.3g}")
    assert whole < 1.0 and per_row >= 10.0, (whole, per_row)
