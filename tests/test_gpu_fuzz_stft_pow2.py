"""The register-FFT STFT / ISTFT / Kaldi kernels (csrc/stft_pow2.h: p2::stft_pow2_kernel<E, EPI_SPEC | EPI_MEL>, p2::istft_pow2_kernel<E>,
p2::istft_pow2_run_kernel<E>, p2::kaldi_pow2_kernel<E, 0 | 1>, E = 4 / 8 / 16 / 32 for n_fft 256 / 512 / 1024 / 2048) and the
n_fft = 400 inverse (csrc/istft400.h: m400::istft400_kernel<5 | 8 | 10>, hop 100 / 160 / 200) -- 27 instantiations -- in MULTI-ITEM
launches against float64.

Why: the waves are persistent.  Each runs `for (item = first; item < n; item += gridDim.x * kWaves)` over frame pairs, runs of
pairs, utterance pairs or six-frame tiles, and the launchers start cu_count x {8, 8, 4, 2} workgroups of 4 waves (forward and
inverse), cu_count x 4 (Kaldi) and cu_count workgroups of 8 waves (n_fft 400): on 256 CUs a wave meets its SECOND item only beyond
8192 / 8192 / 4096 / 2048 pairs, 4096 Kaldi pairs, 2048 tiles.  The rest of the suite reaches about 60 pairs, so nothing that acts
from the second item on had run on a device: the forward's prefetch of the next pair's samples (E <= 16; another row, an interior
pair's coalesced loads handing over to an edge pair's index map and back, a pair without a frame b), the wave's LDS region rewritten
while the previous pair's epilogue reads are ordered by one wave_lds_sync, the mel table staged once, the run kernel's ring zeroed
once and relying on ring_flush to clear it, plain stores of a run next to atomics of other waves, the tile buffer of the n_fft-400
inverse re-zeroed per tile and its `exclusive` store rule, the Kaldi kernel rebasing wav / out / noise per utterance in a by-value
argument.

The host mirror (fwd_blocks, inv_plan, kaldi_blocks, inv400_blocks) restates p2::fwd_blocks / p2::inv_plan / p2::kaldi_blocks /
m400::inv_blocks; a device-free test holds it against those functions themselves (through the CPU replay) at 256, 8 and 5 CUs.
Every device case takes the CU count from the device (checked against aamd_device_info), is sized by the mirror and ASSERTS its
regime before it runs: W = waves launched, n_items >= int(2.5 W) + 3, n_items % W != 0 (every wave runs >= 2 items, some 3).  On
another device a case re-sizes or fails loudly.  Regimes:

  forward   rows of 37 frames = 19 pairs (19 does not divide W: a wave's consecutive pairs lie in different rows); the mirror shows
            interior -> edge, edge -> interior and a pair right behind a frame-b-less pair on some wave.  Per E: center + reflect with
            pad 13 and complex output; center + circular with win_length 3/4 n_fft, a hop that is no multiple of 4 and magnitudes;
            center=False with power 2.  Mel per E: 80 mels (table in LDS, tail_G > 1), 64 / 128 mels (tail_G = 1), and a bank that
            does not fit kMelLdsBytes.  The module's triangular banks stay under 32 KB at these n_fft (the 48 kHz / 24-mel bank that
            test_pow2_wave_fft_equals_generic_and_torch_stft calls wide is 888 / 1656 / 3240 / 6360 floats of 8192: it sits in LDS,
            so the global-memory walk had not run on a device), so that case sets the module's filterbank buffer to 72 bands
            of up to 160 bins; the reference uses the same buffer.
  short     inverse, rows of 5 frames = 3 pairs = one run; hop = n_fft / 2 and the natural length, the only 5-frame shape under NOLA
            whose middle pair is interior, so every run goes through the ring: n_runs multi-item
  full      inverse, rows of 33 frames: a 16-pair run and a 1-pair run per row, n_runs >= 1.25 W
  atomic    the 5-frame shape under POLICY_ISTFT_ATOMIC (istft_pow2_kernel), n_pairs multi-item
  inv400    rows of 15 frames (tiles of 6, 6, 3), n_tiles multi-item; hop 200 once with 13 frames and length 2400 = 0 (mod 1200)
  adjoint   the backward of T.Spectrogram(power=None): run kernel, n_fft-400 kernel, atomic kernel with hop > n_fft; reflect, circular
  kaldi     (n_utt, n) batches of 37-frame utterances through compliance.kaldi.spectrogram / fbank: both snip_edges, DC removal,
            raw and windowed energy, pre-emphasis 0.97, an energy column, dither 0, energy_floor 0 (the floor would hide the energy)
`length` ends inside the last frame in half of the 16 inverse cases (full on E = 4, 16; every atomic case; inv400 hop 100 and 160).

Inputs: standard normal float32 clamped to [-1, 1], row gains cycling 1, 1e-3, 1e-2, 1, one all-zero row placed where the mirror
shows it as the second or third item of a wave behind a gain-1 row; fixed seeds.  References, float64, on the device, in slabs of
at most 256 MB of complex128: torch.stft; torch.stft and a matmul with the module's own filterbank; torch.istft; float64 autograd
through torch.stft; oracle/kaldi_oracle.py per utterance.  Every output element is compared.

Bars (none new, none from the product's output): forward and mel 2e-5 (test_fuzz_spectrogram_family_vs_aten_stft), PER ROW against
the row's own reference peak, fractional powers in the power domain; inverse max(2e-5, 4 x err(aten float32 istft vs float64)) per
row (test_fuzz_inverse_spectrogram_vs_aten_istft; every row but the all-zero one has a non-zero finite reference peak, asserted);
adjoint 2e-5 per row; Kaldi kaldi_fuzz_cases.judge, unchanged; all-zero rows exactly 0.0; a second call of a forward case bit-equal.
A failure prints locate(): row, frame or sample, the owning item, its wave and position in the wave's sequence, edge or interior,
err / bar and the mirrored plan.

Device-free: the mirror against the headers, the coverage of the 27 instantiations and of the hand-overs at 256 CUs, and bite
tests -- float64 models on this file's inputs of a pair transformed from the previous pair's prefetched samples, a run on the
previous run's uncleared ring, a tile accumulated onto an unzeroed buffer, a Kaldi pair reading the previous utterance's base --
each far above its bar.

Measured on an MI355X (256 CUs): MEASURED_DEVICE; wall time FILE_SECONDS = 19.6 s on top of the 413 s of the rest of the device
suite.  No case found a kernel wrong.  Worst per-row err / bar per instantiation, E = 4 / 8 / 16 / 32: stft_pow2_kernel<E, EPI_SPEC>
0.020 / 0.018 / 0.022 / 0.018, <E, EPI_MEL> 0.042 / 0.045 / 0.043 / 0.041 (each on the bank outside LDS), istft_pow2_run_kernel<E>
0.024 / 0.024 / 0.025 / 0.020, istft_pow2_kernel<E> 0.022 / 0.020 / 0.020 / 0.021, istft400_kernel<5 | 8 | 10> 0.017 / 0.024 / 0.028,
kaldi_pow2_kernel<E, 0> 0.15 / 0.21 / 0.16 / 0.25 and <E, 1> 0.014 / 0.007 / 0.007 / 0.005 of judge's tolerance; every all-zero row
came out exactly 0.0 and every second forward call bit-equal.  No shape had to be shrunk: the slowest case takes 2 s.

That the DEVICE cases bite was checked once by hand against a library with four precision-only faults (in bounds; that build is
not committed): (1) stft_pow2_kernel's prefetch took the next pair's samples from the CURRENT pair's row; (2) ring_flush did not
clear the ring; (3) kaldi_pow2_kernel rebased `wav` for a wave's first pair only; (4) istft400_kernel zeroed its tile buffer for a
wave's first tile only.  42 of the 54 device tests failed and 12 passed, exactly as the faults predict: (1) the 18 forward and mel
cases of E <= 16 (the all-zero row came out with peaks of 15 .. 8e3) while the six of E = 32, which does not prefetch, passed;
(2) the eight short and full inverse cases and the two adjoint cases of the run kernel (0.1 .. 0.3 and 25 .. 47 at the all-zero row)
while the four atomic inverse cases and the two adjoint cases with hop > n_fft, which have no ring, passed; (3) all eight Kaldi
cases (7.6e3 .. 9.2e3 tolerances); (4) the four n_fft-400 inverse and the two n_fft-400 adjoint cases (0.07 .. 0.14 and 25 at the
all-zero row).
"""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest
import torch

CU_DESIGN = 256
BAR = 2e-5
WAVES = 4                       # csrc/stft_pow2.h p2::kWaves
RUN_LEN = 16                    # p2::inv_plan run_len
INV400_WAVES, TILE_FRAMES = 8, 6          # csrc/istft400.h kInvWaves, csrc/melspec400.h kFramesPerWave
MEL_LDS_BYTES = 32 * 1024       # csrc/stft_pow2.h kMelLdsBytes
POLICY_ISTFT_ATOMIC = 4         # audio_amd/_lib.py
GAINS = (1.0, 1e-3, 1e-2, 1.0)
SEED_BASE = 91300
SLAB_BYTES = 256 << 20
FRAMES = 37                     # forward / adjoint-free rows: 19 pairs, the last without a frame b

# Measured on an MI355X (256 CUs), one run of this file with -s: kernel -> (worst per-row err / bar, its case), from the
# "[fuzz-stft-pow2]" lines.  For the Kaldi kernels err / bar is the worst element's |got - ref| over judge's own tolerance.
MEASURED_DEVICE = {
    "p2::stft_pow2_kernel<4, EPI_SPEC>": (0.0203, "fwd-256-circular-win-oddhop-mag"),
    "p2::stft_pow2_kernel<8, EPI_SPEC>": (0.0183, "fwd-512-circular-win-oddhop-mag"),
    "p2::stft_pow2_kernel<16, EPI_SPEC>": (0.0216, "fwd-1024-circular-win-oddhop-mag"),
    "p2::stft_pow2_kernel<32, EPI_SPEC>": (0.0179, "fwd-2048-nocenter-power"),
    "p2::stft_pow2_kernel<4, EPI_MEL>": (0.0418, "mel-256-wide"), "p2::stft_pow2_kernel<8, EPI_MEL>": (0.0445, "mel-512-wide"),
    "p2::stft_pow2_kernel<16, EPI_MEL>": (0.0428, "mel-1024-wide"), "p2::stft_pow2_kernel<32, EPI_MEL>": (0.0413, "mel-2048-wide"),
    "p2::istft_pow2_run_kernel<4>": (0.0240, "inv-256-short"), "p2::istft_pow2_run_kernel<8>": (0.0238, "inv-512-short"),
    "p2::istft_pow2_run_kernel<16>": (0.0245, "inv-1024-short"), "p2::istft_pow2_run_kernel<32>": (0.0204, "inv-2048-short"),
    "p2::istft_pow2_kernel<4>": (0.0224, "inv-256-atomic"), "p2::istft_pow2_kernel<8>": (0.0204, "inv-512-atomic"),
    "p2::istft_pow2_kernel<16>": (0.0204, "inv-1024-atomic"), "p2::istft_pow2_kernel<32>": (0.0213, "inv-2048-atomic"),
    "m400::istft400_kernel<5>": (0.0172, "inv-400-hop100"), "m400::istft400_kernel<8>": (0.0238, "inv-400-hop160"),
    "m400::istft400_kernel<10>": (0.0281, "inv-400-hop200-len2400"),
    "p2::kaldi_pow2_kernel<4, 0>": (0.1456, "kaldi-256-spectrogram"), "p2::kaldi_pow2_kernel<8, 0>": (0.2117, "kaldi-512-spectrogram"),
    "p2::kaldi_pow2_kernel<16, 0>": (0.1634, "kaldi-1024-spectrogram"), "p2::kaldi_pow2_kernel<32, 0>": (0.2464, "kaldi-2048-spectrogram"),
    "p2::kaldi_pow2_kernel<4, 1>": (0.0140, "kaldi-256-fbank"), "p2::kaldi_pow2_kernel<8, 1>": (0.0070, "kaldi-512-fbank"),
    "p2::kaldi_pow2_kernel<16, 1>": (0.0067, "kaldi-1024-fbank"), "p2::kaldi_pow2_kernel<32, 1>": (0.0045, "kaldi-2048-fbank"),
}
# No case found a kernel wrong: every all-zero row came out exactly 0.0 and every second forward call bit-equal.  The 54 device tests of this file together: FILE_SECONDS of pytest wall time (2 s for the
# slowest case, under 0.1 s for most: a launch and its float64 reference are milliseconds of device time); SUITE_SECONDS is the
# device suite's wall time in one run with this file in it (432.7 s, 1 490 tests), this file's share taken off: the parent's tests on
# the parent's device code (every code object is unchanged).  This file adds 5 %.
FILE_SECONDS = 19.6
SUITE_SECONDS = 413.0


# --------------------------------------------------------------------------- #
# 1. the host mirror of the launch arithmetic                                 #
# --------------------------------------------------------------------------- #

def _cdiv(a, b):
    return -(-a // b)


def fwd_blocks(E, cu, n_pairs):
    """p2::fwd_blocks."""
    return min(cu * (8 if E <= 8 else 4 if E == 16 else 2), _cdiv(n_pairs, WAVES))


def kaldi_blocks(cu, n_pairs):
    """p2::kaldi_blocks."""
    return min(cu * 4, _cdiv(n_pairs, WAVES))


def inv400_blocks(cu, n_tiles):
    """m400::inv_blocks."""
    return min(cu, _cdiv(n_tiles, INV400_WAVES))


def inv_plan(n_fft, hop, cu, rows, n_frames, atomic):
    """p2::inv_plan."""
    ppr = (n_frames + 1) // 2
    n_pairs = rows * ppr
    blocks = fwd_blocks(n_fft // 64, cu, n_pairs)
    use_runs = hop <= n_fft and not atomic
    rpr = _cdiv(ppr, RUN_LEN)
    n_runs = rows * rpr
    if use_runs:
        blocks = min(blocks, _cdiv(n_runs, WAVES))
    return dict(use_runs=use_runs, run_len=RUN_LEN, runs_per_row=rpr, n_runs=n_runs, blocks=blocks, pairs_per_row=ppr, n_pairs=n_pairs)


def mel_lds_floats(n_mels, max_width):
    """p2::mel_lds_floats (mel_stride = (max_width + 2) | 1)."""
    return n_mels * ((max_width + 2) | 1) + 2 * n_mels


def mel_in_lds(n_mels, max_width):
    return mel_lds_floats(n_mels, max_width) * 4 <= MEL_LDS_BYTES


def mel_tail_lanes(n_mels):
    """p2::mel_tail_lanes."""
    r = n_mels - 64 * ((n_mels - 1) // 64)
    g = 1
    while g < 8 and 2 * g * r <= 64:
        g *= 2
    return g


def stft_frames(length, n_fft, hop, center, pad):
    """functional._stft_desc: n_frames."""
    l1 = length + 2 * pad + (2 * (n_fft // 2) if center else 0)
    return 1 + (l1 - n_fft) // hop


def kaldi_frames(n, win, shift, snip_edges):
    """compliance.kaldi._num_frames."""
    return (0 if n < win else 1 + (n - win) // shift) if snip_edges else (n + shift // 2) // shift


def pair_kind(p, n_fft, hop, length, n_frames, center=True, pad=0):
    """load_raw / inv_store: `interior` (coalesced branch, no index map), `edge`, or `edge-nob` (no frame b)."""
    if 2 * p + 1 >= n_frames:
        return "edge-nob"
    ba = 2 * p * hop - (n_fft // 2 if center else 0) - pad
    return "interior" if ba >= 0 and ba + hop + n_fft <= length else "edge"


def run_interior(k, n_fft, hop, length, n_frames, center=True, pad=0):
    """p2::run_plan: (pi_lo, pi_hi) of run k of a row, pi_lo > pi_hi when the run has no interior pair."""
    ppr = (n_frames + 1) // 2
    p_lo, p_hi = k * RUN_LEN, min(k * RUN_LEN + RUN_LEN, ppr)
    c = (n_fft // 2 if center else 0) + pad
    first = (c + 2 * hop - 1) // (2 * hop)
    last_t = -1 if length + c - n_fft < 0 else min((length + c - n_fft) // hop, n_frames - 1)
    last = -1 if last_t < 1 else (last_t - 1) // 2
    return max(p_lo, first), min(p_hi - 1, last)


def tile_kind(k, hop, length, n_frames):
    """inv400_flush: `interior` (straight-line stores, the `exclusive` rule) or `edge` (index map, atomics)."""
    t0 = k * TILE_FRAMES
    n_valid = min(TILE_FRAMES, n_frames - t0)
    start = t0 * hop - 200
    return "interior" if n_valid == TILE_FRAMES and start >= 0 and start + (TILE_FRAMES - 1) * hop + 400 <= length else "edge"


def make_plan(run, cu):
    """The launch of `run` on a device of `cu` CUs.  An item is a frame pair (forward, atomic inverse, Kaldi), a run of <= 16 pairs
    (run inverse) or a six-frame tile (n_fft 400); item = row * ipr + index in the row; wave w = item % W runs the items w, w + W, ..."""
    fam, n_fft, hop, rows, T = run["family"], run["n_fft"], run["hop"], run["rows"], run["n_frames"]
    E = n_fft // 64
    p = dict(family=fam, cu_count=cu, n_fft=n_fft, hop=hop, rows=rows, n_frames=T, length=run["length"], center=run.get("center", True),
             pad=run.get("pad", 0), kernel=run["kernel"])
    ppr = (T + 1) // 2
    if fam in ("fwd", "mel"):
        p.update(unit="pair", ipr=ppr, blocks=fwd_blocks(E, cu, rows * ppr), waves=WAVES)
    elif fam == "kaldi":
        p.update(unit="pair", ipr=ppr, blocks=kaldi_blocks(cu, rows * ppr), waves=WAVES)
    elif n_fft == 400:
        p.update(unit="tile", ipr=_cdiv(T, TILE_FRAMES), waves=INV400_WAVES)
        p["blocks"] = inv400_blocks(cu, rows * p["ipr"])
    else:
        ip = inv_plan(n_fft, hop, cu, rows, T, run.get("atomic", False))
        p.update(unit="run" if ip["use_runs"] else "pair", ipr=ip["runs_per_row"] if ip["use_runs"] else ppr, blocks=ip["blocks"],
                 waves=WAVES, inv=ip)
    p["items"] = rows * p["ipr"]
    p["W"] = p["blocks"] * p["waves"]
    p["items_per_wave_min"], p["items_per_wave_max"] = p["items"] // p["W"], _cdiv(p["items"], p["W"])
    return p


def item_kind(plan, k):
    """Edge or interior, for item index k within its row."""
    a = (plan["n_fft"], plan["hop"], plan["length"], plan["n_frames"], plan["center"], plan["pad"])
    if plan["family"] == "kaldi":
        return "edge-nob" if 2 * k + 1 >= plan["n_frames"] else "full"
    if plan["unit"] == "pair":
        return pair_kind(k, *a)
    if plan["unit"] == "run":
        lo, hi = run_interior(k, *a)
        return "ring" if lo <= hi else "edge"
    return tile_kind(k, plan["hop"], plan["length"], plan["n_frames"])


def handovers(plan):
    """The set of (kind of an item, kind of the wave's next item) over every wave's sequence."""
    ipr, W = plan["ipr"], plan["W"]
    kinds = [item_kind(plan, k) for k in range(ipr)]
    return {(kinds[i % ipr], kinds[(i + W) % ipr]) for i in range(plan["items"] - W)}


def locate(plan, row, frame=None, sample=None):
    """The item that owns output frame `frame` (forward, Kaldi) or sample `sample` (inverse: the frame whose centre is nearest)."""
    if frame is None:
        frame = min(plan["n_frames"] - 1, max(0, (sample + plan["pad"] + plan["hop"] // 2) // plan["hop"]))
    k = {"pair": frame // 2, "run": frame // 2 // RUN_LEN, "tile": frame // TILE_FRAMES}[plan["unit"]]
    item = row * plan["ipr"] + k
    return dict(row=row, frame=frame, sample=sample, unit=plan["unit"], index_in_row=k, item=item, wave=item % plan["W"],
                position=item // plan["W"], run_length=_cdiv(plan["items"] - item % plan["W"], plan["W"]), kind=item_kind(plan, k),
                kernel=plan["kernel"])


def place_zero_row(plan):
    """The row to silence: the first whose first item is the second or third of its wave, directly behind an item of another, gain-1
    row.  None where no wave runs two items."""
    ipr, W = plan["ipr"], plan["W"]
    for row in range(1, plan["rows"]):
        i0 = row * ipr
        if W <= i0 < 3 * W:
            prev = (i0 - W) // ipr
            if prev != row and GAINS[prev % 4] == 1.0:
                return row
    return None


def regime_fault(run, plan):
    """None when `plan` is what `run` claims, else what it misses (every device case asserts this on the device's CU count)."""
    W, items = plan["W"], plan["items"]
    factor = 1.25 if run["regime"] == "full" else 2.5
    if items < int(factor * W) + (3 if factor == 2.5 else 0) or items % W == 0:
        return "%d items on %d waves" % (items, W)
    if factor == 2.5 and (plan["items_per_wave_min"] < 2 or plan["items_per_wave_max"] < 3):
        return "items per wave %d .. %d" % (plan["items_per_wave_min"], plan["items_per_wave_max"])
    if plan["items_per_wave_max"] < 2 or place_zero_row(plan) is None:
        return "no wave runs a second item"
    if items > int(factor * W) + 3 + 2 * plan["ipr"] + W // 8:
        return "larger than needed: %d items on %d waves" % (items, W)
    h = handovers(plan)
    if run["family"] in ("fwd", "mel"):
        if W % plan["ipr"] == 0:
            return "pairs_per_row %d divides W %d" % (plan["ipr"], W)
        if not (any(a == "interior" and b != "interior" for a, b in h) and any(a != "interior" and b == "interior" for a, b in h)
                and any(a == "edge-nob" for a, b in h)):
            return "hand-overs %s" % sorted(h)
    want_unit = dict(short="run", full="run", atomic="pair", inv400="tile", adj_run="run", adj_atomic="pair", adj400="tile").get(run["regime"])
    if want_unit and plan["unit"] != want_unit:
        return "unit %s, not %s" % (plan["unit"], want_unit)
    if run["regime"] in ("short", "adj_run") and (plan["ipr"] != 1 or item_kind(plan, 0) != "ring"):
        return "a short run without an interior pair"
    if run["regime"] == "full" and (plan["ipr"] != 2 or item_kind(plan, 0) != "ring" or plan["n_frames"] != 2 * RUN_LEN + 1):
        return "not a 16-pair and a 1-pair run"
    if plan["unit"] == "tile" and [item_kind(plan, k) for k in range(plan["ipr"])] != ["edge", "interior", "edge"]:
        return "tiles %s" % [item_kind(plan, k) for k in range(plan["ipr"])]
    if run["regime"] == "adj_atomic" and not plan["hop"] > plan["n_fft"]:
        return "hop <= n_fft"
    return None


# --------------------------------------------------------------------------- #
# 2. the cases                                                                #
# --------------------------------------------------------------------------- #

ES = (4, 8, 16, 32)
ODD_HOP = {4: 101, 8: 161, 16: 411, 32: 513}           # no multiple of 4: unaligned row bases for the coalesced branch


def _k_fwd(E, epi):
    return "p2::stft_pow2_kernel<%d, EPI_%s>" % (E, epi)


def _cases():
    out = []
    for E in ES:
        N = 64 * E
        out += [
            dict(id="fwd-%d-reflect-pad-complex" % N, family="fwd", regime="fwd", kernel=_k_fwd(E, "SPEC"), n_fft=N, hop=N // 4, center=True,
                 pad_mode="reflect", pad=13, wl=N, power=None),
            dict(id="fwd-%d-circular-win-oddhop-mag" % N, family="fwd", regime="fwd", kernel=_k_fwd(E, "SPEC"), n_fft=N, hop=ODD_HOP[E],
                 center=True, pad_mode="circular", pad=0, wl=3 * N // 4, power=1.0),
            dict(id="fwd-%d-nocenter-power" % N, family="fwd", regime="fwd", kernel=_k_fwd(E, "SPEC"), n_fft=N, hop=N // 2, center=False,
                 pad_mode="reflect", pad=0, wl=N, power=2.0),
            dict(id="mel-%d-80" % N, family="mel", regime="fwd", kernel=_k_fwd(E, "MEL"), n_fft=N, hop=N // 4, mel="lds-tail", n_mels=80),
            dict(id="mel-%d-x64" % N, family="mel", regime="fwd", kernel=_k_fwd(E, "MEL"), n_fft=N, hop=ODD_HOP[E], mel="lds-full",
                 n_mels=64 if E <= 8 else 128),
            dict(id="mel-%d-wide" % N, family="mel", regime="fwd", kernel=_k_fwd(E, "MEL"), n_fft=N, hop=N // 2, mel="wide", n_mels=72),
        ]
    for E in ES:
        N = 64 * E
        out += [
            dict(id="inv-%d-short" % N, family="inv", regime="short", kernel="p2::istft_pow2_run_kernel<%d>" % E, n_fft=N, hop=N // 2,
                 n_frames=5, cut=False),
            dict(id="inv-%d-full" % N, family="inv", regime="full", kernel="p2::istft_pow2_run_kernel<%d>" % E, n_fft=N, hop=N // 4,
                 n_frames=2 * RUN_LEN + 1, cut=E in (4, 16)),
            dict(id="inv-%d-atomic" % N, family="inv", regime="atomic", kernel="p2::istft_pow2_kernel<%d>" % E, n_fft=N, hop=N // 2,
                 n_frames=5, cut=True, atomic=True),
        ]
    out += [dict(id="inv-400-hop%d" % hop, family="inv", regime="inv400", kernel="m400::istft400_kernel<%d>" % (hop // 20), n_fft=400, hop=hop,
                 n_frames=15, cut=hop != 200) for hop in (100, 160, 200)]
    out += [dict(id="inv-400-hop200-len2400", family="inv", regime="inv400", kernel="m400::istft400_kernel<10>", n_fft=400, hop=200,
                 n_frames=13, cut=False)]
    out += [
        dict(id="adj-256-run-reflect", family="adj", regime="adj_run", kernel="p2::istft_pow2_run_kernel<4>", n_fft=256, hop=128, n_frames=5,
             pad_mode="reflect"),
        dict(id="adj-1024-run-circular", family="adj", regime="adj_run", kernel="p2::istft_pow2_run_kernel<16>", n_fft=1024, hop=512, n_frames=5,
             pad_mode="circular"),
        dict(id="adj-256-atomic-hop300-reflect", family="adj", regime="adj_atomic", kernel="p2::istft_pow2_kernel<4>", n_fft=256, hop=300,
             n_frames=5, pad_mode="reflect"),
        dict(id="adj-512-atomic-hop600-circular", family="adj", regime="adj_atomic", kernel="p2::istft_pow2_kernel<8>", n_fft=512, hop=600,
             n_frames=5, pad_mode="circular"),
        dict(id="adj-400-hop160-reflect", family="adj", regime="adj400", kernel="m400::istft400_kernel<8>", n_fft=400, hop=160, n_frames=15,
             pad_mode="reflect"),
        dict(id="adj-400-hop100-circular", family="adj", regime="adj400", kernel="m400::istft400_kernel<5>", n_fft=400, hop=100, n_frames=15,
             pad_mode="circular"),
    ]
    frame_ms = {4: 12.5, 8: 25.0, 16: 50.0, 32: 100.0}            # 200 / 400 / 800 / 1600 samples at 16 kHz, padded to 64 E
    for E in ES:
        common = dict(sample_frequency=16000.0, frame_length=frame_ms[E], frame_shift=10.0, round_to_power_of_two=True, dither=0.0,
                      remove_dc_offset=True, preemphasis_coefficient=0.97, energy_floor=0.0)
        out += [
            dict(id="kaldi-%d-spectrogram" % (64 * E), family="kaldi", regime="kaldi", kernel="p2::kaldi_pow2_kernel<%d, 0>" % E, n_fft=64 * E,
                 hop=160, fn="spectrogram", kw=dict(common, snip_edges=E in (4, 16), raw_energy=E in (4, 8), window_type="povey")),
            dict(id="kaldi-%d-fbank" % (64 * E), family="kaldi", regime="kaldi", kernel="p2::kaldi_pow2_kernel<%d, 1>" % E, n_fft=64 * E,
                 hop=160, fn="fbank", kw=dict(common, snip_edges=E in (8, 32), raw_energy=E in (16, 32), window_type="hamming",
                                              num_mel_bins=23 if E <= 8 else 40, use_energy=True, htk_compat=E in (8, 16))),
        ]
    return out


CASES = _cases()
CASE_IDS = [c["id"] for c in CASES]
KERNELS_WANTED = ({_k_fwd(E, e) for E in ES for e in ("SPEC", "MEL")} | {"p2::istft_pow2_kernel<%d>" % E for E in ES}
                  | {"p2::istft_pow2_run_kernel<%d>" % E for E in ES} | {"p2::kaldi_pow2_kernel<%d, %d>" % (E, m) for E in ES for m in (0, 1)}
                  | {"m400::istft400_kernel<%d>" % h for h in (5, 8, 10)})


def _geometry(case):
    """(n_frames, signal length per row, `length` argument of the inverse or None) of a case: the frame counts the issue sets."""
    N, hop = case["n_fft"], case["hop"]
    fam = case["family"]
    if fam in ("fwd", "mel"):
        center, pad = case.get("center", True), case.get("pad", 0)
        L = (FRAMES - 1) * hop + 7 - 2 * pad + (0 if center else N)       # + 7: odd row lengths, unaligned row bases
        assert stft_frames(L, N, hop, center, pad) == FRAMES
        return FRAMES, L, None
    if fam == "inv":
        T = case["n_frames"]
        natural = hop * (T - 1)
        if case["id"].endswith("len2400"):
            assert natural == 2400 and natural % 1200 == 0
        length = natural - 37 if case["cut"] else None                      # ends inside the last frame (whose centre is `natural`)
        return T, length if case["cut"] else natural, length
    if fam == "adj":
        T = case["n_frames"]
        L = hop * (T - 1) + (0 if case["regime"] == "adj_run" else 7)       # the run shape needs L = 2 n_fft exactly (an interior pair)
        assert stft_frames(L, N, hop, True, 0) == T
        return T, L, None
    kw = case["kw"]
    win, shift = int(16000 * kw["frame_length"] * 0.001), 160
    n = win + (FRAMES - 1) * shift + 7 if kw["snip_edges"] else FRAMES * shift - shift // 2 + 7
    assert kaldi_frames(n, win, shift, kw["snip_edges"]) == FRAMES and (1 << (win - 1).bit_length()) == N
    return FRAMES, n, None


@functools.lru_cache(maxsize=None)
def draw_run(idx, cu=CU_DESIGN):
    """Case `idx` sized for a device of `cu` CUs by the mirror -- a function of (idx, cu) alone."""
    case = CASES[idx]
    T, L, length_arg = _geometry(case)
    run = dict(case, n_frames=T, length=L, length_arg=length_arg, seed=SEED_BASE + 10 * idx)
    probe = make_plan(dict(run, rows=1 << 22), cu)              # W with the grid at its cap
    factor = 1.25 if case["regime"] == "full" else 2.5
    rows = _cdiv(int(factor * probe["W"]) + (3 if factor == 2.5 else 1), probe["ipr"])
    fault = None
    for more in range(8):
        run["rows"] = rows + more
        plan = make_plan(run, cu)
        fault = regime_fault(run, plan)
        if fault is None:
            run["zero_row"] = place_zero_row(plan)
            return run
    raise AssertionError((case["id"], fault, "%d CUs" % cu))


# --------------------------------------------------------------------------- #
# 3. inputs, references and checks (torch, on whatever device is asked)       #
# --------------------------------------------------------------------------- #

def gains(rows, dev):
    return torch.tensor([GAINS[r % 4] for r in range(rows)], device=dev, dtype=torch.float32)


def make_rows(run, width, dev, extra=()):
    """(rows, *extra, width) float32: standard normal clamped to [-1, 1], times the row gain, the run's zero row silenced."""
    gen = torch.Generator(device=dev).manual_seed(run["seed"])
    x = torch.randn((run["rows"],) + tuple(extra) + (width,), generator=gen, device=dev, dtype=torch.float32).clamp_(-1.0, 1.0)
    x.mul_(gains(run["rows"], dev).view((-1,) + (1,) * (x.dim() - 1)))
    if run["zero_row"] is not None:
        x[run["zero_row"]] = 0.0
    return x


def make_spectrum(run, dev):
    """(rows, T, F) complex64, frame-major (what the inverse kernels read): DC and Nyquist imaginary parts zero."""
    s = make_rows(run, 2, dev, extra=(run["n_frames"], run["n_fft"] // 2 + 1))
    s[:, :, 0, 1] = 0.0
    s[:, :, -1, 1] = 0.0
    return torch.view_as_complex(s)


def window64(run, dev):
    return torch.hann_window(run.get("wl", run["n_fft"]), dtype=torch.float64, device=dev)


def wide_bank(n_freq, n_mels=72):
    """A banded filterbank that cannot sit in the kernel's 32 KB table: 72 bands of min(n_freq, 160) bins, spread over the bins."""
    width = min(n_freq, 160)
    g = torch.Generator().manual_seed(SEED_BASE + n_freq)
    fb = torch.zeros(n_freq, n_mels)
    for m in range(n_mels):
        lo = m * (n_freq - width) // (n_mels - 1)
        fb[lo:lo + width, m] = (0.25 + 0.75 * torch.rand(width, generator=g)) / width
    return fb


@functools.lru_cache(maxsize=None)
def mel_module(idx):
    """The MelSpectrogram of a mel case (on the CPU; the device test moves it) and the mirror's view of its filterbank:
    (module, table in LDS, tail_G)."""
    import audio_amd.transforms as T
    from audio_amd import _host
    case = CASES[idx]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")           # (narrow filters at the low end have no bin at small n_fft: the reference warns too)
        m = T.MelSpectrogram(sample_rate=16000, n_fft=case["n_fft"], hop_length=case["hop"], n_mels=case["n_mels"])
    if case["mel"] == "wide":
        m.mel_scale.fb = wide_bank(case["n_fft"] // 2 + 1, case["n_mels"])
    max_width = _host.mel_band_table(m.mel_scale.fb.numpy())[3]
    in_lds = mel_in_lds(case["n_mels"], max_width)
    return m, in_lds, mel_tail_lanes(case["n_mels"]) if in_lds else 1


MEL_CLAIMS = {"lds-tail": lambda in_lds, g: in_lds and g > 1, "lds-full": lambda in_lds, g: in_lds and g == 1,
              "wide": lambda in_lds, g: not in_lds}


def ref_stft64(run, x):
    """(r, L) float32 -> (r, F, T) complex128: the reference composition of Spectrogram (zero padding, torch.stft)."""
    xd = x.double()
    if run.get("pad", 0):
        xd = torch.nn.functional.pad(xd, (run["pad"], run["pad"]))
    wl = run.get("wl", run["n_fft"])
    return torch.stft(xd, run["n_fft"], run["hop"], wl, window64(run, x.device), run.get("center", True), run.get("pad_mode", "reflect"),
                      False, True, return_complex=True)


def ref_istft(run, spec_fm, dtype):
    """(r, T, F) complex -> (r, length): torch.istft in `dtype` (complex128: the reference; complex64: the yardstick)."""
    w = window64(run, spec_fm.device)
    return torch.istft(spec_fm.transpose(-1, -2).to(dtype), run["n_fft"], run["hop"], run["n_fft"], w if dtype == torch.complex128 else w.float(),
                       True, False, True, run["length_arg"], False)


def row_errors(got, ref):
    """(r, ...) x 2 -> per row (max|got - ref|, max|ref|, flat index of the worst element)."""
    d = (got.double() - ref).abs().flatten(1)
    e, where = d.max(1)
    return e, ref.abs().flatten(1).amax(1), where


def slab_rows(bytes_per_row):
    return max(1, SLAB_BYTES // max(1, bytes_per_row))


_WORST = {}


def _note(plan, run, ratio, loc):
    k = plan["kernel"]
    if ratio >= _WORST.get(k, (-1.0,))[0]:
        _WORST[k] = (ratio, run["id"])
    print(f"[fuzz-stft-pow2] {k} {run['id']} rows={run['rows']} items={plan['items']} W={plan['W']} err/bar={ratio:.4f} "
          f"(worst of this kernel so far {_WORST[k][0]:.4f} {_WORST[k][1]}) at {loc}")


def judge_rows(run, plan, err, peak, where, bars, where_to_loc):
    """Per-row relative errors against per-row bars; the zero row is checked apart (exactly 0.0) and left out here."""
    live = torch.ones_like(err, dtype=torch.bool)
    if run["zero_row"] is not None:
        live[run["zero_row"]] = False
    assert bool((torch.isfinite(peak) & (peak > 0))[live].all()), (run["id"], "a row without a reference peak: its bar cannot be evaluated")
    ratio = torch.where(live, err / peak.clamp_min(1e-300) / bars, torch.zeros_like(err))
    r = int(ratio.argmax())
    loc = where_to_loc(r, int(where[r]))
    _note(plan, run, float(ratio[r]), loc)
    assert float(ratio[r]) <= 1.0, (run["id"], "per-row err / bar", float(ratio[r]), "err", float(err[r] / peak[r]), "bar", float(bars[r]),
                                    loc, plan)
    return float(ratio[r])


def assert_zero_row(run, plan, got_row, where_to_loc):
    z = run["zero_row"]
    worst = float(got_row.abs().max())
    assert worst == 0.0, (run["id"], "the all-zero row", worst, where_to_loc(z, int(got_row.abs().flatten().argmax())), plan)


# --------------------------------------------------------------------------- #
# 4. the device tests                                                         #
# --------------------------------------------------------------------------- #

def device_cu():
    """The CU count as csrc/api_common.hip reads it (multiProcessorCount), checked against aamd_device_info."""
    from audio_amd import _lib
    cu = int(torch.cuda.get_device_properties(0).multi_processor_count)
    name, cus, mem = C.create_string_buffer(128), C.c_int32(0), C.c_int64(0)
    _lib.check(_lib.lib().aamd_device_info(name, 128, C.byref(cus), C.byref(mem)))
    assert cus.value == cu and cu >= 5, (cus.value, cu)
    return cu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from audio_amd import _lib
    _lib.lib()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def cu(dev):
    return device_cu()


def _sized(idx, cu):
    run = draw_run(idx, cu)
    plan = make_plan(run, cu)
    fault = regime_fault(run, plan)
    assert fault is None and run["zero_row"] is not None, (run, fault, f"{cu} CUs", plan)
    return run, plan


def check_forward(idx, cu, dev):
    import audio_amd.transforms as T
    run, plan = _sized(idx, cu)
    T_, F, rows = run["n_frames"], run["n_fft"] // 2 + 1, run["rows"]
    x = make_rows(run, run["length"], dev)
    if run["family"] == "mel":
        m, in_lds, tail_g = mel_module(idx)
        assert MEL_CLAIMS[run["mel"]](in_lds, tail_g), (run["id"], in_lds, tail_g)
        t = m.to(dev)
        fb64 = t.mel_scale.fb.double()
        power, cols = 2.0, run["n_mels"]
    else:
        w32 = window64(run, "cpu").float()
        t = T.Spectrogram(n_fft=run["n_fft"], win_length=run["wl"], hop_length=run["hop"], pad=run["pad"], power=run["power"],
                          center=run["center"], pad_mode=run["pad_mode"], window_fn=lambda n: w32).to(dev)
        power, cols = run["power"], F
    with torch.no_grad():
        got = t(x)
        again = t(x)
    assert got.shape == (rows, cols, T_), (got.shape, run)
    assert torch.equal(torch.view_as_real(got) if got.is_complex() else got, torch.view_as_real(again) if again.is_complex() else again), \
        (run["id"], "a second call differs")
    del again

    def loc(row, flat):
        per = cols * T_ * (2 if power is None else 1)
        flat %= per
        return locate(plan, row, frame=(flat // (2 if power is None else 1)) % T_)          # (r, cols, T[, 2]) logical order

    assert bool(torch.isfinite(torch.view_as_real(got) if got.is_complex() else got).all()), (run["id"], "non-finite output")
    errs, peaks, wheres = [], [], []
    step = slab_rows(T_ * F * 16)
    for ra in range(0, rows, step):
        ref = ref_stft64(run, x[ra:ra + step])
        g = got[ra:ra + step]
        if run["family"] == "mel":
            ref = torch.matmul(ref.abs().pow(2.0).transpose(-1, -2), fb64).transpose(-1, -2)
            e = row_errors(g, ref)
        elif power is None:
            e = row_errors(torch.view_as_real(g), torch.view_as_real(ref))
        else:                      # in the power-spectrum domain: fractional powers amplify the rounding of near-zero bins without bound
            e = row_errors(g.double().pow(2.0 / power), ref.abs().pow(2.0))
        for acc, v in zip((errs, peaks, wheres), e):
            acc.append(v)
        del ref
    err, peak, where = torch.cat(errs), torch.cat(peaks), torch.cat(wheres)
    gz = got[run["zero_row"]]
    assert_zero_row(run, plan, torch.view_as_real(gz) if gz.is_complex() else gz, loc)
    judge_rows(run, plan, err, peak, where, torch.full_like(err, BAR), loc)


def check_inverse(idx, cu, dev):
    import audio_amd.transforms as T
    from audio_amd import _lib
    run, plan = _sized(idx, cu)
    rows, T_, F = run["rows"], run["n_frames"], run["n_fft"] // 2 + 1
    spec = make_spectrum(run, dev)
    assert spec.numel() * 8 < 1 << 30, (run["id"], "spectrum of 1 GB or more")
    inv = T.InverseSpectrogram(n_fft=run["n_fft"], hop_length=run["hop"]).to(dev)
    with torch.no_grad():
        if run.get("atomic"):
            with _lib.kernel_policy(POLICY_ISTFT_ATOMIC):
                got = inv(spec.transpose(-1, -2), run["length_arg"])
        else:
            got = inv(spec.transpose(-1, -2), run["length_arg"])
    assert got.shape == (rows, run["length"]), (got.shape, run)
    assert bool(torch.isfinite(got).all()), (run["id"], "non-finite output")

    def loc(row, flat):
        return locate(plan, row, sample=flat)

    errs, peaks, wheres, e32s = [], [], [], []
    step = slab_rows(T_ * max(F, run["n_fft"] // 2) * 16)
    for ra in range(0, rows, step):
        ref = ref_istft(run, spec[ra:ra + step], torch.complex128)
        e, p, w = row_errors(got[ra:ra + step], ref)
        e32 = row_errors(ref_istft(run, spec[ra:ra + step], torch.complex64), ref)[0]
        for acc, v in zip((errs, peaks, wheres, e32s), (e, p, w, e32)):
            acc.append(v)
        del ref
    err, peak, where, e32 = torch.cat(errs), torch.cat(peaks), torch.cat(wheres), torch.cat(e32s)
    assert_zero_row(run, plan, got[run["zero_row"]], loc)
    # yardstick: aten's own float32 istft on the same spectrum, per row (test_fuzz_inverse_spectrogram_vs_aten_istft)
    bars = torch.clamp_min(4.0 * e32 / peak.clamp_min(1e-300), BAR)
    bars[run["zero_row"]] = BAR
    assert bool(torch.isfinite(bars).all()), (run["id"], "a row whose float32 yardstick cannot be evaluated")
    judge_rows(run, plan, err, peak, where, bars, loc)


def check_adjoint(idx, cu, dev):
    import audio_amd.transforms as T
    run, plan = _sized(idx, cu)
    rows, T_, F, L = run["rows"], run["n_frames"], run["n_fft"] // 2 + 1, run["length"]
    r_fm = make_spectrum(run, dev)                                    # the cotangent: its row gains and zero row become the gradient's
    x = make_rows(dict(run, seed=run["seed"] + 1, zero_row=None), L, dev).requires_grad_()
    w32 = window64(run, "cpu").float()
    t = T.Spectrogram(n_fft=run["n_fft"], hop_length=run["hop"], power=None, center=True, pad_mode=run["pad_mode"],
                      window_fn=lambda n: w32).to(dev)
    y = t(x)
    assert y.shape == (rows, F, T_), (y.shape, run)
    (y * r_fm.transpose(-1, -2).conj()).real.sum().backward()
    got = x.grad
    assert got.shape == (rows, L) and bool(torch.isfinite(got).all()), (run["id"], got.shape)

    def loc(row, flat):
        return locate(plan, row, sample=flat)

    errs, peaks, wheres = [], [], []
    step = slab_rows(T_ * F * 16 * 2)
    for ra in range(0, rows, step):
        xr = x.detach()[ra:ra + step].double().requires_grad_()
        ref = ref_stft64(run, xr)
        (ref * r_fm[ra:ra + step].transpose(-1, -2).to(torch.complex128).conj()).real.sum().backward()
        for acc, v in zip((errs, peaks, wheres), row_errors(got[ra:ra + step], xr.grad)):
            acc.append(v)
        del ref, xr
    err, peak, where = torch.cat(errs), torch.cat(peaks), torch.cat(wheres)
    assert_zero_row(run, plan, got[run["zero_row"]], loc)
    judge_rows(run, plan, err, peak, where, torch.full_like(err, BAR), loc)      # no taper division in the adjoint: 2e-5


def kaldi_tolerance(ref, fn, kw):
    """judge's tolerance for natural-log features, restated for the err / bar record and for locating a failure; the assertion is
    judge's own."""
    under = ref.max(axis=1, keepdims=True) - ref
    if fn == "fbank" and not kw.get("use_power", True):
        under = 2.0 * under
    return 3e-3 + 2.0 * 3e-7 * np.exp(np.minimum(0.5 * under, 30.0))


def kaldi_reference(run, x):
    """oracle/kaldi_oracle.py per utterance: (n_utt, n) -> (n_utt * n_frames, cols) float64."""
    from oracle import kaldi_oracle as KO
    return np.concatenate([getattr(KO, run["fn"])(u, **run["kw"]) for u in x], axis=0)


def check_kaldi(idx, cu, dev):
    import kaldi_fuzz_cases as KC
    import audio_amd.compliance.kaldi as K
    run, plan = _sized(idx, cu)
    x = make_rows(run, run["length"], dev)
    with torch.no_grad():
        got = getattr(K, run["fn"] + "_batch")(x, **run["kw"])
    assert got.shape[:2] == (run["rows"], run["n_frames"]) and bool(torch.isfinite(got).all()), (got.shape, run["id"])
    got = got.cpu().numpy().reshape(run["rows"] * run["n_frames"], -1)
    ref = kaldi_reference(run, x.cpu().numpy())
    ratio = np.abs(got - ref) / kaldi_tolerance(ref, run["fn"], run["kw"])
    flat = int(ratio.argmax())
    frame_row = flat // ref.shape[1]
    loc = dict(locate(plan, frame_row // run["n_frames"], frame=frame_row % run["n_frames"]), column=flat % ref.shape[1])
    _note(plan, run, float(ratio.max()), loc)
    try:
        KC.judge(got, ref, run["fn"], run["kw"], ref)
    except AssertionError as e:
        raise AssertionError((run["id"], str(e), "err / tolerance", float(ratio.max()), loc, plan)) from e


CHECKS = dict(fwd=check_forward, mel=check_forward, inv=check_inverse, adj=check_adjoint, kaldi=check_kaldi)


@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(len(CASES)), ids=CASE_IDS)
def test_fuzz_register_fft_kernels_in_multi_item_runs_vs_float64(idx, dev, cu):
    CHECKS[CASES[idx]["family"]](idx, cu, dev)


# --------------------------------------------------------------------------- #
# 5. no device: the mirror against the headers, coverage, bite                #
# --------------------------------------------------------------------------- #

def _against_headers(n_fft, hop, cu, rows, n_frames, atomic):
    import sim_util as S
    ppr = (n_frames + 1) // 2
    if n_fft == 400:
        n_tiles = rows * _cdiv(n_frames, TILE_FRAMES)
        assert S.sim_m400_inv_blocks(cu, n_tiles) == inv400_blocks(cu, n_tiles), (cu, n_tiles)
        return
    assert S.sim_p2_fwd_blocks(n_fft // 64, cu, rows * ppr) == fwd_blocks(n_fft // 64, cu, rows * ppr), (n_fft, cu, rows, ppr)
    assert S.sim_p2_kaldi_blocks(cu, rows * ppr) == kaldi_blocks(cu, rows * ppr), (cu, rows, ppr)
    assert S.sim_p2_inv_plan(n_fft, hop, cu, rows, n_frames, atomic) == inv_plan(n_fft, hop, cu, rows, n_frames, atomic), \
        (n_fft, hop, cu, rows, n_frames, atomic)


def test_mirror_equals_the_headers_launch_arithmetic():
    """fwd_blocks / inv_plan / kaldi_blocks / inv400_blocks against p2::fwd_blocks / p2::inv_plan / p2::kaldi_blocks / m400::inv_blocks
    themselves for every case's shape at 256, 8 and 5 CUs, and over a sweep on both sides of every cap."""
    n = 0
    for idx in range(len(CASES)):
        for cu in (CU_DESIGN, 8, 5):
            run = draw_run(idx, cu)
            assert regime_fault(run, make_plan(run, cu)) is None, (run["id"], cu)
            _against_headers(run["n_fft"], run["hop"], cu, run["rows"], run["n_frames"], bool(run.get("atomic")))
            n += 1
    r = np.random.default_rng(SEED_BASE)
    for n_fft in (256, 512, 1024, 2048, 400):
        for _ in range(40):
            cu, rows = int(r.choice([1, 2, 5, 8, 104, 256, 304])), int(r.choice([1, 2, 3, 7, 100, 1079, 5121, 20483, 100000]))
            hop = int(r.choice([n_fft // 4, n_fft // 2, n_fft, n_fft + 1, 2 * n_fft, 100]))
            _against_headers(n_fft, hop, cu, rows, int(r.integers(1, 80)), bool(r.integers(0, 2)))
            n += 1
    assert n > 300


def test_launch_arithmetic_by_hand():
    """The mirror on numbers worked out by hand from the launchers at 256 CUs."""
    assert [fwd_blocks(E, 256, 10 ** 6) * WAVES for E in ES] == [8192, 8192, 4096, 2048]
    assert kaldi_blocks(256, 10 ** 6) * WAVES == 4096 and inv400_blocks(256, 10 ** 6) * INV400_WAVES == 2048
    assert fwd_blocks(8, 256, 57) == 15 and inv400_blocks(256, 9) == 2
    p = inv_plan(512, 128, 256, 3, 33, False)
    assert (p["use_runs"], p["runs_per_row"], p["n_runs"], p["n_pairs"], p["blocks"]) == (True, 2, 6, 51, 2)
    assert not inv_plan(512, 513, 256, 3, 33, False)["use_runs"] and not inv_plan(512, 128, 256, 3, 33, True)["use_runs"]
    assert inv_plan(512, 128, 256, 3, 33, True)["blocks"] == 13
    run = draw_run(CASE_IDS.index("fwd-256-reflect-pad-complex"))
    plan = make_plan(run, CU_DESIGN)
    assert (run["rows"], plan["ipr"], plan["items"], plan["W"]) == (1079, 19, 20501, 8192)
    # pad 13 makes pair 1 an edge pair too: its frame a starts 13 samples in front of the row
    assert [item_kind(plan, k) for k in (0, 1, 2, 16, 17, 18)] == ["edge", "edge", "interior", "interior", "edge", "edge-nob"]
    w = locate(plan, 432, frame=5)
    assert (w["item"], w["wave"], w["position"], w["run_length"], w["kind"]) == (8210, 18, 1, 3, "interior")
    run = draw_run(CASE_IDS.index("inv-512-full"))
    plan = make_plan(run, CU_DESIGN)
    assert (run["rows"], plan["unit"], plan["ipr"], plan["items"], plan["W"]) == (5121, "run", 2, 10242, 8192)
    assert [item_kind(plan, k) for k in (0, 1)] == ["ring", "edge"] and run_interior(0, 512, 128, run["length"], 33) == (1, 14)
    run = draw_run(CASE_IDS.index("inv-400-hop200-len2400"))
    plan = make_plan(run, CU_DESIGN)
    assert (run["length"], plan["ipr"], plan["W"], [item_kind(plan, k) for k in range(3)]) == (2400, 3, 2048, ["edge", "interior", "edge"])


def test_cases_cover_the_instantiations_and_the_handovers():
    """What the cases pin, from the mirror at 256 CUs; a change of a case or of the sizing cannot silently lose one."""
    assert len(set(CASE_IDS)) == len(CASES)
    every = [(draw_run(i), make_plan(draw_run(i), CU_DESIGN)) for i in range(len(CASES))]
    for run, plan in every:
        assert regime_fault(run, plan) is None, (run, plan)
        assert plan["items_per_wave_max"] >= 2 and run["zero_row"] is not None, run["id"]
        z = run["zero_row"] * plan["ipr"]
        assert z // plan["W"] in (1, 2) and GAINS[((z - plan["W"]) // plan["ipr"]) % 4] == 1.0, run["id"]
    # the 27 instantiations, each in a launch whose every wave runs >= 2 items (the 1-pair-run regime: a quarter of them)
    assert {p["kernel"] for _, p in every} == KERNELS_WANTED and len(KERNELS_WANTED) == 27
    assert {p["kernel"] for r, p in every if p["items_per_wave_min"] >= 2 and p["items_per_wave_max"] >= 3} == KERNELS_WANTED
    # the issue's item counts at 256 CUs: about 20 483 / 20 483 / 10 243 / 5 123 pairs, 10 243 Kaldi pairs, 5 123 tiles
    for run, plan in every:
        if run["regime"] != "full":
            want = int(2.5 * plan["W"]) + 3
            assert want <= plan["items"] < want + 8 * plan["ipr"], (run["id"], plan["items"], want)
    assert {(p["n_fft"], p["W"]) for r, p in every if r["family"] in ("fwd", "mel")} == {(256, 8192), (512, 8192), (1024, 4096), (2048, 2048)}
    assert {p["W"] for r, p in every if r["family"] == "kaldi"} == {4096} and {p["W"] for r, p in every if p["unit"] == "tile"} == {2048}
    # forward: the three hand-overs on every case; per E the padding modes, pad > 0, win_length < n_fft, an odd hop, the three outputs
    for run, plan in every:
        if run["family"] in ("fwd", "mel"):
            h = handovers(plan)
            assert any(a == "interior" and b != "interior" for a, b in h) and any(a != "interior" and b == "interior" for a, b in h) \
                and any(a == "edge-nob" for a, b in h), (run["id"], h)
            if run.get("center", True):                     # (center=False has no edge pair but the frame-b-less one)
                assert {("interior", "edge"), ("edge", "interior")} <= h, (run["id"], h)
            assert plan["W"] % plan["ipr"] and run["n_frames"] % 2 == 1
    for E in ES:
        f = [r for r, _ in every if r["family"] == "fwd" and r["n_fft"] == 64 * E]
        assert {(r["center"], r["pad_mode"]) for r in f} >= {(True, "reflect"), (True, "circular")} and any(not r["center"] for r in f)
        assert any(r["pad"] > 0 for r in f) and any(r["wl"] < r["n_fft"] for r in f) and any(r["hop"] % 4 for r in f)
        assert {r["power"] for r in f} == {None, 1.0, 2.0}
        assert {r["mel"] for r, _ in every if r["family"] == "mel" and r["n_fft"] == 64 * E} == {"lds-tail", "lds-full", "wide"}
    for i, c in enumerate(CASES):
        if c["family"] == "mel":
            _, in_lds, tail_g = mel_module(i)
            assert MEL_CLAIMS[c["mel"]](in_lds, tail_g), (c["id"], in_lds, tail_g)
    # inverse: per E short runs through the ring, a 16-pair and a 1-pair run, the atomic kernel; `length` cut on half of the cases
    inv = [(r, p) for r, p in every if r["family"] == "inv"]
    assert len(inv) == 16 and sum(1 for r, _ in inv if r["cut"]) == 8
    for E in ES:
        assert {r["regime"] for r, _ in inv if r["n_fft"] == 64 * E} == {"short", "full", "atomic"}
    assert all(r["length"] % 1200 == 0 for r, _ in inv if r["id"].endswith("len2400"))
    assert all(r["hop"] <= r["n_fft"] // 2 for r, _ in inv)                               # NOLA with the Hann window
    assert all(r["rows"] * r["n_frames"] * (r["n_fft"] // 2 + 1) * 8 < 1 << 30 for r, _ in every if r["family"] in ("inv", "adj"))
    # adjoint: the three kernels, both folding pad modes each
    adj = [r for r, _ in every if r["family"] == "adj"]
    assert {(r["regime"], r["pad_mode"]) for r in adj} == {(g, m) for g in ("adj_run", "adj_atomic", "adj400") for m in ("reflect", "circular")}
    # Kaldi: both kernels per E; both snip_edges and raw_energy values on each mode; DC removal, pre-emphasis, an energy column
    kal = [r for r, _ in every if r["family"] == "kaldi"]
    for fn in ("spectrogram", "fbank"):
        k = [r["kw"] for r in kal if r["fn"] == fn]
        assert {(a["snip_edges"], a["raw_energy"]) for a in k} == {(True, True), (True, False), (False, True), (False, False)}
        assert all(a["remove_dc_offset"] and a["preemphasis_coefficient"] == 0.97 and a["dither"] == 0.0 for a in k)
    assert all(r["kw"]["use_energy"] for r in kal if r["fn"] == "fbank")


BITE_MIN = 100.0           # "far above": every model must miss its bar by at least this factor


def test_bite_prefetched_samples_of_the_previous_pair():
    """A pair transformed from the samples the wave fetched for its PREVIOUS pair: every item behind a wave's first carries the
    frames of the item W before it."""
    idx = CASE_IDS.index("fwd-256-nocenter-power")
    run, plan = draw_run(idx), make_plan(draw_run(idx), CU_DESIGN)
    x = make_rows(run, run["length"], "cpu")
    ref = ref_stft64(run, x).abs().pow(2.0)                               # (rows, F, T)
    rows, F, T_ = ref.shape
    items = torch.nn.functional.pad(ref, (0, 1)).reshape(rows, F, plan["ipr"], 2).permute(0, 2, 1, 3).reshape(rows * plan["ipr"], F, 2)
    bad = items.clone()
    bad[plan["W"]:] = items[:-plan["W"]]
    bad = bad.reshape(rows, plan["ipr"], F, 2).permute(0, 2, 1, 3).reshape(rows, F, T_ + 1)[:, :, :T_]
    e, peak, _ = row_errors(bad, ref)
    z = run["zero_row"]
    assert float(bad[z].abs().max()) > 0.0                                # the zero row picks up a gain-1 row's frames
    live = torch.arange(rows) != z
    first_wave_rows = plan["W"] // plan["ipr"]                            # rows wholly in front of item W are untouched
    assert float((e / peak.clamp_min(1e-300))[:first_wave_rows][live[:first_wave_rows]].max()) == 0.0
    later = (e / peak.clamp_min(1e-300))[first_wave_rows + 1:][live[first_wave_rows + 1:]]
    assert float(later.min()) / BAR >= BITE_MIN, float(later.min()) / BAR


def _inverse_bite(case_id, add_frames):
    """torch.istft of the file's own spectrum for the rows of 48 items behind their waves' first, with add_frames(faulty row, spec,
    k, prow, pk) adding what the fault leaves of item (prow, pk) in item k of the row; returns the per-row err / bar of those rows
    under the device cases' own bar, max(2e-5, 4 x the float32 yardstick)."""
    idx = CASE_IDS.index(case_id)
    run, plan = draw_run(idx), make_plan(draw_run(idx), CU_DESIGN)
    spec = make_spectrum(run, "cpu")
    rows = sorted({i // plan["ipr"] for i in range(plan["W"] + plan["ipr"], plan["W"] + 49 * plan["ipr"])} - {run["zero_row"]})
    faulty = spec[rows].clone()
    for n, row in enumerate(rows):
        for k in range(plan["ipr"]):
            j = row * plan["ipr"] + k - plan["W"]
            assert j >= 0 and j // plan["ipr"] != row
            add_frames(faulty[n], spec, k, j // plan["ipr"], j % plan["ipr"])
    ref = ref_istft(run, spec[rows], torch.complex128)
    e32 = row_errors(ref_istft(run, spec[rows], torch.complex64), ref)[0]
    e, peak, _ = row_errors(ref_istft(run, faulty, torch.complex128), ref)
    return (e / peak) / torch.clamp_min(4.0 * e32 / peak, BAR), run


def test_bite_run_on_the_previous_runs_uncleared_ring():
    """A run that starts on the ring its wave's previous run left: in the 5-frame shape the ring index is the sample index, so the
    residue of the previous run's interior pair (frames 2, 3) lands on this run's frames 2, 3.  (W is a multiple of 4: a run and
    its wave's previous run have the same gain.)"""
    def add(f, spec, k, prow, pk):
        f[2:4] += spec[prow, 2:4]
    ratio, _ = _inverse_bite("inv-256-short", add)
    assert float(ratio.min()) >= BITE_MIN, float(ratio.min())


def test_bite_tile_accumulated_onto_an_unzeroed_buffer():
    """A six-frame tile overlap-added onto the buffer of the wave's previous tile: frame j of that tile lands on frame j of this
    one.  A gain-1 row that inherits only tiles of 1e-3 and 1e-2 rows still misses by tens of bars; the median row by thousands."""
    def add(f, spec, k, prow, pk):
        T_ = f.shape[0]
        nv = min(TILE_FRAMES, T_ - TILE_FRAMES * k, T_ - TILE_FRAMES * pk)
        f[TILE_FRAMES * k:TILE_FRAMES * k + nv] += spec[prow, TILE_FRAMES * pk:TILE_FRAMES * pk + nv]
    ratio, _ = _inverse_bite("inv-400-hop200", add)
    assert float(ratio.min()) >= 10.0 and float(ratio.median()) >= BITE_MIN, (float(ratio.min()), float(ratio.median()))


def test_bite_kaldi_pair_reading_the_previous_utterances_base():
    """A Kaldi pair whose wav pointer still stands on the utterance of the wave's previous pair: the frames come from that utterance
    at this pair's own frame index.  judge must refuse it, far above its tolerance."""
    import kaldi_fuzz_cases as KC
    from oracle import kaldi_oracle as KO
    idx = CASE_IDS.index("kaldi-512-fbank")
    run, plan = draw_run(idx), make_plan(draw_run(idx), CU_DESIGN)
    x = make_rows(run, run["length"], "cpu").numpy()
    utts = [u for u in range(plan["W"] // plan["ipr"] + 1, plan["W"] // plan["ipr"] + 7) if u != run["zero_row"]]
    worst = []
    for u in utts:
        ref = getattr(KO, run["fn"])(x[u], **run["kw"])
        bad = ref.copy()
        for k in range(plan["ipr"]):
            prev = (u * plan["ipr"] + k - plan["W"]) // plan["ipr"]
            assert prev != u
            bad[2 * k:2 * k + 2] = getattr(KO, run["fn"])(x[prev], **run["kw"])[2 * k:2 * k + 2]
        with pytest.raises(AssertionError):
            KC.judge(bad, ref, run["fn"], run["kw"], ref)
        worst.append(float((np.abs(bad - ref) / kaldi_tolerance(ref, run["fn"], run["kw"])).max()))
    assert min(worst) >= BITE_MIN, worst


def test_measured_table_names_every_instantiation():
    """MEASURED_DEVICE holds one figure per instantiation, each under its bar, and FILE_SECONDS is recorded."""
    assert set(MEASURED_DEVICE) == KERNELS_WANTED
    assert all(0.0 <= v[0] <= 1.0 and v[1] in CASE_IDS for v in MEASURED_DEVICE.values())
    assert FILE_SECONDS is not None and FILE_SECONDS > 0
