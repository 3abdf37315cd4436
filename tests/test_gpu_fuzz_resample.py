"""Every matrix-core resampling kernel (csrc/resample_mfma.h, launched by aamd_resample_prepared_f32 in csrc/api_resample.hip) in
LONG-RUN launches against float64: resample_mfma_kernel<KS> (POLICY_RESAMPLE_FP32) for KS 16 / 48 / 80 / 104 / 112, the binary16-split
resample_f16_kernel<KS, 0, 0, 0> (4-byte operand reads) for the same five KS, and its 8-byte instantiations <KS, 0, 1, FULL> for
KS 80 / 104 / 112 with FULL = 1 (exact 64 x 2 x 30-piece chunk buffer) and FULL = 0 -- sixteen kernels.

Why: the workgroups are persistent -- each works through `chunks_per_block` consecutive chunks -- and the launcher takes
blocks = min(cu_count * per_cu, n_chunks), so chunks_per_block is 1 until a call has more chunks than workgroups: about 256 chunks
of 5 000 .. 19 000 input samples on 256 CUs.  Everything that only does something from the second chunk of a run onward (the two
LDS chunk buffers alternating by k & 1, the loaders holding chunk k + 2 in registers while k + 1 is staged and k is multiplied, the
chunk maximum in slot k % 3 that thread 0 zeroes behind the chunk's barrier, the monotonic arrival counter waited on with
n_loaders * (k / 3 + 1), chunk_src recomputing row / a0 / interior per chunk so that an edge chunk sits between two interior ones,
the FULL instantiations reading a few samples of the next chunk into the chunk maximum) was compared with an independent reference
in ONE instantiation (KS 104, 8-byte reads, FULL) at run positions 0 .. 6 of runs that start at a row start; the full-size
self-consistency test cannot see an error that both of its arms share.

launch_plan() is a host mirror of aamd_resample_prepared_f32 + rsm::plan_chunk + the kernels' chunk_src; every device run ASSERTS
the regime it claims from the mirror with the device's own CU count and LDS limit (another device fails loudly, it does not pass
vacuously), and the mirror's output length against the product's output shape.  Regimes (sized by the mirror from the CU count --
the smallest shapes that reach the code, not the workload's):

  long       rows of a whole number of chunks + a ragged tail, chunks_per_row coprime to chunks_per_block >= 5 (runs start and end
             inside rows; both buffers used twice, slots 0 and 1 reused, the counter waited on for its second round), n_chunks %
             chunks_per_block != 0 (the last run is shorter), about 4.3 x blocks chunks; FULL-capable pairs: the shortest rows that
             ARE full (10 chunks of 14 112 samples; 12 / 16 chunks for 35 : 15 / 25 : 15, whose chunk is shorter than the buffer).  Row gains cycle through 1, 1e-3, 1e-2, 1; one row is all zeros and must come out exactly zero
  one        ONE row of >= 5 x blocks chunks, once 16-byte aligned and once as a view that starts one sample in (vec_in off: every
             chunk takes load_piece, in the FULL kernels too)
  short      rows of 0.4 and of 1.3 chunks, chunks_per_block >= 5: every chunk is an edge chunk, a row boundary at every (every
             other) step of a run, qg / rounds reduced by the nq rule; this reaches the 8-byte NOT-FULL instantiations
  staircase  (f16 kernels) rows in which each chunk's gain is constant: one chunk at gain 1, four at QUIET_GAIN = 1e-9, repeating.  A quiet
             chunk is CLEAN when the mirror shows its whole buffer footprint [a0, a0 + buf_floats) inside quiet samples (the second
             and third quiet chunk behind a loud one); the third uses the loud chunk's maximum slot whenever both lie in one run:
             >= 20 such pairs per case and pass, asserted from the mirror.  FULL-capable pairs run it twice: in rows long enough
             to be FULL and in rows of 8 chunks (the 8-byte NOT-FULL instantiation with interior chunks)

Every case runs `long` plus two or three of the others (test_cases_cover_the_gaps lists what the 24 cases pin).

Reference: the reference implementation's own composition in float64 on the device -- pad (width, width + orig), correlate with
the module's own `kernel` at stride `orig` -- on the stored float32 waveform widened exactly, with the module's reduced rates, as
tests/test_gpu_fuzz.py::test_fuzz_resample_vs_reference_composition does with oracle.torch_cpu_ref.resample.  The SAME sums are
evaluated as a float64 matmul over an unfolded (as_strided) view of the padded rows, slab by slab: its cost is known in advance
(2 x taps x outputs flops, one unfolded copy per slab).  Timed once on the device, 1.06 M samples: matmul 0.3 / 0.2 / 1.1 ms,
pad + conv1d 2.3 / 0.4 / 1.3 ms (44.1k -> 16k kaiser_best / 48k -> 16k / 8k -> 16k kaiser_best) -- either would do; the matmul is
kept.  test_reference_forms_agree shows on the CPU, and test_reference_forms_agree_on_the_device on the device, that the two forms
give the same numbers (1e-13 of the peak).  Every output of every row is compared.

Bars (none is new, none is derived from the product's output):
  2e-5 peak-relative (test_fuzz_resample_vs_reference_composition), PER WAVEFORM ROW against that row's own reference peak: both
      kernel classes have scale-invariant error, a whole-tensor peak takes the gain of a quiet row off the margin
  staircase: over the outputs of each clean quiet chunk, 2e-5 x that window's own reference peak -- the quiet-part rule of
      tests/test_gpu_parity.py::test_resample_binary16_split_kernel_against_fp32_kernel_and_oracle
  the silent row: exactly 0.0
A failure names the worst element's locate() record (chunk in row, global chunk, workgroup, position k in the run, LDS buffer k & 1,
maximum slot k % 3, phase tile, launch pass, interior or edge), err / bar and the case's plan.

Two things the issue's text did not foresee.  (1) The staircase at a quiet gain of 1e-4 cannot see a stale maximum slot: the
kernel's hi / lo pair is FLOATING point (binary16 each), so a chunk scaled by a maximum 1e4 times too large loses nothing until its
samples fall under binary16's normal range.  The device cases, run at 1e-4 against a library without the slot's zeroing, all
passed; test_bite_staircase_honest_and_stale_scale replays the kernel's split on the CPU and moves QUIET_GAIN to 1e-9 (stale: 99 x
the bar, honest: 0.006 x).  (2) "The whole-tensor bar does not catch the quiet-row fault": resampling is LINEAR, so a chunk of a
quiet row computed from the previous row's samples is wrong by the row's gain (>= 1e-3) of the batch's peak -- 50 x the
whole-tensor bar and more, not under it (for the mel spectrogram, a power, the same fault is 1e-6).  What the whole-tensor
metric does is take the row's gain off the margin (test_bite_whole_tensor_metric_loses_the_rows_gain asserts exactly that), and
what it MISSES -- like the per-row bar -- is the stale maximum in a quiet passage: only the window bar sees that.

Device-free tests: the mirror's chunk geometry against rsm::plan_chunk itself through the CPU replay (sim_rsm_plan) for every case,
regime and launch pass at 256 CUs / 160 KiB and at 64 KiB, pick_ks against _host._rs_pick_ks, the coverage of the cases at the
design point, the two forms of the reference, and bite tests on small arrays with oracle/dsp_oracle.py (BITE_MEASURED).

Measured on an MI355X (256 CUs, 160 KiB LDS): MEASURED_DEVICE; wall time FILE_SECONDS.  No case found a kernel wrong: the worst
err / bar is 0.10 (resample_mfma_kernel<104>, short rows), 0.058 among the binary16-split kernels.  One observation for a later
issue, no fault: 16 k -> 22.05 k (320 : 441) plans a chunk of 2 565 pieces against the 2 560 its two loader waves hold in
registers, so EVERY chunk of that pair is staged through LDS (in_registers(); the mirror shows it, the results are right).

That the DEVICE cases bite was checked twice by hand against a library built with the zeroing of mx[k % kSlots] behind the chunk
barrier removed (the line above frag_build_kernel: the `mx` store only, counters and barriers left alone; in bounds, precision
only; that build is not committed).  At the issue's quiet gain of 1e-4 all 25 device tests PASSED against it -- the finding that
moved QUIET_GAIN.  At 1e-9 exactly the 15 cases with a staircase failed (every f16 case; 5-3-kb runs none), each in its first
staircase run at a clean window whose chunk sits three positions behind a loud one in the same run (run position 3 or 4, maximum
slot 0 or 1, loud_chunk_3_back_in_run True in every record) with err / bar 118 .. 158 (the CPU replay of the split says 99), in
interior and in edge chunks, in 4-byte, 8-byte and FULL kernels; the long / one / short runs of those cases, the eight fp32 cases and 5-3-kb passed.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

Q_PER_GROUP, LOADER_WAVES, SLOTS = 32, 2, 3                           # csrc/resample_mfma.h kQPerGroup, kLoaderWaves, kSlots
CU_DESIGN, LDS_DESIGN = 256, 160 * 1024
BAR = 2e-5
QUIET_GAIN = 1e-9           # see test_bite_staircase_honest_and_stale_scale: 1e-4 leaves a stale maximum invisible
POLICY_FP32, POLICY_B32 = 8, 128                                       # audio_amd/_lib.py POLICY_RESAMPLE_FP32, POLICY_RESAMPLE_B32

# measured on an MI355X (256 CUs, 160 KiB LDS), one run of this file with -s (24 cases, 111 runs, 134 figures, all passed): kernel family ->
# (worst err / bar, its case, regime, layout) from the "[fuzz-resample]" lines; "clean windows" = the staircase's window bar
MEASURED_DEVICE = {
    "fp32 KS 16": (0.023, "48k-16k-fp32", "short", "aligned"), "fp32 KS 48": (0.044, "8k-16k-kb-fp32", "short", "aligned"),
    "fp32 KS 80": (0.064, "22k-16k-kb-fp32", "short", "aligned"), "fp32 KS 104": (0.100, "44k-16k-kb-fp32", "short", "aligned"),
    "fp32 KS 112": (0.088, "48k-16k-kb-fp32", "short", "aligned"),
    "f16 KS 16 b32": (0.027, "22k-16k", "short", "aligned"), "f16 KS 16 b32 clean windows": (0.028, "22k-16k", "staircase", "aligned"),
    "f16 KS 48 b32": (0.028, "48k-16k-w16", "long", "aligned"), "f16 KS 48 b32 clean windows": (0.031, "48k-16k-w16", "staircase", "aligned"),
    "f16 KS 80 b32": (0.042, "16k-8k-kb", "long", "aligned"), "f16 KS 80 b32 clean windows": (0.041, "16k-8k-kb", "staircase", "aligned"),
    "f16 KS 104 b32": (0.053, "44k-16k-kb-b32", "long", "aligned"),
    "f16 KS 104 b32 clean windows": (0.046, "44k-16k-kb-b32", "staircase", "aligned"),
    "f16 KS 112 b32": (0.055, "48k-16k-kb", "long", "aligned"), "f16 KS 112 b32 clean windows": (0.040, "48k-16k-kb", "staircase", "aligned"),
    "f16 KS 80 b64": (0.044, "22k-16k-kb", "short", "aligned"), "f16 KS 80 b64 clean windows": (0.039, "22k-16k-kb", "staircase", "aligned"),
    "f16 KS 80 b64 FULL": (0.043, "22k-16k-kb", "staircase", "aligned"),
    "f16 KS 80 b64 FULL clean windows": (0.045, "22k-16k-kb", "staircase", "aligned"),
    "f16 KS 104 b64": (0.040, "44k-16k-kb", "staircase", "aligned"), "f16 KS 104 b64 clean windows": (0.053, "44k-16k-kb", "staircase", "aligned"),
    "f16 KS 104 b64 FULL": (0.047, "44k-16k-kb", "long", "aligned"),
    "f16 KS 104 b64 FULL clean windows": (0.054, "44k-16k-kb", "staircase", "aligned"),
    "f16 KS 112 b64": (0.051, "44k-16k-k64r9", "short", "aligned"),
    "f16 KS 112 b64 clean windows": (0.044, "44k-16k-k64r9", "staircase", "aligned"),
    "f16 KS 112 b64 FULL": (0.058, "44k-16k-k64r9", "long", "aligned"),
    "f16 KS 112 b64 FULL clean windows": (0.053, "44k-16k-k64r9", "staircase", "aligned"),
}
# the 25 device tests together: 4.3 s of pytest wall time (0.6 s for the first case, which loads the library and builds the first
# module; 0.01 .. 0.05 s for the others: a run of 10 .. 24 M samples is milliseconds of device time) -- 1 % on top of the 404 s the
# device suite took at the parent commit (420 s with them, 1 251 tests)
FILE_SECONDS = 4.3


# --------------------------------------------------------------------------- #
# 1. the host mirror of the launch arithmetic                                 #
# --------------------------------------------------------------------------- #

def pick_ks(span, orig=0):
    """rsm::pick_ks."""
    need = (span + 3) // 4
    if need <= 16:
        return 16
    if need <= 48:
        return 48
    if need <= 80:
        return 80
    if need <= 104 and (orig & 1):
        return 104
    if need <= 112:
        return 112
    return 0


def max_compute_waves(ks):
    return 10 if ks >= 80 else 14


def pieces_per_lane(ks):
    return 30 if ks >= 80 else 20


def buf_floats_needed(qc, orig, taps, max_lo, ks):
    reach = max(max_lo + 4 * ks, taps)
    return ((qc - 1) * orig + reach + 3 + 3) & ~3


def plan_chunk(n_pt, ks, f16, nq, max_lo, orig, taps, lds_cap):
    """rsm::plan_chunk: dict(ok, qg, rounds, n_loaders, buf_floats)."""
    qg = max_compute_waves(ks) // n_pt
    while qg > 1 and Q_PER_GROUP * (qg - 1) >= nq:
        qg -= 1
    rounds, n_loaders = 1, LOADER_WAVES
    if f16 and ks < 80 and n_pt * qg + 4 <= 16:
        n_loaders = 4

    def fits(q_groups):
        fl = buf_floats_needed(Q_PER_GROUP * q_groups, orig, taps, max_lo, ks)
        if 2 * fl * 4 + 48 > lds_cap:
            return False
        return (not f16) or fl <= 4 * 64 * n_loaders * pieces_per_lane(ks)

    while qg > 1 and not fits(qg):
        qg -= 1
    if f16:
        while rounds < 8 and Q_PER_GROUP * qg * rounds < nq and fits(qg * (rounds + 1)):
            rounds += 1
    buf = buf_floats_needed(Q_PER_GROUP * qg * rounds, orig, taps, max_lo, ks)
    if f16 and ks >= 80 and n_loaders == LOADER_WAVES:
        full = 4 * 64 * LOADER_WAVES * pieces_per_lane(ks)
        if buf <= full and nq * orig >= 8 * full and 2 * full * 4 + 48 <= lds_cap:
            buf = full
    return dict(ok=2 * buf * 4 + (48 if f16 else 0) <= lds_cap, qg=qg, rounds=rounds, n_loaders=n_loaders, buf_floats=buf)


def launch_plan(rows, length, orig, new, width, tap_lo, span, *, fp32=False, b32=False, in_aligned=True, row_stride=None,
                out_aligned=True, cu_count=CU_DESIGN, lds_cap=LDS_DESIGN):
    """aamd_resample_prepared_f32 for `rows` rows of `length` samples; orig / new / width and the band table (tap_lo per tile of
    16 phases, span) are the call's, i.e. after _host.resample_fill_phase_tiles.  fp32 / b32: the policy flags; in_aligned /
    out_aligned: the pointers are 16-byte aligned; row_stride defaults to what functional._polyphase passes.  One dict per launch
    pass in ["passes"]; ["generic"] when the call falls back to the scalar kernel."""
    if lds_cap == 0:
        lds_cap = 64 * 1024
    if row_stride is None:
        row_stride = max(length, 1)
    out_len = (new * length + orig - 1) // orig
    n_tiles = (new + 15) // 16
    assert len(tap_lo) == n_tiles, (len(tap_lo), n_tiles)
    ks = pick_ks(span, orig)
    taps = 2 * width + orig
    nq = (out_len + new - 1) // new
    plan = dict(rows=rows, length=length, orig=orig, new=new, width=width, taps=taps, out_len=out_len, nq=nq, ks=ks, n_tiles=n_tiles,
                f16=not fp32, vec_in=bool(in_aligned and row_stride % 4 == 0),
                vec_out=bool(out_aligned and out_len % 4 == 0 and new % 4 == 0), cu_count=cu_count, lds_cap=lds_cap,
                generic=ks == 0, passes=[])
    if ks == 0 or rows == 0 or out_len == 0:
        return plan
    f16 = not fp32
    max_cw = max_compute_waves(ks)
    rd64 = f16 and (orig & 1) == 1 and ks in (80, 104, 112) and not b32
    for pt0 in range(0, n_tiles, max_cw):
        n_pt = min(n_tiles - pt0, max_cw)
        max_lo = max([0] + [int(v) for v in tap_lo[pt0:pt0 + n_pt]])
        c = plan_chunk(n_pt, ks, f16, nq, max_lo, orig, taps, lds_cap)
        if not c["ok"]:
            plan["generic"] = True
            return plan
        qg, rounds, n_loaders, buf = c["qg"], c["rounds"], c["n_loaders"], c["buf_floats"]
        qc = Q_PER_GROUP * qg * rounds
        lds = 2 * buf * 4 + (48 if f16 else 0)
        cpr = (nq + qc - 1) // qc
        n_chunks = rows * cpr
        wg_waves = n_pt * qg + n_loaders
        per_cu = 1 if ks >= 80 else 16 // wg_waves
        per_cu = max(1, min(per_cu, lds_cap // lds))
        blocks = min(cu_count * per_cu, n_chunks)
        cpb = (n_chunks + blocks - 1) // blocks
        blocks = (n_chunks + cpb - 1) // cpb
        full = rd64 and ks >= 80 and n_loaders == LOADER_WAVES and buf == 4 * 64 * LOADER_WAVES * pieces_per_lane(ks)
        kernel = ("fp32", ks, 4, False) if fp32 else ("f16", ks, 8 if rd64 else 4, bool(full))
        plan["passes"].append(dict(pt0=pt0, n_pt=n_pt, max_lo=max_lo, qg=qg, rounds=rounds, n_loaders=n_loaders, buf_floats=buf,
                                   chunk_q=qc, lds=lds, rd64=bool(rd64), full=bool(full), kernel=kernel, chunks_per_row=cpr,
                                   n_chunks=n_chunks, per_cu=per_cu, blocks=blocks, chunks_per_block=cpb, threads=64 * wg_waves))
    return plan


def chunk_a0(plan, p, chunk_in_row):
    """rsm::chunk_a0: sample index of LDS float 0 of the chunk (16-byte phase aligned with global memory when vec_in)."""
    s = chunk_in_row * plan["passes"][p]["chunk_q"] * plan["orig"] - plan["width"]
    return s - (s % 4) if plan["vec_in"] else s


def in_registers(plan, p):
    """Does a whole chunk of pass p fit the registers of the f16 kernel's loader waves (the fp32 kernel's load_chunk has no limit)?"""
    ps = plan["passes"][p]
    return (not plan["f16"]) or ps["buf_floats"] // 4 <= 64 * ps["n_loaders"] * pieces_per_lane(plan["ks"])


def chunk_interior(plan, p, chunk_in_row):
    """The loaders' `interior` (chunk_src / load_chunk): fetched without index checks, in the f16 kernels converted from registers;
    otherwise an edge chunk, staged through LDS with zero padding by index."""
    ps = plan["passes"][p]
    a0 = chunk_a0(plan, p, chunk_in_row)
    return bool(plan["vec_in"] and a0 >= 0 and a0 + ps["buf_floats"] <= plan["length"] and in_registers(plan, p))


def locate(plan, row, oi):
    """Where the launch computes output `oi` of row `row`."""
    q, phase = divmod(oi, plan["new"])
    tile = phase // 16
    p = tile // max_compute_waves(plan["ks"])
    ps = plan["passes"][p]
    c = q // ps["chunk_q"]
    g = row * ps["chunks_per_row"] + c
    wg, k = divmod(g, ps["chunks_per_block"])
    run = min(ps["chunks_per_block"], ps["n_chunks"] - wg * ps["chunks_per_block"])
    return dict(row=row, out=oi, q=q, phase=phase, phase_tile=tile, launch_pass=p, chunk_in_row=c, chunk=g, workgroup=wg, k=k,
                run_length=run, lds_buffer=k & 1, max_slot=k % SLOTS, interior=chunk_interior(plan, p, c), kernel=ps["kernel"])


def regime_fault(name, plan, full_capable=False):
    """None when `plan` is in regime `name`, else what it misses (the condition every run asserts on the mirror's plan)."""
    if plan["generic"] or not plan["passes"]:
        return "scalar fall-back"
    for p, ps in enumerate(plan["passes"]):
        cpr, cpb, n = ps["chunks_per_row"], ps["chunks_per_block"], ps["n_chunks"]
        if cpb < 5:
            return f"pass {p}: chunks_per_block {cpb} < 5"
        if name in ("long", "staircase"):
            if plan["rows"] < 2 or cpr < 2:
                return f"pass {p}: rows {plan['rows']}, chunks_per_row {cpr}"
            if math.gcd(cpr, cpb) != 1:
                return f"pass {p}: chunks_per_row {cpr} not coprime to chunks_per_block {cpb}"
            if n % cpb == 0:
                return f"pass {p}: the last run is not shorter ({n} % {cpb})"
            if full_capable and not ps["full"]:
                return f"pass {p}: rows too short for the FULL instantiation (chunks_per_row {cpr})"
            # (a chunk of more pieces than the loader waves hold in registers is staged through LDS wherever it lies: 16 k -> 22.05 k)
            if plan["vec_in"] and in_registers(plan, p) and not any(chunk_interior(plan, p, c) for c in range(cpr)):
                return f"pass {p}: no interior chunk"
        elif name == "one":
            if plan["rows"] != 1 or n < 5 * plan["cu_count"] * ps["per_cu"]:
                return f"pass {p}: rows {plan['rows']}, {n} chunks on {ps['blocks']} workgroups"
        elif name == "short":
            if cpr > 2 or ps["full"] or n % cpb == 0:
                return f"pass {p}: chunks_per_row {cpr}, full {ps['full']}, {n} % {cpb}"
            if any(chunk_interior(plan, p, c) for c in range(cpr)):
                return f"pass {p}: an interior chunk"
        else:
            raise KeyError(name)
    return None


# --------------------------------------------------------------------------- #
# 2. the cases                                                                #
# --------------------------------------------------------------------------- #

KB = dict(resampling_method="sinc_interp_kaiser", lowpass_filter_width=64, rolloff=0.9475937167399596, beta=14.769656459379492)
PAIRS = {
    "48k-16k": (48000, 16000, {}),                                    # KS 16: 3 : 1 filled to 30 : 10, one phase tile, qg 10
    "48k-44k": (48000, 44100, {}),                                    # KS 16: 10 tiles, 4 loaders, rounds 3
    "16k-22k": (16000, 22050, {}),                                    # KS 16: 28 tiles, two launches of 14
    "22k-16k": (22050, 16000, {}),                                    # KS 16: 20 tiles, launches of 14 and 6 (the second with 4 loaders)
    "44k-16k": (44100, 16000, {}),                                    # KS 48: 10 tiles, 4 loaders
    "8k-16k-kb": (8000, 16000, KB),                                   # KS 48: qg 14, rounds 2
    "48k-16k-w16": (48000, 16000, dict(lowpass_filter_width=16)),     # KS 48: qg 6, per_cu 2
    "16k-8k-kb": (16000, 8000, KB),                                   # KS 80: 32 : 16, even orig
    "22k-16k-kb": (22050, 16000, KB),                                 # KS 80: 441 : 320, 8-byte reads, two launches of 10
    "5-3-kb": (5, 3, KB),                                             # KS 80: 25 : 15, 8-byte reads, one tile, qg 10
    "44k-16k-kb": (44100, 16000, KB),                                 # KS 104: BASELINE config 3
    "7-3-kb": (7, 3, KB),                                             # KS 104: 35 : 15, one tile
    "48k-16k-kb": (48000, 16000, KB),                                 # KS 112: 36 : 12, even orig
    "44k-16k-k64r9": (44100, 16000, dict(KB, rolloff=0.9)),           # KS 112: span 434, odd orig, 8-byte reads
}


def _c(pair, policy=0, others=None):
    name = pair + {0: "", POLICY_FP32: "-fp32", POLICY_B32: "-b32"}[policy]
    return dict(id=name, pair=pair, policy=policy, others=others)


CASES = [
    # the binary16-split kernels as the product picks them
    _c("48k-16k"), _c("48k-44k"), _c("16k-22k"), _c("22k-16k"),
    _c("44k-16k"), _c("8k-16k-kb"), _c("48k-16k-w16"),
    _c("16k-8k-kb"), _c("22k-16k-kb", others=("short", "staircase")), _c("5-3-kb", others=("one", "short")),
    _c("44k-16k-kb", others=("one", "staircase")), _c("7-3-kb", others=("short", "staircase")),
    _c("48k-16k-kb"), _c("44k-16k-k64r9", others=("one", "short", "staircase")),
    # 4-byte reads where the product would take the 8-byte layout: the only way to resample_f16_kernel<104, 0, 0, 0>
    _c("44k-16k-kb", POLICY_B32, others=("short", "staircase")), _c("7-3-kb", POLICY_B32, others=("one", "staircase")),
    # the exact-fp32 matrix-core kernels
    _c("48k-16k", POLICY_FP32), _c("22k-16k", POLICY_FP32), _c("44k-16k", POLICY_FP32), _c("8k-16k-kb", POLICY_FP32),
    _c("5-3-kb", POLICY_FP32), _c("22k-16k-kb", POLICY_FP32), _c("44k-16k-kb", POLICY_FP32), _c("48k-16k-kb", POLICY_FP32),
]
CASE_IDS = [c["id"] for c in CASES]
# the regimes a case runs besides `long`, by its index (or the case's own `others`); fp32 kernels have no chunk maximum: no staircase
OTHERS_F16 = (("one", "staircase"), ("short", "staircase"))
OTHERS_FP32 = (("one", "short"),)
SEED_BASE = 52500
GAINS = (1.0, 1e-3, 1e-2, 1.0)

_GEOM = {}


def geometry(pair, kernel=None):
    """What functional._polyphase passes to the launcher for rate pair `pair`: the reduced rates after
    _host.resample_fill_phase_tiles, the band table of the filled tap table, and the unfilled kernel (float64, (new0, taps0)) with
    its reduced rates for the reference.  `kernel`: the module's own buffer (device test); None: built on the host the way
    T.Resample builds it."""
    if pair in _GEOM and kernel is None:
        return _GEOM[pair]
    from audio_amd import _host
    orig_freq, new_freq, kw = PAIRS[pair]
    gcd = math.gcd(orig_freq, new_freq)
    built, width = _host.sinc_resample_kernel(orig_freq, new_freq, gcd, kw.get("lowpass_filter_width", 6), kw.get("rolloff", 0.99),
                                              kw.get("resampling_method", "sinc_interp_hann"), kw.get("beta"), dtype=None)
    orig0, new0 = orig_freq // gcd, new_freq // gcd
    built = built.reshape(new0, -1)
    if kernel is not None:
        assert torch.equal(kernel.reshape(new0, -1).cpu(), built), pair
    kp, m = _host.resample_fill_phase_tiles(built.numpy(), orig0, new0, width)
    tap_lo, span = _host.resample_band_table(built.numpy() if m == 1 else kp)
    g = dict(pair=pair, orig0=orig0, new0=new0, width=width, m=m, orig=m * orig0, new=m * new0, tap_lo=[int(v) for v in tap_lo],
             span=int(span), kernel64=built.double(), taps0=built.shape[1])
    _GEOM[pair] = g
    return g


def _plan(case, rows, length, cu, lds_cap, in_aligned=True):
    g = geometry(case["pair"])
    return launch_plan(rows, length, g["orig"], g["new"], g["width"], g["tap_lo"], g["span"], fp32=case["policy"] == POLICY_FP32,
                       b32=case["policy"] == POLICY_B32, in_aligned=in_aligned, cu_count=cu, lds_cap=lds_cap)


def _full_capable(case, cu, lds_cap):
    return all(ps["full"] for ps in _plan(case, 1, 10 ** 8, cu, lds_cap)["passes"])


def _tune_length(case, base, want_vec_in, want_vec_out):
    """The first length >= base whose 16-byte phase (length % 4 == 0: a contiguous batch, or a single row, is vec_in) and output
    length (out_len % 4 == 0, where new % 4 == 0) are as wanted."""
    g = geometry(case["pair"])
    first = None
    for d in range(0, 8 * g["orig"] + 8):
        n = base + d
        if (n % 4 == 0) != want_vec_in:
            continue
        first = n if first is None else first
        out_len = (g["new"] * n + g["orig"] - 1) // g["orig"]
        if g["new"] % 4 != 0 or (out_len % 4 == 0) == want_vec_out:
            return n
    return first


def draw_runs(idx, cu=CU_DESIGN, lds_cap=LDS_DESIGN):
    """The runs of case `idx` on a device with `cu` CUs and an LDS limit of `lds_cap`: dict(regime, rows, length, offset, seed)
    -- sized by the mirror, a function of (idx, cu, lds_cap) alone."""
    case = CASES[idx]
    g = geometry(case["pair"])
    fp32 = case["policy"] == POLICY_FP32
    others = case["others"] or (OTHERS_FP32[idx % len(OTHERS_FP32)] if fp32 else OTHERS_F16[idx % len(OTHERS_F16)])
    inf = _plan(case, 1, 10 ** 8, cu, lds_cap)
    assert not inf["generic"], case
    qc0 = inf["passes"][0]["chunk_q"]
    max_blocks = max(cu * ps["per_cu"] for ps in inf["passes"])
    full_capable = all(ps["full"] for ps in inf["passes"])
    want_in, want_out = idx % 2 == 0, idx % 3 != 0
    runs = []

    def many_rows(regime, cpr_choices, tail, j, full=full_capable):
        target = math.ceil(4.3 * max_blocks)
        for cpr in cpr_choices:
            length = _tune_length(case, int(((cpr - 1) + tail) * qc0 * g["orig"]), regime == "long" or want_in, want_out)
            for rows in range(max(2, -(-target // cpr)), -(-target // cpr) + 64):
                plan = _plan(case, rows, length, cu, lds_cap, in_aligned=True)
                if regime_fault(regime, plan, full) is None and all(ps["full"] == full for ps in plan["passes"]):
                    runs.append(dict(regime=regime, rows=rows, length=length, offset=0, full=full,
                                     seed=SEED_BASE + 100 * idx + 10 * j + (0 if full == full_capable else 5)))
                    return
        raise AssertionError((case["id"], regime, "no shape found", cu, lds_cap))

    many_rows("long", range(9, 24) if full_capable else (7, 9, 11, 6, 8), 0.37, 0)
    for j, regime in enumerate(others, 1):
        if regime == "one":
            qc_max = max(ps["chunk_q"] for ps in inf["passes"])
            length = _tune_length(case, int((5 * max_blocks + 0.37) * qc_max * g["orig"]), True, want_out)
            for offset in (0, 1):
                runs.append(dict(regime="one", rows=1, length=length, offset=offset, seed=SEED_BASE + 100 * idx + 10 * j + offset))
        elif regime == "short":
            for i, frac in enumerate((0.4, 1.3)):
                length = _tune_length(case, int(frac * qc0 * g["orig"]), want_in ^ (i == 1), want_out)
                for rows in range(2, 40 * max_blocks):
                    plan = _plan(case, rows, length, cu, lds_cap)
                    if plan["passes"] and min(ps["n_chunks"] for ps in plan["passes"]) < 4.3 * max_blocks:
                        continue
                    if regime_fault("short", plan) is None:
                        runs.append(dict(regime="short", rows=rows, length=length, offset=0, seed=SEED_BASE + 100 * idx + 10 * j + i))
                        break
                else:
                    raise AssertionError((case["id"], "short", frac, "no shape found"))
        else:
            many_rows("staircase", (11, 12, 13, 16, 17, 18, 19, 21) if full_capable else (11, 12, 13), 0.37, j)
            if full_capable:          # rows of 8 chunks are too short for the FULL instantiation: the 8-byte NOT-FULL one
                many_rows("staircase", (8, 7, 6), 0.37, j, full=False)
    return runs


def run_plan(case, run, cu, lds_cap):
    """The mirror's plan of a run as its layout gives it by construction (the device test asserts the alignment on the pointers)."""
    return _plan(case, run["rows"], run["length"], cu, lds_cap, in_aligned=run["offset"] == 0)


# --------------------------------------------------------------------------- #
# 3. the staircase                                                            #
# --------------------------------------------------------------------------- #

def stair_region(plan):
    """Samples per step of the staircase: pass 0's chunk."""
    return plan["passes"][0]["chunk_q"] * plan["orig"]


def stair_loud(plan, row, sample):
    """Is `sample` of `row` at gain 1?  Step s of a row covers the samples [s R - width, (s + 1) R - width): what chunk s of pass 0
    starts with; one step in five is loud, shifted by two steps from row to row so that loud chunks sit at every run position."""
    return ((sample + plan["width"]) // stair_region(plan) + 2 * row) % 5 == 0


def stair_chunks(plan, p):
    """(loud, clean) boolean arrays (rows, chunks_per_row) of pass p: the chunk's footprint [a0, a0 + buf_floats), cut to the row,
    holds a loud sample / only quiet ones."""
    ps = plan["passes"][p]
    R, width, length = stair_region(plan), plan["width"], plan["length"]
    rows, cpr = plan["rows"], ps["chunks_per_row"]
    loud = np.zeros((rows, cpr), dtype=bool)
    for c in range(cpr):
        a0 = chunk_a0(plan, p, c)
        lo, hi = max(a0, 0), min(a0 + ps["buf_floats"], length)
        if hi <= lo:
            continue
        steps = np.arange((lo + width) // R, (hi - 1 + width) // R + 1)
        loud[:, c] = (((steps[None, :] + 2 * np.arange(rows)[:, None]) % 5) == 0).any(1)
    return loud, ~loud


def stair_pairs(plan, p):
    """(loud chunk g, clean chunk g + 3) pairs of pass p inside one run: the clean chunk reuses the loud one's maximum slot."""
    ps = plan["passes"][p]
    loud, clean = stair_chunks(plan, p)
    loud, clean = loud.reshape(-1), clean.reshape(-1)
    g = np.arange(ps["n_chunks"] - 3)
    same_run = g // ps["chunks_per_block"] == (g + 3) // ps["chunks_per_block"]
    return int((loud[:-3] & clean[3:] & same_run).sum())


# --------------------------------------------------------------------------- #
# 4. the reference and the checks (torch, on whatever device the tensors are) #
# --------------------------------------------------------------------------- #

SLAB_DOUBLES = 1 << 26


def reference64(x, kernel64, orig, new, width, out_len):
    """(rows, length) float32 or float64 -> (rows, nq * new) float64 with nq = ceil(out_len / new), outputs past out_len zeroed:
    y[q new + p] = sum_k kernel[p][k] xpad[q orig + k], xpad = x padded by (width, width + orig) -- oracle.torch_cpu_ref.resample's
    conv1d, evaluated as a matmul over an unfolded view of the padded rows, one slab of (rows, q) at a time."""
    rows, length = x.shape
    taps = kernel64.shape[1]
    assert kernel64.shape[0] == new and taps == 2 * width + orig
    nq = -(-out_len // new)
    xp = torch.nn.functional.pad(x.double(), (width, width + orig))
    Lp = xp.shape[1]
    assert (nq - 1) * orig + taps <= Lp
    kT = kernel64.t().contiguous()
    ref = torch.empty((rows, nq, new), dtype=torch.float64, device=x.device)
    q_step = max(1, min(nq, SLAB_DOUBLES // taps))
    r_step = max(1, SLAB_DOUBLES // (taps * q_step))
    for ra in range(0, rows, r_step):
        rb = min(rows, ra + r_step)
        for qa in range(0, nq, q_step):
            qb = min(nq, qa + q_step)
            win = xp.as_strided((rb - ra, qb - qa, taps), (Lp, orig, 1), xp.storage_offset() + ra * Lp + qa * orig)
            ref[ra:rb, qa:qb] = (win.reshape(-1, taps) @ kT).view(rb - ra, qb - qa, new)
    ref = ref.view(rows, nq * new)
    ref[:, out_len:] = 0.0
    return ref


def pad_outputs(got, nq, new):
    return torch.nn.functional.pad(got, (0, nq * new - got.shape[1]))


def row_errors(got, ref):
    """(rows, n) x 2 -> per row max|got - ref| / max|ref of that row|, and the index of each row's worst element."""
    d = (got.double() - ref).abs()
    e, where = d.max(1)
    peak = ref.abs().amax(1)
    return torch.where(peak > 0, e / peak.clamp_min(1e-300), e), where


def whole_tensor_error(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max())


def window_errors(got, ref, plan, p):
    """Per (row, chunk of pass p): max|got - ref| over the chunk's outputs of pass p's phase tiles, and the window's reference peak."""
    ps = plan["passes"][p]
    rows, new, nq, qc, cpr = plan["rows"], plan["new"], plan["nq"], ps["chunk_q"], ps["chunks_per_row"]
    p0, p1 = 16 * ps["pt0"], min(new, 16 * (ps["pt0"] + ps["n_pt"]))
    pad = cpr * qc - nq

    def windows(t):
        t = t.view(rows, nq, new)[:, :, p0:p1]
        return torch.nn.functional.pad(t, (0, 0, 0, pad)).reshape(rows, cpr, qc * (p1 - p0))

    g, r = windows(got.double()), windows(ref)
    return (g - r).abs().amax(2), r.abs().amax(2)


_WORST = {}


def _note(family, cid, run, what, err, bar, where):
    ratio = err / bar if bar > 0 else (0.0 if err == 0 else float("inf"))
    if ratio >= _WORST.get(family, (-1.0,))[0]:
        _WORST[family] = (ratio, cid, run["regime"], "aligned" if run.get("offset", 0) == 0 else "one sample in")
    print(f"[fuzz-resample] {family} {cid} {run['regime']} rows={run['rows']} L={run['length']} off={run.get('offset', 0)} {what}: "
          f"err={err:.3e} bar={bar:.3e} err/bar={ratio:.3f} (worst so far {_WORST[family][0]:.3f} {_WORST[family][1:]}) at {where}")


def family_of(kernel):
    cls, ks, rd, full = kernel
    return f"fp32 KS {ks}" if cls == "fp32" else f"f16 KS {ks} b{rd * 8}" + (" FULL" if full else "")


def assert_rows_close(got, ref, plan, cid, run, bar=BAR):
    """The 2e-5 bar per waveform row against that row's own reference peak; a silent row's bar is 0."""
    rel, where = row_errors(got, ref)
    r = int(rel.argmax())
    err = float(rel[r])
    loc = locate(plan, r, int(where[r]))
    _note(family_of(loc["kernel"]), cid, run, "per-row", err, bar, loc)
    assert err <= bar, (cid, run, "per-row", err, bar, err / bar, loc, plan)


def assert_clean_windows_close(got, ref, plan, cid, run, bar=BAR):
    """The quiet-part rule over the outputs of every clean quiet chunk of every pass."""
    n_clean = 0
    for p, ps in enumerate(plan["passes"]):
        err, peak = window_errors(got, ref, plan, p)
        clean = torch.from_numpy(stair_chunks(plan, p)[1]).to(err.device)
        assert bool((peak[clean] > 0).all()), (cid, run, p, "a clean window without signal")
        ratio = torch.where(clean, err / peak.clamp_min(1e-300), torch.zeros_like(err))
        i = int(ratio.argmax())
        row, c = divmod(i, ps["chunks_per_row"])
        loc = locate(plan, row, c * ps["chunk_q"] * plan["new"] + 16 * ps["pt0"])
        g = loc["chunk"]
        loud = stair_chunks(plan, p)[0].reshape(-1)
        loc["loud_chunk_3_back_in_run"] = bool(loc["k"] >= 3 and loud[g - 3])
        n_clean += int(clean.sum())
        _note(family_of(ps["kernel"]), cid, run, f"clean windows pass {p} ({int(clean.sum())})", float(ratio.reshape(-1)[i]), bar, loc)
        assert float(ratio.reshape(-1)[i]) <= bar, (cid, run, "clean window", float(ratio.reshape(-1)[i]), bar, loc, plan)
    return n_clean


# --------------------------------------------------------------------------- #
# 5. the device tests                                                         #
# --------------------------------------------------------------------------- #

HIP_ATTR_CU_COUNT, HIP_ATTR_LDS_PER_BLOCK, HIP_ATTR_LDS_PER_BLOCK_OPTIN = 63, 74, 75      # hip_runtime_api.h hipDeviceAttribute_t (ROCm 7)


def device_limits():
    """(cu_count, lds_cap) as csrc/api_common.hip reads them: multiProcessorCount and sharedMemPerBlockOptin (0: sharedMemPerBlock).
    torch's device properties carry the first; the second is asked of the HIP runtime the process has loaded, and the attribute
    numbering is checked against the two values torch does carry.  The CU count is also checked against aamd_device_info."""
    from audio_amd import _lib
    props = torch.cuda.get_device_properties(0)
    cu = int(props.multi_processor_count)
    name, cus, mem = C.create_string_buffer(128), C.c_int32(0), C.c_int64(0)
    _lib.check(_lib.lib().aamd_device_info(name, 128, C.byref(cus), C.byref(mem)))
    assert cus.value == cu, (cus.value, cu)
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line}, key=lambda p: ("torch" in p, p))
    assert paths, "no HIP runtime in this process"
    hip = C.CDLL(paths[0])
    hip.hipDeviceGetAttribute.argtypes = [C.POINTER(C.c_int), C.c_int, C.c_int]

    def attr(a):
        v = C.c_int(-1)
        assert hip.hipDeviceGetAttribute(C.byref(v), a, torch.cuda.current_device()) == 0, a
        return int(v.value)

    assert attr(HIP_ATTR_CU_COUNT) == cu and attr(HIP_ATTR_LDS_PER_BLOCK) == int(props.shared_memory_per_block), \
        ("hipDeviceAttribute_t numbering", attr(HIP_ATTR_CU_COUNT), cu, attr(HIP_ATTR_LDS_PER_BLOCK), props.shared_memory_per_block)
    optin = attr(HIP_ATTR_LDS_PER_BLOCK_OPTIN)
    lds_cap = optin if optin > 0 else int(props.shared_memory_per_block)
    assert lds_cap % 1024 == 0 and 32 * 1024 <= lds_cap <= 1024 * 1024, lds_cap
    return cu, lds_cap


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from audio_amd import _lib
    _lib.lib()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def limits(dev):
    return device_limits()


_MODULES = {}


def _module(pair):
    import audio_amd.transforms as T
    if pair not in _MODULES:
        orig_freq, new_freq, kw = PAIRS[pair]
        _MODULES[pair] = T.Resample(orig_freq, new_freq, **kw).cuda()
    return _MODULES[pair]


def device_wave(run, plan, dev):
    """float32 (rows, length) on the device: clipped noise at 0.5; `offset` samples past a 16-byte boundary.  long / short: row r
    times GAINS[r % 4], in `long` row rows // 2 is all zeros; staircase: the steps of stair_loud."""
    rows, length, off = run["rows"], run["length"], run["offset"]
    flat = torch.empty(rows * length + 8, dtype=torch.float32, device=dev)
    x = flat[off:off + rows * length]
    x.normal_(generator=torch.Generator(device=dev).manual_seed(run["seed"]))
    x.mul_(0.5).clamp_(-1.0, 1.0)
    x = x.view(rows, length)
    if run["regime"] == "staircase":
        steps = (torch.arange(length, device=dev) + plan["width"]) // stair_region(plan)
        loud = (steps[None, :] + 2 * torch.arange(rows, device=dev)[:, None]) % 5 == 0
        x.mul_(torch.where(loud, 1.0, QUIET_GAIN).float())
    elif rows > 1:
        x.mul_(torch.tensor([GAINS[r % len(GAINS)] for r in range(rows)], device=dev)[:, None])
        if run["regime"] == "long":
            x[rows // 2] = 0.0
    return x


def run_product(case, x):
    from audio_amd import _lib
    t = _module(case["pair"])
    with torch.no_grad():
        if case["policy"]:
            with _lib.kernel_policy(case["policy"]):
                return t(x)
        return t(x)


def check_run(case, run, cu, lds_cap, dev):
    """One run: the regime asserted on the mirror with the device's numbers, the product against float64.  Returns the plan."""
    g = geometry(case["pair"], _module(case["pair"]).kernel)
    plan = run_plan(case, run, cu, lds_cap)
    fault = regime_fault(run["regime"], plan, run.get("full", False))
    assert fault is None, (case["id"], run, fault, f"{cu} CUs, {lds_cap} bytes of LDS", plan)
    if run["regime"] == "staircase":
        assert all(ps["full"] == run["full"] for ps in plan["passes"]), (case["id"], run, plan)
        pairs = [stair_pairs(plan, p) for p in range(len(plan["passes"]))]
        assert min(pairs) >= 20, (case["id"], run, pairs)
    x = device_wave(run, plan, dev)
    assert (x.data_ptr() % 16 == 0) == (run["offset"] == 0), (case["id"], run)
    assert plan["vec_in"] == (x.data_ptr() % 16 == 0 and plan["length"] % 4 == 0), (case["id"], run)
    got = run_product(case, x)
    assert got.shape == (run["rows"], plan["out_len"]), (got.shape, plan["out_len"], case["id"], run)
    assert got.data_ptr() % 16 == 0 and got.is_contiguous()
    ref = reference64(x, g["kernel64"].to(dev), g["orig0"], g["new0"], g["width"], plan["out_len"])[:, :plan["out_len"]]
    ref = pad_outputs(ref, plan["nq"], plan["new"])
    got = pad_outputs(got, plan["nq"], plan["new"])
    assert bool(torch.isfinite(got).all()), (case["id"], run)
    if run["regime"] == "long":
        silent = run["rows"] // 2
        assert float(ref[silent].abs().max()) == 0.0
        assert float(got[silent].abs().max()) == 0.0, (case["id"], run, "the silent row", locate(plan, silent, int(got[silent].abs().argmax())))
    assert_rows_close(got, ref, plan, case["id"], run)
    if run["regime"] == "staircase":
        n_clean = assert_clean_windows_close(got, ref, plan, case["id"], run)
        print(f"[fuzz-resample] {case['id']} staircase full={run['full']}: (loud k, clean k + 3) pairs per pass {pairs}, {n_clean} clean windows")
    return plan


@pytest.mark.gpu
def test_reference_forms_agree_on_the_device(dev):
    """reference64 (unfolded matmul) against oracle.torch_cpu_ref.resample (pad + conv1d) in float64 on the device."""
    from oracle import torch_cpu_ref as R
    for pair in ("44k-16k-kb", "48k-16k", "16k-22k"):
        g = geometry(pair, _module(pair).kernel)
        x = (0.5 * torch.randn(3, 30011, generator=torch.Generator().manual_seed(SEED_BASE))).clamp_(-1, 1).to(dev)
        want = R.resample(x.double(), g["kernel64"].to(dev)[:, None, :], g["orig0"], g["new0"], g["width"])
        have = reference64(x, g["kernel64"].to(dev), g["orig0"], g["new0"], g["width"], want.shape[1])[:, :want.shape[1]]
        assert float((have - want).abs().max()) <= 1e-13 * float(want.abs().max()), pair


@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(len(CASES)), ids=CASE_IDS)
def test_fuzz_resample_kernels_in_long_runs_vs_float64(idx, dev, limits):
    cu, lds_cap = limits
    case = CASES[idx]
    kernels = set()
    for run in draw_runs(idx, cu, lds_cap):
        plan = check_run(case, run, cu, lds_cap, dev)
        kernels |= {ps["kernel"] for ps in plan["passes"]}
    # the instantiations the case is listed for (the mirror at the design point), reached on THIS device
    assert kernels == case_kernels(idx), (case["id"], sorted(kernels), sorted(case_kernels(idx)), f"{cu} CUs, {lds_cap} bytes of LDS")


def case_kernels(idx, cu=CU_DESIGN, lds_cap=LDS_DESIGN):
    return {ps["kernel"] for run in draw_runs(idx, cu, lds_cap) for ps in run_plan(CASES[idx], run, cu, lds_cap)["passes"]}


# --------------------------------------------------------------------------- #
# 6. no device: the mirror against rsm::plan_chunk, coverage, bite            #
# --------------------------------------------------------------------------- #

def test_pick_ks_equals_the_hosts():
    from audio_amd import _host
    for span in range(1, 470):
        for orig in (0, 1, 2, 441, 320):
            assert pick_ks(span, orig) == _host._rs_pick_ks(span, orig), (span, orig)


def test_mirror_equals_plan_chunk():
    """The mirror's chunk geometry against rsm::plan_chunk itself (the CPU replay's sim_rsm_plan), for every launch pass of every
    run of every case at 256 CUs / 160 KiB, and for the same shapes once more with a 64 KiB limit (no FULL buffer, shorter chunks,
    16 k -> 22.05 k does not fit at all: scalar kernel)."""
    import sim_util as S
    f = S.sim().sim_rsm_plan
    f.argtypes = [C.c_int] * 5 + [C.c_int64, C.c_int, C.c_int64, C.c_void_p]
    n = refused = 0
    for idx, case in enumerate(CASES):
        g = geometry(case["pair"])
        ks, f16 = pick_ks(g["span"], g["orig"]), case["policy"] != POLICY_FP32
        for run in draw_runs(idx):
            for lds_cap in (LDS_DESIGN, 64 * 1024):
                plan = run_plan(case, run, CU_DESIGN, lds_cap)
                oks = []
                for p, pt0 in enumerate(range(0, len(g["tap_lo"]), max_compute_waves(ks))):
                    n_pt = min(len(g["tap_lo"]) - pt0, max_compute_waves(ks))
                    max_lo = max(g["tap_lo"][pt0:pt0 + n_pt])
                    c = plan_chunk(n_pt, ks, f16, plan["nq"], max_lo, g["orig"], plan["taps"], lds_cap)
                    out = np.zeros(8, dtype=np.int32)
                    # (sim_rsm_plan plans the first min(n_tiles, max_cw) tiles of `new`: a pass of n_pt tiles = 16 n_pt phases)
                    rc = f(g["orig"], 16 * n_pt, g["width"], g["span"], max_lo, plan["nq"], int(f16), lds_cap, out.ctypes.data_as(C.c_void_p))
                    assert rc == int(c["ok"]), (case["id"], run, lds_cap, p, rc, c)
                    assert [int(v) for v in out] == [c["qg"], c["rounds"], c["n_loaders"], c["buf_floats"], n_pt * c["qg"] + c["n_loaders"],
                                                     Q_PER_GROUP * c["qg"] * c["rounds"], ks, pieces_per_lane(ks)], (case["id"], run, lds_cap, p, c)
                    oks.append(c["ok"])
                    if not plan["generic"]:
                        ps = plan["passes"][p]
                        assert (ps["pt0"], ps["n_pt"], ps["max_lo"], ps["qg"], ps["rounds"], ps["n_loaders"], ps["buf_floats"]) == \
                            (pt0, n_pt, max_lo, c["qg"], c["rounds"], c["n_loaders"], c["buf_floats"])
                        assert ps["lds"] <= lds_cap and (lds_cap == LDS_DESIGN or not ps["full"])
                    n += 1
                assert plan["generic"] == (not all(oks)) and (lds_cap != LDS_DESIGN or not plan["generic"]), (case["id"], run, lds_cap)
                refused += plan["generic"]
    assert n > 200 and refused >= 1
    # lds_cap = 0 (no opt-in limit reported): the launcher plans with 64 KiB
    g = geometry("44k-16k-kb")
    assert launch_plan(8, 200000, g["orig"], g["new"], g["width"], g["tap_lo"], g["span"], lds_cap=0)["passes"] == \
        launch_plan(8, 200000, g["orig"], g["new"], g["width"], g["tap_lo"], g["span"], lds_cap=64 * 1024)["passes"]


def test_launch_plan_by_hand():
    """The mirror on numbers worked out by hand from csrc/api_resample.hip (256 CUs, 160 KiB): BASELINE config 3's filter."""
    g = geometry("44k-16k-kb")
    assert (g["orig"], g["new"], g["width"], g["span"], len(g["tap_lo"])) == (441, 160, 187, 414, 10)
    plan = launch_plan(256, 1323000, 441, 160, 187, g["tap_lo"], g["span"])          # 256 rows of 30 s
    ps, = plan["passes"]
    assert plan["out_len"] == 480000 and plan["nq"] == 3000 and plan["ks"] == 104 and plan["vec_in"] and plan["vec_out"]
    assert (ps["qg"], ps["rounds"], ps["n_loaders"], ps["buf_floats"], ps["chunk_q"]) == (1, 1, 2, 15360, 32) and ps["full"]
    assert (ps["chunks_per_row"], ps["n_chunks"], ps["per_cu"], ps["blocks"], ps["chunks_per_block"]) == (94, 24064, 1, 256, 94)
    assert ps["kernel"] == ("f16", 104, 8, True) and ps["lds"] == 2 * 15360 * 4 + 48
    assert chunk_a0(plan, 0, 0) == -188 and chunk_a0(plan, 0, 1) == 32 * 441 - 187 - 1 and not chunk_interior(plan, 0, 0)
    assert chunk_interior(plan, 0, 1) and chunk_interior(plan, 0, 92) and not chunk_interior(plan, 0, 93)
    w = locate(plan, 3, 160 * 32 * 5 + 47)                                          # row 3, chunk 5, phase 47
    assert (w["chunk_in_row"], w["chunk"], w["workgroup"], w["k"], w["lds_buffer"], w["max_slot"], w["phase_tile"], w["launch_pass"]) == \
        (5, 287, 3, 5, 1, 2, 2, 0) and w["interior"]
    b32 = launch_plan(256, 1323000, 441, 160, 187, g["tap_lo"], g["span"], b32=True)["passes"][0]
    assert b32["kernel"] == ("f16", 104, 4, False) and b32["buf_floats"] == 15360        # (padded all the same: plan_chunk does not ask)
    fp32 = launch_plan(256, 1323000, 441, 160, 187, g["tap_lo"], g["span"], fp32=True)["passes"][0]
    assert fp32["kernel"] == ("fp32", 104, 4, False) and fp32["buf_floats"] == buf_floats_needed(32, 441, 815, max(g["tap_lo"]), 104)
    one_in = launch_plan(1, 1323000, 441, 160, 187, g["tap_lo"], g["span"], in_aligned=False)
    assert not one_in["vec_in"] and chunk_a0(one_in, 0, 1) == 32 * 441 - 187 and not chunk_interior(one_in, 0, 1)


KERNELS_WANTED = ({("fp32", ks, 4, False) for ks in (16, 48, 80, 104, 112)} | {("f16", ks, 4, False) for ks in (16, 48, 80, 104, 112)}
                  | {("f16", ks, 8, full) for ks in (80, 104, 112) for full in (True, False)})


def test_cases_cover_the_gaps():
    """What the cases pin, with the mirror at 256 CUs / 160 KiB; a change of a case or of a draw cannot silently lose one."""
    assert 20 <= len(CASES) <= 28 and len(set(CASE_IDS)) == len(CASES)
    every = []
    for idx, case in enumerate(CASES):
        runs = draw_runs(idx)
        assert runs[0]["regime"] == "long" and len({r["regime"] for r in runs}) >= 3, case["id"]
        for run in runs:
            plan = run_plan(case, run, CU_DESIGN, LDS_DESIGN)
            assert regime_fault(run["regime"], plan, run.get("full", False)) is None, (case["id"], run)
            assert run["rows"] * run["length"] <= 30_000_000, (case["id"], run)
            every.append((case, run, plan))
    passes = [(c, r, pl, ps) for c, r, pl in every for ps in pl["passes"]]
    # gap: the sixteen product kernels, and each of them in `long` -- but the 8-byte NOT-FULL ones, which only short rows reach
    assert {ps["kernel"] for _, _, _, ps in passes} == KERNELS_WANTED and len(KERNELS_WANTED) == 16
    assert {ps["kernel"] for _, r, _, ps in passes if r["regime"] == "long"} == {k for k in KERNELS_WANTED if k[2] == 4 or k[3]}
    assert {ps["kernel"] for _, r, _, ps in passes if r["regime"] == "short"} >= {("f16", ks, 8, False) for ks in (80, 104, 112)}
    # gap: every f16 instantiation on the staircase (the NOT-FULL 8-byte ones in rows of 8 chunks), every kernel in `one` and `short`
    f16 = {k for k in KERNELS_WANTED if k[0] == "f16"}
    assert {ps["kernel"] for _, r, _, ps in passes if r["regime"] == "staircase"} == f16
    assert {r["regime"] for _, r, _ in every} == {"long", "one", "short", "staircase"}
    assert {ps["kernel"][:2] for _, r, _, ps in passes if r["regime"] == "one"} == {k[:2] for k in KERNELS_WANTED}
    assert {ps["kernel"] for _, r, _, ps in passes if r["regime"] == "one"} >= {("f16", ks, 8, True) for ks in (80, 104, 112)}
    assert {ps["kernel"][:2] for _, r, _, ps in passes if r["regime"] == "short"} == {k[:2] for k in KERNELS_WANTED}
    # gap: the side regimes -- four loader waves, rounds > 1, two launch passes (14 + 14, 14 + 6 with four loaders in the second,
    # 10 + 10), two workgroups per CU, vec_in and vec_out on and off, per kernel class
    for cls in ("f16", "fp32"):
        mine = [(c, r, pl, ps) for c, r, pl, ps in passes if ps["kernel"][0] == cls]
        assert {pl["vec_in"] for _, _, pl, _ in mine} == {True, False} == {pl["vec_out"] for _, _, pl, _ in mine}, cls
        assert {len(pl["passes"]) for _, _, pl, _ in mine} == {1, 2}, cls
        assert {ps["per_cu"] for _, _, _, ps in mine} == {1, 2}, cls
    assert {ps["n_loaders"] for _, _, _, ps in passes if ps["kernel"][0] == "f16"} == {2, 4}
    assert {ps["rounds"] for _, r, _, ps in passes if r["regime"] == "long"} >= {1, 2, 3}
    assert {tuple(ps["n_pt"] for ps in pl["passes"]) for _, _, pl in every if len(pl["passes"]) == 2} == {(14, 14), (14, 6), (10, 10)}
    assert any(ps["n_loaders"] == 4 and ps["pt0"] > 0 for _, _, _, ps in passes)
    assert any(ps["per_cu"] == 2 and ps["blocks"] > CU_DESIGN and r["regime"] == "long" for _, r, _, ps in passes)
    # gap: every `one` run twice (aligned / one sample in), with vec_in off in the FULL kernels too
    ones = [(r, pl) for _, r, pl in every if r["regime"] == "one"]
    assert {(r["offset"], pl["vec_in"]) for r, pl in ones} == {(0, True), (1, False)}
    assert any(not pl["vec_in"] and pl["passes"][0]["full"] for r, pl in ones)
    # gap: `long` -- vec_in on, interior chunks between edge chunks, runs that start and end inside rows, a shorter last run
    for c, r, pl in every:
        for p, ps in enumerate(pl["passes"]):
            if r["regime"] == "long":
                kinds = [chunk_interior(pl, p, k) for k in range(ps["chunks_per_row"])]
                assert pl["vec_in"] and not kinds[0] and not kinds[-1] and (any(kinds) or not in_registers(pl, p)), (c["id"], r)
                assert ps["chunks_per_block"] >= 5 and math.gcd(ps["chunks_per_row"], ps["chunks_per_block"]) == 1
                assert ps["n_chunks"] % ps["chunks_per_block"] != 0 and 4.0 * ps["blocks"] <= ps["n_chunks"]
    for c in CASES:                                          # `short`: a row boundary at every and at every other step of a run
        cprs = [ps["chunks_per_row"] for cc, r, pl in every if cc is c and r["regime"] == "short" for ps in pl["passes"]]
        assert not cprs or set(cprs) == {1, 2}, (c["id"], cprs)
    # gap: `short` -- qg or rounds reduced by the nq rule in some case of each class
    for cls in ("f16", "fp32"):
        reduced = 0
        for c, r, pl in every:
            if r["regime"] == "short" and pl["passes"][0]["kernel"][0] == cls:
                inf = _plan(c, 1, 10 ** 8, CU_DESIGN, LDS_DESIGN)["passes"][0]
                reduced += (pl["passes"][0]["qg"], pl["passes"][0]["rounds"]) < (inf["qg"], inf["rounds"])
        assert reduced >= 3, (cls, reduced)
    # gap: the staircase -- >= 20 (loud k, clean k + 3) pairs inside runs, in every pass; clean chunks are the second and third
    # quiet chunk behind a loud one
    for c, r, pl in every:
        if r["regime"] == "staircase":
            assert all(ps["full"] == r["full"] for ps in pl["passes"]), (c["id"], r)
            for p, ps in enumerate(pl["passes"]):
                assert stair_pairs(pl, p) >= 20, (c["id"], r, p)
                loud, clean = stair_chunks(pl, p)
                if ps["chunk_q"] == pl["passes"][0]["chunk_q"]:
                    for row in (0, 1, pl["rows"] - 1):
                        first = [k for k in range(ps["chunks_per_row"]) if (k + 2 * row) % 5 == 0]
                        for k in first:
                            # of the four quiet chunks behind the loud chunk k the second and third are clean (the first starts
                            # up to 3 samples early when vec_in rounds a0 down, the fourth reaches into the next loud step)
                            have = [bool(clean[row, j]) for j in range(k + 2, min(k + 4, ps["chunks_per_row"]))]
                            assert loud[row, k] and all(have), (c["id"], row, k, have)
                            if k + 4 < ps["chunks_per_row"] - 1:
                                assert not clean[row, k + 4], (c["id"], row, k)
    print("[fuzz-resample] gaps pinned: 16 kernels; long / one / short / staircase; 2 and 4 loaders; rounds 1 / 2 / 3; passes 14 + 14, "
          "14 + 6, 10 + 10; per_cu 1 / 2; vec_in, vec_out on / off per class; FULL with vec_in off; the staircase on all 11 f16 kernels")


def test_reference_forms_agree():
    """reference64 (unfolded matmul, slabs) against oracle.torch_cpu_ref.resample (pad + conv1d) and the numpy oracle, float64."""
    from oracle import dsp_oracle as O
    from oracle import torch_cpu_ref as R
    global SLAB_DOUBLES
    x = (0.5 * torch.randn(3, 5003, generator=torch.Generator().manual_seed(SEED_BASE))).clamp_(-1, 1)
    keep = SLAB_DOUBLES
    try:
        for pair, slab in (("44k-16k", 1 << 26), ("48k-16k", 4000), ("16k-22k", 1 << 26), ("5-3-kb", 50000)):
            SLAB_DOUBLES = slab                   # (small slabs: rows and q both cut)
            g = geometry(pair)
            want = R.resample(x.double(), g["kernel64"][:, None, :], g["orig0"], g["new0"], g["width"])
            have = reference64(x, g["kernel64"], g["orig0"], g["new0"], g["width"], want.shape[1])
            assert float(have[:, want.shape[1]:].abs().max() if have.shape[1] > want.shape[1] else 0.0) == 0.0
            assert float((have[:, :want.shape[1]] - want).abs().max()) <= 1e-13 * float(want.abs().max()), pair
            exp = O.apply_sinc_resample_kernel(x.numpy(), g["orig0"], g["new0"], 1, g["kernel64"].numpy(), g["width"])
            assert float(np.abs(have[:, :want.shape[1]].numpy() - exp).max()) <= 1e-13 * float(np.abs(exp).max()), pair
    finally:
        SLAB_DOUBLES = keep


# ---- bite: small arrays, the numpy oracle ---------------------------------------------------------------------------------------

# (perturbed reference - reference) / bar, measured on the CPU with the shapes below
BITE_MEASURED = {"float32-rounded reference": 0.00264, "chunk from the previous row's samples": 4.56e4,
                 "chunk that gets the buffer of chunk k - 2": 6.19e4, "last chunk of a run unwritten": 4.42e4,
                 "quiet row (1e-2): chunk from the previous (1e-3) row's samples": 4.67e4,
                 "the same fault under the whole-tensor metric (caught: linear op, margin x the row's gain)": 419,
                 "staircase at QUIET_GAIN = 1e-9, clean window: honest fixed21 / binary16": (0.021, 0.0062),
                 "staircase at QUIET_GAIN = 1e-9, clean window: stale fixed21 / binary16": (5e4, 99.5),
                 "stale binary16, per-row and whole-tensor metric": 0.0026,
                 "staircase at 1e-4: honest / stale fixed21": (0.014, 250), "staircase at 1e-4: honest / stale binary16": (0.0055, 0.0055),
                 "stale binary16 at 1e-7 / 1e-8 / 1e-10": (0.99, 11.8, 958)}
BITE_PAIR, BITE_CU = "44k-16k", 4
BITE_GAINS = (1.0, 1e-3, 1e-2, 1.0, 1.0, 1e-3)


def _bite_plan(rows, cpr):
    g = geometry(BITE_PAIR)
    qc = launch_plan(1, 10 ** 8, g["orig"], g["new"], g["width"], g["tap_lo"], g["span"], cu_count=BITE_CU)["passes"][0]["chunk_q"]
    length = int((cpr - 1 + 0.37) * qc * g["orig"]) // 4 * 4
    plan = launch_plan(rows, length, g["orig"], g["new"], g["width"], g["tap_lo"], g["span"], cu_count=BITE_CU)
    assert plan["passes"][0]["chunks_per_row"] == cpr and plan["passes"][0]["chunks_per_block"] >= 5, plan
    return g, plan


def _bite_oracle(x, g):
    from oracle import dsp_oracle as O
    return O.apply_sinc_resample_kernel(x, g["orig0"], g["new0"], 1, g["kernel64"].numpy(), g["width"])


_BITE = {}


def _bite_reference():
    """(geometry, plan, x float64 (6, L) with BITE_GAINS, reference (6, nq * new) as a tensor) of 6 rows of 5 chunks on 4 CUs:
    4 workgroups, runs of 8 chunks that start and end inside rows."""
    if not _BITE:
        g, plan = _bite_plan(6, 5)
        x = (0.5 * torch.randn(6, plan["length"], generator=torch.Generator().manual_seed(SEED_BASE + 7))).clamp_(-1, 1)
        x = (x * torch.tensor(BITE_GAINS)[:, None]).double().numpy()
        ref = torch.from_numpy(_bite_oracle(x, g))
        assert ref.shape == (6, plan["out_len"])
        _BITE["v"] = (g, plan, x, pad_outputs(ref, plan["nq"], plan["new"]))
    return _BITE["v"]


def _chunk_span(plan, c):
    qc, new = plan["passes"][0]["chunk_q"], plan["new"]
    return slice(c * qc * new, min((c + 1) * qc * new, plan["out_len"]))


def _bite_factor(got, ref):
    return float(row_errors(got, ref)[0].max()) / BAR


_BITE_RUN = dict(regime="bite", rows=6, length=0)


def test_bite_reference_rounded_to_float32_passes():
    g, plan, x, ref = _bite_reference()
    ps = plan["passes"][0]
    assert (ps["blocks"], ps["chunks_per_block"], ps["n_chunks"]) == (4, 8, 30)
    f = _bite_factor(ref.float(), ref)
    print(f"[fuzz-resample] bite: float32-rounded reference err/bar {f:.3g}")
    assert f <= 0.01
    assert_rows_close(ref.float(), ref, plan, "bite-rounded", _BITE_RUN)


@pytest.mark.parametrize("fault", ["chunk_from_previous_rows_samples", "chunk_gets_the_buffer_of_chunk_k_minus_2",
                                   "last_chunk_of_a_run_unwritten", "quiet_row_chunk_from_previous_rows_samples"])
def test_bite_addressing_faults(fault):
    """One chunk wrong, the way a slip of the chunk loop would leave it.  A chunk's outputs are the taps times its buffer, so a
    chunk that got another chunk's samples holds that chunk's outputs."""
    g, plan, x, ref = _bite_reference()
    ps = plan["passes"][0]
    got = ref.float().clone()
    if fault == "chunk_from_previous_rows_samples":
        row, c = 3, 2                                  # gain 1 from the 1e-2 row
        got[row, _chunk_span(plan, c)] = ref[row - 1, _chunk_span(plan, c)].float()
    elif fault == "quiet_row_chunk_from_previous_rows_samples":
        row, c = 2, 2                                  # the 1e-2 row from the 1e-3 row
        got[row, _chunk_span(plan, c)] = ref[row - 1, _chunk_span(plan, c)].float()
    elif fault == "chunk_gets_the_buffer_of_chunk_k_minus_2":
        row, c = divmod(18, ps["chunks_per_row"])     # global chunk 16 is position 0 of run 2: chunk 18 gets its buffer
        assert locate(plan, row, c * ps["chunk_q"] * plan["new"])["k"] == 2
        r2, c2 = divmod(16, ps["chunks_per_row"])
        got[row, _chunk_span(plan, c)] = ref[r2, _chunk_span(plan, c2)].float()
    else:
        row, c = divmod(2 * ps["chunks_per_block"] - 1, ps["chunks_per_row"])       # the last chunk of run 1
        where = locate(plan, row, c * ps["chunk_q"] * plan["new"])
        assert where["k"] == where["run_length"] - 1
        got[row, _chunk_span(plan, c)] = 0.0
    f = _bite_factor(got, ref)
    print(f"[fuzz-resample] bite {fault}: err/bar {f:.3g}")
    assert f >= 10.0, (fault, f)
    with pytest.raises(AssertionError):
        assert_rows_close(got, ref, plan, "bite-" + fault, _BITE_RUN)


def test_bite_whole_tensor_metric_loses_the_rows_gain():
    """Why the bar is applied per row: under a whole-tensor peak the margin of a fault in a quiet row shrinks by the row's gain.
    (Resampling is linear: a whole chunk from the wrong row is still caught -- see the module docstring.)"""
    g, plan, x, ref = _bite_reference()
    got = ref.float().clone()
    got[2, _chunk_span(plan, 2)] = ref[1, _chunk_span(plan, 2)].float()
    whole, per_row = whole_tensor_error(got, ref) / BAR, _bite_factor(got, ref)
    gain = float(ref[2].abs().max() / ref.abs().max())
    print(f"[fuzz-resample] bite quiet row (1e-2) chunk from the 1e-3 row: whole-tensor err/bar {whole:.3g}, per-row err/bar {per_row:.3g}")
    assert per_row >= 10.0 and abs(whole / (per_row * gain) - 1.0) < 1e-6 and gain < 0.02, (whole, per_row, gain)


def _quantise(v, vmax):
    """Samples cut to 21 bits below the binary exponent of `vmax`: the binary16 pair (hi, lo) of a chunk scaled by that maximum."""
    q = 2.0 ** (math.floor(math.log2(vmax)) - 21)
    return np.trunc(v / q) * q


def _split_binary16(v, vmax):
    """The kernel's own split of a chunk's samples (chunk_scale + pack_hl_cut): scaled by 2^(14 - e), e the binary exponent of
    `vmax`; hi = the mantissa cut to binary16's 10 bits, lo = the remainder, both converted to binary16 -- floating point, so a
    scale that is too large costs nothing until hi and lo fall under binary16's normal range (2^-14: an absolute step of 2^-24)."""
    scale = 2.0 ** (14 - math.floor(math.log2(vmax)))
    xs = (v * scale).astype(np.float32)
    hi32 = (xs.view(np.uint32) & np.uint32(0xFFFFE000)).view(np.float32)
    return (hi32.astype(np.float16).astype(np.float64) + (xs - hi32).astype(np.float16).astype(np.float64)) / scale


def _footprint(plan, c):
    a0 = chunk_a0(plan, 0, c)
    return slice(max(a0, 0), min(a0 + plan["passes"][0]["buf_floats"], plan["length"]))


def test_bite_staircase_honest_and_stale_scale():
    """A clean quiet chunk of a staircase row split with ITS OWN maximum passes the window bar by >= 4 x; split with the LOUD
    chunk's maximum (the stale slot) it misses the bar by >= 10 x -- under two emulations of the split: "fixed21", the samples cut
    to 21 bits below the maximum, and "binary16", the kernel's own arithmetic (_split_binary16).  The first gives both at a quiet
    gain of 1e-4 (0.014 / 250); the kernel does NOT: its hi / lo pair is floating point, at 1e-4 a stale scale costs nothing (0.005 /
    0.005, and the device cases passed against a library without the slot's zeroing), at 1e-7 it reaches the bar (0.99), at 1e-8 it
    is 11.8 x, at 1e-9 99 x.  QUIET_GAIN = 1e-9 is the value chosen: both emulations give both.  Only the window bar sees the fault:
    against the row's peak (the loud steps) and against the batch's it is nothing."""
    g, plan = _bite_plan(3, 11)
    rows, length = 3, plan["length"]
    x = (0.5 * torch.randn(rows, length, generator=torch.Generator().manual_seed(SEED_BASE + 9))).clamp_(-1, 1).double().numpy()
    i = np.arange(length)
    loud_s = np.stack([((i + plan["width"]) // stair_region(plan) + 2 * r) % 5 == 0 for r in range(rows)])
    assert bool(loud_s[1, 0]) == stair_loud(plan, 1, 0) and bool(loud_s[2, length - 1]) == stair_loud(plan, 2, length - 1)
    x = (x * np.where(loud_s, 1.0, QUIET_GAIN)).astype(np.float32).astype(np.float64)
    ref = pad_outputs(torch.from_numpy(_bite_oracle(x, g)), plan["nq"], plan["new"])
    loud, clean = stair_chunks(plan, 0)
    row, k = 0, 3                                     # row 0: chunks 0, 5, 10 are loud; 3 is the third quiet chunk behind chunk 0
    assert loud[row, 0] and clean[row, 2] and clean[row, 3] and not clean[row, 1] and not clean[row, 4]
    fp = _footprint(plan, k)
    assert not loud_s[row, fp].any()
    worst = {}
    for name, vmax in (("honest", float(np.abs(x[row, fp]).max())), ("stale", float(np.abs(x[row, _footprint(plan, 0)]).max()))):
        for emu, split in (("fixed21", _quantise), ("binary16", _split_binary16)):
            bad = x[row:row + 1].copy()
            bad[0, fp] = split(bad[0, fp], vmax)
            got = ref.float().clone()
            got[row, _chunk_span(plan, k)] = torch.from_numpy(_bite_oracle(bad, g))[0, _chunk_span(plan, k)].float()
            err, peak = window_errors(got, ref, plan, 0)
            worst[name, emu] = float(err[row, k] / peak[row, k]) / BAR
            print(f"[fuzz-resample] bite staircase {name} {emu}: clean window err/bar {worst[name, emu]:.3g}, per-row "
                  f"{_bite_factor(got, ref):.3g}, whole-tensor {whole_tensor_error(got, ref) / BAR:.3g}")
            if name == "stale":
                assert _bite_factor(got, ref) < 1.0 and whole_tensor_error(got, ref) / BAR < 1.0
    assert max(worst["honest", "fixed21"], worst["honest", "binary16"]) <= 0.25, worst
    assert min(worst["stale", "fixed21"], worst["stale", "binary16"]) >= 10.0, worst
    # the float32-rounded reference passes the window bar everywhere, and the assertion the device cases use sees the stale chunk
    run = dict(regime="staircase", rows=rows, length=length)
    assert assert_clean_windows_close(ref.float(), ref, plan, "bite-staircase", run) >= 4
    with pytest.raises(AssertionError):
        assert_clean_windows_close(got, ref, plan, "bite-staircase-stale", run)
