"""Every biquad-class IIR kernel behind aamd_lfilter_f32 (csrc/lfilter_wave.h, chosen by lfw::pick, launched by csrc/api_lfilter.hip)
in MULTI-SEQUENCE launches against float64: lfw::lfilter_wave_kernel<0, 8, true> (16-byte aligned rows, W = 1, 2, 4 waves per
sequence), <0, 8, false> (unaligned rows, W <= 8), <0, 16, false> (unaligned, W = 16), lfw::lfilter_wave_pipe_kernel<0> (aligned,
W >= 8, 1 - 2 stages) and lfw::lfilter_wave_mover_kernel<0> (aligned, W >= 8, >= 3 stages) -- five launch targets.  The sixth
instantiation, <0, 16, true>, is never picked (test_wave16_vec_is_never_picked).

Why: the workgroups are persistent -- the launcher starts blocks = min(n_seq, 8 x CUs) of them and each loops
`for (seq = blockIdx.x; seq < n_seq; seq += gridDim.x)` -- and W grows only while n_seq * 2 W <= 8192, so before this file no
workgroup had run a SECOND sequence with W >= 2 on a device (the largest case was 3000 sequences of 100 samples: W = 1, one ragged
block each, shared coefficients).  What only acts from the second sequence on: the `built_crow` cache of the fp64 tables (rebuilt
when consecutive sequences of a workgroup use different coefficient rows: 3 channels on 2048 workgroups; kept with 2 or 4), the
zeroing of the exchange area (block carries), the `nw0 > 0` guards of the history row, and the LDS-DMA that may still be in flight
at a sequence's end.  The "unaligned rows" case of tests/test_gpu_parity.py ran the aligned pipe kernel on a copy (its view was
not contiguous): VEC = false had been reached only through length % 4 != 0, never with more than one stage at W = 8 or 16.  Poles
near the unit circle (the cross-wave fold Mc^(64 k), the block carry and the mover kernel's pre-loaded tables with values that
matter) had only met the CPU replay.  Pipe and mover had never run a single-block sequence, the launcher's width boundaries,
clamp = 0, first-order or gain-only stages.  And nothing checked which kernel a case ran.

launch_plan() is a host mirror of lfw::pick; every device run ASSERTS the kernel, W and regime it claims from the mirror with the
device's own CU count (checked against aamd_device_info) and LDS opt-in, and the mirror against aamd_lfilter_plan for the very
tensors of the call: on another device a case is re-sized by the mirror or fails loudly.  Every launch goes through
functional._lfilter_launch, which hands the tensor's own pointer to the launcher (F.lfilter makes non-contiguous views contiguous,
i.e. aligned; the torch op and the ctypes route keep a contiguous view's storage offset -- asserted: data_ptr() % 16 != 0).
Regimes (sizes at 256 CUs):

  many-seq   W = 1: 5123 .. 5124 sequences (2.5 x blocks + 3) of 2085 / 2088 samples, two blocks, and 4097 of 4096 (two WHOLE
             blocks: the last block's carry is not one that decayed through padded zeros); W = 2: 4096 sequences of
             4100 / 4101 (the second block holds 4 - 5 samples of wave 0, wave 1 wholly past the end) and 3075 = 1025 x 3 of
             6148 .. 6150; shared and per-channel coefficients (3 channels: tables rebuilt between a workgroup's sequences;
             2 or 4: kept -- both asserted from the mirror); 1, 2 and 4 stages; one all-zero row as the second sequence of a
             workgroup behind a gain-1 row: its output is exactly 0.0
             (a covering selection of 13 cases of 43 .. 76 MB, not the full cross product: test_cases_cover_the_gaps lists it)
  unaligned  a row base off by 1, 2, 3 floats with L % 4 == 0 (a contiguous view into a flat buffer), and L % 4 != 0, at
             W = 4, 8, 16 with 1, 2, 3, 5, 8 stages over 3 blocks (W = 16: 3 and 4), the last one ragged.  (Four blocks at W = 4
             or 8 need >= 1025 / 513 rows of >= 24576 / 49152 samples: 100 MB, above this file's 70 MB.)
  slow       resonators a = [1, -2 r cos t, r^2], b = [1 - r, 0, 0] with the (r, t) of
             test_sim_lfilter_wave_slowly_decaying_poles_across_waves, 0.1 x randn, clamp 0, 3 blocks + 515 .. 516 samples: on
             <0, 16, false>, pipe (1 and 2 stages), mover (3 and 4 stages, another t per stage) and W = 2 many-seq (2 blocks + 516:
             2051 rows of 3 whole blocks are 105 MB).  Device-free precondition on one row: the CPU replay of the same design
             stays <= 4e-5 of the float64 peak.  Every design meets it at the replay test's own r (no r was lowered); the 4-stage
             cascade only with the near-DC resonator (0.99, 0.05) as its FIRST stage (3.0e-5; as the last stage 6.5e-5).
  edges      pipe / mover at L = 8196, 12292, 16384, 16388 (one block without has_next and with waves 5 .. 7 wholly past the end;
             an exact block; a second block of 4 samples), n_seq 1, 6, 1024 and 1025 (mirror: W = 4, <0, 8, true>), 1, 2, 3, 8
             stages, clamp 0 / 1 / 2, per-channel rows, n_order 3, 2 and 1 (the ABI has ONE n_order per call: first-order and
             gain-only stages inside a second-order cascade are zero-padded rows)
  tiny       L = 1, 2, 3, 31, 32, 33, 63, 64, 65, 2047, 2048, 3 rows, 2 stages

Inputs: standard normal float32 rows with gains cycling 1, 1e-3, 1e-2, 1, clipped to [-1, 1] where the case clamps.
Reference: the float64 sequential recursion of the stored float32 coefficients normalised by the fp32 division a / a0 (as
lfw::build_stage does), stage by stage, clamped as the call clamps: scipy.signal.lfilter, held against oracle.dsp_oracle.lfilter
on a 3000-sample prefix at 1e-9 in every run (tiny: the oracle itself).  Every output sample is compared.

Bars (none is new, none is derived from the product's output): 1e-4 peak-relative for one stage
(tests/test_gpu_fuzz.py::test_fuzz_lfilter_vs_oracle), 2e-4 for cascades (test_lfilter_pipelined_kernel_against_oracle; a clamp
is 1-Lipschitz, so the clamped cascades' bar also holds the unclamped ones), PER OUTPUT ROW against that row's own reference
peak; the all-zero row exactly 0.0; a repeated call bit-equal.  A failure prints sequence, workgroup, position in the
workgroup's run, block, wave and lane of the worst sample.

Device-free: the mirror against lfw::pick itself (sim_lfw_pick) for every case at 256, 64 and 8 CUs and over a sweep, <0, 16, true>
never picked, pipe / mover never with more sequences than workgroups at >= 128 CUs, the coverage at 256 CUs, the replay
preconditions, the float32 sequential recursion's own error (FLOAT32_SEQUENTIAL, context for MEASURED_DEVICE) and bite tests:
float64 models on this file's inputs of a second sequence started from the first one's block carry, of a second sequence
filtered with the previous coefficient row's tables and of a first block that reads a non-zero history row, each > 10 x its bar.

Measured on an MI355X (256 CUs): MEASURED_DEVICE, FILE_SECONDS.  No case found a kernel wrong: the worst per-row err / bar is 0.026
among the three one-tile instantiations and the pipe kernel and 0.142 for the mover kernel (the 4-stage slow-pole cascade, whose
CPU replay stands at 0.152 of the same bar on row 0 and a float32 sequential recursion at 0.060; every decaying design stays
under 0.03), every all-zero row came out 0.0, every
repeated call bit-equal, and the library's plan equalled the mirror in all 41 device tests.

That the DEVICE cases bite was checked once by hand against a library with two precision-only faults in lfilter_wave_kernel (in
bounds; that build is not committed): (1) the exchange area zeroed for a workgroup's first sequence only; (2) the fp64 tables
built once per workgroup.  6 of the 41 device tests failed and 35 passed, as the faults predict: (2) the four cases with 3
coefficient rows (err / bar 1.0e4 .. 1.8e4; 2 and 4 rows divide the 2048 workgroups and passed); (1) ms-w1-shared-2st-4096-exact
(the all-zero row peaks at 0.158) and slow-w2-many (0.004) -- and no other many-sequence case, because there the last block ends in
~2000 padded zeros through which the radius-0.9 poles decay to exactly nothing before the carry is left behind: the reason the
whole-block case and the slow-pole W = 2 case exist.  Pipe, mover and <0, 16, false> were not touched and passed.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

CU_DESIGN = 256
LDS_CAP_DESIGN = 160 * 1024
BAR_ONE, BAR_CASCADE = 1e-4, 2e-4
REPLAY_BAR = 4e-5                                                   # tests/test_cpu_sim.py, the slow-pole replay test
K_CH, WAVE_BLOCK, K_HIST, MAX_CASCADE, MAX_WAVES, TAB_FLOATS = 32, 2048, 64, 8, 16, 368      # csrc/lfilter_wave.h
TILE, PIPE_TILE = K_HIST + WAVE_BLOCK, K_HIST + 2 * WAVE_BLOCK
GAINS = (1.0, 1e-3, 1e-2, 1.0)
SEED_BASE = 91700
SLOW = ((0.9995, 0.3), (0.999, 1.2), (0.99, 0.05), (0.9999, 2.0))   # the replay test's (r, theta)

GENERAL, WAVE8_VEC, WAVE8, WAVE16_VEC, WAVE16, PIPE, MOVER = range(7)            # lfw::PickKernel
KERNEL_NAMES = {GENERAL: "lfilter_kernel<D>", WAVE8_VEC: "lfw::lfilter_wave_kernel<0, 8, true>",
                WAVE8: "lfw::lfilter_wave_kernel<0, 8, false>", WAVE16_VEC: "lfw::lfilter_wave_kernel<0, 16, true>",
                WAVE16: "lfw::lfilter_wave_kernel<0, 16, false>", PIPE: "lfw::lfilter_wave_pipe_kernel<0>",
                MOVER: "lfw::lfilter_wave_mover_kernel<0>"}
KERNELS_WANTED = {KERNEL_NAMES[k] for k in (WAVE8_VEC, WAVE8, WAVE16, PIPE, MOVER)}

# measured on an MI355X (256 CUs), one run of this file with -s: kernel -> (worst per-row err / bar, its case) from the
# "[fuzz-lfilter]" lines; FLOAT32_SEQUENTIAL beside it is the same figure for a float32 sequential recursion in numpy
MEASURED_DEVICE = {
    "lfw::lfilter_wave_kernel<0, 8, true>": (0.0256, "slow-w2-many"), "lfw::lfilter_wave_kernel<0, 8, false>": (0.0179, "ms-w1-shared-1st-2085"),
    "lfw::lfilter_wave_kernel<0, 16, false>": (0.0191, "un-w16-off3-8st"), "lfw::lfilter_wave_pipe_kernel<0>": (0.0188, "slow-pipe-2st"),
    "lfw::lfilter_wave_mover_kernel<0>": (0.1421, "slow-mover-4st"),
}
# the 41 device tests of this file together: 12.7 s of pytest wall time (1.1 s for the first case, which loads the library; 0.4 .. 0.7 s
# for the fifteen cases of 60 .. 76 MB -- host randn, two copies and the scipy reference, the launches are milliseconds; under 0.2 s
# for every other) -- 3 % on top of the 404 s the device suite takes without it (1 279 tests; 417 s and 1 320 tests with it)
FILE_SECONDS = 12.7
# err / bar of a float32 sequential recursion (numpy, w = b2 x2 + b1 x1 + b0 x0; y = w - a2 y2 - a1 y1, the reference's order) on
# rows 0 .. 3 of one case per kernel and of every slow-pole case, against the same float64 reference
# (test_float32_sequential_recursion_context prints them; no device involved)
FLOAT32_SEQUENTIAL = {"ms-w2-ch3-4st-6148": 0.0097, "ms-w2-shared-4st-4101": 0.0095, "pm-6x12292-2st-c0": 0.0103, "pm-6x16384-3st-c2": 0.0136,
                      "slow-w16": 0.0582, "slow-pipe-1st": 0.0388, "slow-pipe-2st": 0.0408, "slow-mover-3st": 0.0451,
                      "slow-mover-4st": 0.0596, "slow-w2-many": 0.0480}


# --------------------------------------------------------------------------- #
# 1. the host mirror of lfw::pick                                             #
# --------------------------------------------------------------------------- #

def _cdiv(a, b):
    return -(-a // b)


def lds_bytes(W, n_stages):
    return (W * TILE + n_stages * TAB_FLOATS + 4 * W + 4 * n_stages + 4) * 4


def pipe_lds_bytes(W, n_stages):
    return (W * PIPE_TILE + n_stages * TAB_FLOATS + 4 * W + 4 * n_stages + 4) * 4


def pick(n_seq, length, n_order, n_stages, vec_ok, lds_cap=LDS_CAP_DESIGN, cu_count=CU_DESIGN):
    """lfw::pick without the lab overrides: (kernel id, W, blocks, LDS bytes)."""
    blocks = max(1, min(n_seq, 8 * cu_count))
    if not (n_order <= 3 and n_stages <= MAX_CASCADE and length < (1 << 30)):
        return GENERAL, 0, blocks, 0
    W = 1
    while W < MAX_WAVES and n_seq * 2 * W <= 8192 and W * WAVE_BLOCK < length:
        W *= 2
    while W > 1 and lds_bytes(W, n_stages) > lds_cap:
        W //= 2
    lds = lds_bytes(W, n_stages)
    if lds > lds_cap:
        return GENERAL, 0, blocks, 0
    if vec_ok and W >= 8 and pipe_lds_bytes(8, n_stages) <= lds_cap:
        return (MOVER if n_stages >= 3 else PIPE), 8, blocks, pipe_lds_bytes(8, n_stages)
    if W <= 8:
        return (WAVE8_VEC if vec_ok else WAVE8), W, blocks, lds
    return (WAVE16_VEC if vec_ok else WAVE16), W, blocks, lds


def launch_plan(n_seq, length, n_order, n_stages, vec_ok, channels=1, n_coeff_rows=1, cu_count=CU_DESIGN, lds_cap=LDS_CAP_DESIGN):
    """aamd_lfilter_f32 for n_seq = batch x channels rows of `length` samples on a device of `cu_count` CUs: workgroup g filters the
    sequences g, g + blocks, ... in blocks of W x 2048 samples; `rebuilds`: consecutive sequences of some workgroup use different
    coefficient rows (the fp64 tables are built again), `kept`: a workgroup runs several sequences on one build."""
    kid, W, blocks, lds = pick(n_seq, length, n_order, n_stages, vec_ok, lds_cap, cu_count)
    p = dict(n_seq=n_seq, length=length, n_order=n_order, n_stages=n_stages, vec_ok=bool(vec_ok), channels=channels,
             n_coeff_rows=n_coeff_rows, cu_count=cu_count, lds_cap=lds_cap, kid=kid, kernel=KERNEL_NAMES[kid], W=W, blocks=blocks,
             lds=lds, block_len=W * WAVE_BLOCK, n_blocks=_cdiv(length, W * WAVE_BLOCK) if W else 0,
             seqs_per_wg_max=_cdiv(n_seq, blocks), seqs_per_wg_min=n_seq // blocks)
    second = n_seq > blocks
    p["rebuilds"] = bool(second and n_coeff_rows > 1 and blocks % channels != 0)
    p["kept"] = bool(second and not p["rebuilds"])
    return p


def crow_of(plan, seq):
    return 0 if plan["n_coeff_rows"] == 1 else seq % plan["channels"]


def locate(plan, seq, sample):
    """Where the launch computes output `sample` of sequence `seq`."""
    bl = max(plan["block_len"], 1)
    return dict(sequence=seq, sample=sample, workgroup=seq % plan["blocks"], position=seq // plan["blocks"],
                run_length=_cdiv(plan["n_seq"] - seq % plan["blocks"], plan["blocks"]), block=sample // bl,
                last_block=sample // bl == plan["n_blocks"] - 1, wave=(sample % bl) // WAVE_BLOCK,
                lane=(sample % WAVE_BLOCK) // K_CH, crow=crow_of(plan, seq), kernel=plan["kernel"], W=plan["W"])


# --------------------------------------------------------------------------- #
# 2. the cases                                                                #
# --------------------------------------------------------------------------- #

def _c(cid, regime, kid, W, L, stages, shape=None, clamp=1, rows="shared", order=3, offset=0, design="decay", many=None):
    """shape: (batch, channels), None where the mirror sizes it (`many`: "w1" 2.5 x blocks + 3 sequences, "w1min" / "w2" two per workgroup,
    "w2x3" 1.5 per workgroup on 3 channels); offset: floats between a 16-byte boundary and the first row; design: "decay" (poles of
    radius ~0.9, gain 1.3 where the case clamps), "mixed" (second- / first-order / gain-only stages as zero-padded rows) or a
    tuple of indices into SLOW, one per stage."""
    return dict(id=cid, regime=regime, kid=kid, W=W, L=L, stages=stages, shape=shape, clamp=clamp, rows=rows, order=order,
                offset=offset, design=design, many=many)


B3, B4 = 2 * WAVE_BLOCK, 3 * WAVE_BLOCK                            # two / three whole blocks per wave of W
CASES = [
    # many sequences: every workgroup (W = 1, 4096-sequence W = 2) or half of them (3075) runs a second sequence
    _c("ms-w1-shared-1st-2085", "many-seq", WAVE8, 1, 2085, 1, many="w1"),
    _c("ms-w1-ch3-2st-2085", "many-seq", WAVE8, 1, 2085, 2, many="w1", rows=3),
    _c("ms-w1-ch4-4st-2088", "many-seq", WAVE8_VEC, 1, 2088, 4, many="w1", rows=4),
    _c("ms-w1-shared-2st-2088", "many-seq", WAVE8_VEC, 1, 2088, 2, many="w1", clamp=2),
    # (two WHOLE blocks: the carry the last block leaves is the row's true end state, not that of ~2000 padded zeros through which
    # a pole of radius 0.9 has decayed to nothing -- an exchange area that is not zeroed shows on an ordinary design here)
    _c("ms-w1-shared-2st-4096-exact", "many-seq", WAVE8_VEC, 1, 4096, 2, many="w1min"),
    _c("ms-w2-shared-1st-4100", "many-seq", WAVE8_VEC, 2, 4100, 1, many="w2"),
    _c("ms-w2-ch4-2st-4100", "many-seq", WAVE8_VEC, 2, 4100, 2, many="w2", rows=4),
    _c("ms-w2-shared-4st-4101", "many-seq", WAVE8, 2, 4101, 4, many="w2"),
    _c("ms-w2-ch2-4st-4100", "many-seq", WAVE8_VEC, 2, 4100, 4, many="w2", rows=2),
    _c("ms-w2-ch3-1st-6148", "many-seq", WAVE8_VEC, 2, 6148, 1, many="w2x3", rows=3),
    _c("ms-w2-ch3-4st-6148", "many-seq", WAVE8_VEC, 2, 6148, 4, many="w2x3", rows=3),
    _c("ms-w2-shared3-2st-6150", "many-seq", WAVE8, 2, 6150, 2, many="w2x3"),
    _c("ms-w2-ch3-2st-6149", "many-seq", WAVE8, 2, 6149, 2, many="w2x3", rows=3, clamp=0),
    # unaligned rows: the dword copies and element-wise stores with a history row, over 3 (4) blocks, the last one ragged
    _c("un-w16-off1-3st", "unaligned", WAVE16, 16, 16 * B3 + 516, 3, (5, 1), offset=1),
    _c("un-w16-off2-5st-4blk", "unaligned", WAVE16, 16, 16 * B4 + 516, 5, (1, 3), offset=2, rows=3),
    _c("un-w16-off3-8st", "unaligned", WAVE16, 16, 16 * B3 + 516, 8, (2, 2), offset=3, clamp=2),
    _c("un-w16-len-1st", "unaligned", WAVE16, 16, 16 * B3 + 515, 1, (3, 1)),
    _c("un-w16-len-2st-4blk", "unaligned", WAVE16, 16, 16 * B4 + 513, 2, (1, 4), rows=4, clamp=0),
    _c("un-w8-off1-3st", "unaligned", WAVE8, 8, 8 * B3 + 516, 3, (513, 1), offset=1),
    _c("un-w8-len-5st", "unaligned", WAVE8, 8, 8 * B3 + 514, 5, (171, 3), rows=3),
    _c("un-w4-off3-2st", "unaligned", WAVE8, 4, 4 * B3 + 516, 2, (1025, 1), offset=3),
    _c("un-w4-off2len-5st", "unaligned", WAVE8, 4, 4 * B3 + 515, 5, (1025, 1), offset=2, clamp=2),
    # poles near the unit circle: the cross-wave fold, the block carry and the pre-loaded tables with values that matter
    _c("slow-w16", "slow", WAVE16, 16, 16 * B4 + 515, 1, (3, 1), clamp=0, design=(0,)),
    _c("slow-pipe-1st", "slow", PIPE, 8, 8 * B4 + 516, 1, (3, 1), clamp=0, design=(3,)),
    _c("slow-pipe-2st", "slow", PIPE, 8, 8 * B4 + 516, 2, (1, 3), clamp=0, design=(0, 1)),
    _c("slow-mover-3st", "slow", MOVER, 8, 8 * B4 + 516, 3, (3, 1), clamp=0, design=(0, 1, 3)),
    # (the near-DC resonator goes FIRST: behind a narrow-band stage it passes that stage's low-frequency rounding noise at gain 3.8 and
    # the signal at 1e-3 -- the replay of (0.9999, 2.0) -> (0.99, 0.05) misses even 2e-4, as any float32 filter of that order would)
    _c("slow-mover-4st", "slow", MOVER, 8, 8 * B4 + 516, 4, (2, 2), clamp=0, design=(2, 3, 1, 0)),
    _c("slow-w2-many", "slow-many", WAVE8_VEC, 2, 2 * B3 + 516, 1, clamp=0, design=(0,), many="w2min"),
    # pipe / mover: single-block sequences, the launcher's width boundaries, every clamp mode, first-order and gain-only stages
    _c("pm-1x8196-1st", "edges", PIPE, 8, 8196, 1, (1, 1)),
    _c("pm-6x12292-2st-c0", "edges", PIPE, 8, 12292, 2, (2, 3), clamp=0, rows=3),
    _c("pm-6x16384-3st-c2", "edges", MOVER, 8, 16384, 3, (3, 2), clamp=2, rows=2),
    _c("pm-1x16388-8st", "edges", MOVER, 8, 16388, 8, (1, 1)),
    _c("pm-6x8196-8st-mixed-c0", "edges", MOVER, 8, 8196, 8, (6, 1), clamp=0, design="mixed"),
    _c("pm-1024x8196-3st-ch4", "edges", MOVER, 8, 8196, 3, (256, 4), rows=4),
    _c("pm-1024x16388-2st-c2", "edges", PIPE, 8, 16388, 2, (1024, 1), clamp=2),
    _c("pm-1025x8196-2st", "edges", WAVE8_VEC, 4, 8196, 2, (1025, 1)),
    _c("pm-6x16388-1st-order1", "edges", PIPE, 8, 16388, 1, (6, 1), clamp=0, order=2),
    _c("pm-6x12292-3st-gain", "edges", MOVER, 8, 12292, 3, (2, 3), order=1, rows=3),
    _c("pm-6x16384-2st-order1", "edges", PIPE, 8, 16384, 2, (6, 1), order=2),
    _c("pm-1x8196-3st-mixed-c2", "edges", MOVER, 8, 8196, 3, (1, 1), clamp=2, design="mixed"),
]
CASE_IDS = [c["id"] for c in CASES]
TINY_LENGTHS = (1, 2, 3, 31, 32, 33, 63, 64, 65, 2047, 2048)


def case_shape(case, cu=CU_DESIGN):
    """(batch, channels) of a case on a device with `cu` CUs -- the mirror's workgroup count sizes the many-sequence cases."""
    if case["shape"] is not None:
        return case["shape"]
    ch = case["rows"] if case["rows"] != "shared" else (3 if case["many"] == "w2x3" else 1)
    cap = 8 * cu
    if case["many"] == "w1":                                     # 2.5 x blocks + 3, too many for W = 2, not a multiple of the workgroups
        n = max(int(2.5 * cap) + 3, 4097)
    elif case["many"] == "w1min":                                # two on every workgroup, too many for W = 2 (4097 at 256 CUs)
        n = max(2 * cap + 1, 4097)
    elif case["many"] == "w2":                                   # two on every workgroup (4096 at 256 CUs)
        n = min(4096, 2 * cap)
    elif case["many"] == "w2x3":                                 # 1.5 x blocks + 3 (3075 at 256 CUs): half the workgroups run two
        n = min(4096, cap + cap // 2 + 3)
    else:                                                        # "w2min": a few workgroups run two
        n = min(4096, cap + 3)
    n = _cdiv(n, ch) * ch
    while n % min(n, cap) == 0 and case["many"] == "w1":
        n += ch
    return n // ch, ch


def design_coeffs(case, channels):
    """(a, b) float32 (stages, rows, n_order): what the call stores on the device."""
    n, order = case["stages"], case["order"]
    crows = 1 if case["rows"] == "shared" else channels
    a, b = np.zeros((n, crows, order)), np.zeros((n, crows, order))
    gain = 1.3 if case["clamp"] else 1.0
    for s in range(n):
        for c in range(crows):
            if isinstance(case["design"], tuple):
                r, t = SLOW[case["design"][s]]
                t = t + 0.07 * c
                a[s, c], b[s, c] = [1.0, -2 * r * math.cos(t), r * r], [1 - r, 0.0, 0.0]
                continue
            kind = (3, 2, 1)[(s + c) % 3] if case["design"] == "mixed" else order
            w0 = 2 * math.pi * (300.0 + 700.0 * s + 450.0 * c) / 16000
            alpha = math.sin(w0) / 2 / (0.6 + 0.1 * s)
            k = gain * (1 - math.cos(w0)) / 2
            if kind == 3:                                        # low-pass biquad, a0 != 1: the fp32 division matters
                row_a, row_b = [1 + alpha, -2 * math.cos(w0), 1 - alpha], [k, 2 * k, k]
            elif kind == 2:                                      # first order
                row_a, row_b = [1.25, -1.25 * (0.85 - 0.03 * s - 0.02 * c), 0.0], [0.3 * gain, 0.25 * gain, 0.0]
            else:                                                # a gain
                row_a, row_b = [2.0 + 0.125 * s, 0.0, 0.0], [(1.9 + 0.2 * c) * (gain if s == 0 else 1.0), 0.0, 0.0]
            a[s, c], b[s, c] = row_a[:order], row_b[:order]
    return a.astype(np.float32), b.astype(np.float32)


def make_run(idx, cu=CU_DESIGN, lds_cap=LDS_CAP_DESIGN):
    case = CASES[idx]
    batch, ch = case_shape(case, cu)
    crows = 1 if case["rows"] == "shared" else ch
    vec_ok = case["offset"] == 0 and case["L"] % 4 == 0
    plan = launch_plan(batch * ch, case["L"], case["order"], case["stages"], vec_ok, ch, crows, cu, lds_cap)
    a, b = design_coeffs(case, ch)
    run = dict(case, idx=idx, batch=batch, channels=ch, n_seq=batch * ch, crows=crows, vec_ok=vec_ok, a=a, b=b,
               seed=SEED_BASE + idx, scale=0.1 if isinstance(case["design"], tuple) else 1.0)
    run["zero_seq"] = zero_row_of(plan)
    return run, plan


def zero_row_of(plan):
    """The sequence to silence: the first that is the SECOND of its workgroup's run behind a gain-1 row (None: no second sequence)."""
    for seq in range(plan["blocks"], min(plan["n_seq"], 2 * plan["blocks"])):
        if GAINS[(seq - plan["blocks"]) % 4] == 1.0:
            return seq
    return None


def regime_fault(run, plan):
    """None when `plan` is what `run` claims, else what it misses (every device run asserts this on the device's own numbers)."""
    if plan["kid"] != run["kid"] or plan["W"] != run["W"]:
        return "%s W = %d, not %s W = %d" % (plan["kernel"], plan["W"], KERNEL_NAMES[run["kid"]], run["W"])
    if run["regime"] in ("many-seq", "slow-many"):
        if plan["seqs_per_wg_max"] < 2 or run["zero_seq"] is None:
            return "%d sequences on %d workgroups" % (plan["n_seq"], plan["blocks"])
        if run["many"] == "w1" and (plan["n_seq"] < int(2.5 * plan["blocks"]) + 3 or plan["n_seq"] % plan["blocks"] == 0
                                    or plan["seqs_per_wg_max"] < 3):
            return "%d sequences on %d workgroups" % (plan["n_seq"], plan["blocks"])
        if run["many"] == "w2" and plan["seqs_per_wg_min"] < 2:
            return "a workgroup with one sequence"
        if run["crows"] == 3 and not plan["rebuilds"] or run["crows"] in (2, 4) and not plan["kept"]:
            return "tables rebuilt %s, kept %s with %d coefficient rows" % (plan["rebuilds"], plan["kept"], run["crows"])
        if plan["n_blocks"] < 2:
            return "%d blocks" % plan["n_blocks"]
    if run["regime"] in ("unaligned", "slow", "slow-many") and plan["n_blocks"] < 3:
        return "%d blocks" % plan["n_blocks"]
    if run["regime"] == "unaligned" and (plan["vec_ok"] or plan["length"] % plan["block_len"] == 0):
        return "aligned rows or no ragged block"
    return None


def bar_of(run):
    return BAR_ONE if run["stages"] == 1 else BAR_CASCADE


# --------------------------------------------------------------------------- #
# 3. inputs, the reference and the checks                                     #
# --------------------------------------------------------------------------- #

def make_inputs(run):
    """(n_seq, L) float32 on the host: randn x gain of the row, clipped where the case clamps, the zero row silenced."""
    g = torch.Generator().manual_seed(run["seed"])
    x = torch.randn(run["n_seq"], run["L"], generator=g)
    x.mul_(torch.tensor([GAINS[s % 4] for s in range(run["n_seq"])])[:, None] * run["scale"])
    if run["clamp"]:
        x.clamp_(-1.0, 1.0)
    if run["zero_seq"] is not None:
        x[run["zero_seq"]] = 0.0
    return x


def normalised(a, b):
    """ah, bh float64 of the fp32 division a / a0, b / a0 (lfw::build_stage)."""
    a0 = a[..., :1]
    return (a / a0).astype(np.float32).astype(np.float64), (b / a0).astype(np.float32).astype(np.float64)


def stage_clamps(clamp, st, n_stages):
    return clamp == 1 or (clamp == 2 and st == n_stages - 1)


def reference64(x, a, b, clamp, channels, seqs=None):
    """The float64 sequential recursion of rows `seqs` (all) of x (n_seq, L): stage by stage, row seq with the coefficient
    row seq % channels (or the one row), clamped as the call clamps."""
    from scipy import signal
    ah, bh = normalised(a, b)
    if isinstance(x, torch.Tensor):
        y = x.double().numpy() if seqs is None else x[torch.as_tensor(np.asarray(seqs))].double().numpy()
    else:
        y = np.array(x, dtype=np.float64) if seqs is None else np.asarray(x, dtype=np.float64)[np.asarray(seqs)]
    seqs = np.arange(y.shape[0]) if seqs is None else np.asarray(seqs)
    n_stages, crows = a.shape[0], a.shape[1]
    for st in range(n_stages):
        for c in range(crows):
            sel = np.nonzero(seqs % channels == c)[0] if crows > 1 else slice(None)
            if crows == 1 or len(sel):
                y[sel] = signal.lfilter(bh[st, c], ah[st, c], y[sel], axis=-1)
        if stage_clamps(clamp, st, n_stages):
            np.clip(y, -1.0, 1.0, out=y)
    return y


def oracle64(x, a, b, clamp, channels):
    """The same cascade by oracle.dsp_oracle.lfilter (a Python loop over the samples) for x (batch * channels, L)."""
    from oracle import dsp_oracle as O
    ah, bh = normalised(a, b)
    crows = a.shape[1]
    y = np.asarray(x, dtype=np.float64).reshape(-1, channels, x.shape[-1])
    for st in range(a.shape[0]):
        ar, br = (ah[st], bh[st]) if crows > 1 else (np.repeat(ah[st], channels, 0), np.repeat(bh[st], channels, 0))
        y = O.lfilter(y, ar, br, stage_clamps(clamp, st, a.shape[0]))
    return y.reshape(-1, x.shape[-1])


def float32_sequential(x, a, b, clamp, channels, seqs):
    """The same cascade in float32, sample by sample in the reference's operation order (numpy; context only)."""
    ah, bh = (v.astype(np.float32) for v in normalised(a, b))
    seqs = np.asarray(seqs)
    y = x[seqs].numpy().astype(np.float32)
    order = a.shape[-1]
    for st in range(a.shape[0]):
        rows = np.zeros(len(seqs), dtype=np.int64) if a.shape[1] == 1 else seqs % channels
        A, Bc = ah[st][rows], bh[st][rows]
        A, Bc = np.pad(A, ((0, 0), (0, 3 - order))), np.pad(Bc, ((0, 0), (0, 3 - order)))
        x1 = x2 = y1 = y2 = np.zeros(len(seqs), dtype=np.float32)
        out = np.empty_like(y)
        for n in range(y.shape[1]):
            x0 = y[:, n]
            w = Bc[:, 2] * x2
            w = w + Bc[:, 1] * x1
            w = w + Bc[:, 0] * x0
            o = w - A[:, 2] * y2
            o = o - A[:, 1] * y1
            out[:, n] = o
            x2, x1, y2, y1 = x1, x0, y1, o
        y = np.clip(out, -1.0, 1.0) if stage_clamps(clamp, st, a.shape[0]) else out
    return y


def row_errors(got, ref):
    """(r, n) x 2 numpy -> per row max|got - ref| / max|ref of that row| (the absolute error where the row's reference is all
    zero), and the index of each row's worst element."""
    d = np.abs(got.astype(np.float64) - ref)
    where = d.argmax(1)
    e = d.max(1)
    peak = np.abs(ref).max(1)
    return np.where(peak > 0, e / np.maximum(peak, 1e-300), e), where


_WORST = {}


def check_outputs(got, ref, plan, run, bar):
    """Every output of every row of got (n_seq, L) against ref: finite, the zero row exactly 0.0, every row within `bar` of its
    own reference peak.  Returns the worst err / bar."""
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert bool(np.isfinite(got).all()), (run["id"], "non-finite output")
    z = run["zero_seq"]
    if z is not None:
        assert float(np.abs(ref[z]).max()) == 0.0
        peak = float(np.abs(got[z]).max())
        assert peak == 0.0, (run["id"], "the all-zero row", peak, locate(plan, z, int(np.abs(got[z]).argmax())), plan)
    rel, where = row_errors(got, ref)
    r = int(rel.argmax())
    err, loc = float(rel[r]), locate(plan, r, int(where[r]))
    ratio = err / bar
    if ratio >= _WORST.get(plan["kernel"], (-1.0,))[0]:
        _WORST[plan["kernel"]] = (ratio, run["id"])
    print(f"[fuzz-lfilter] {plan['kernel']} W={plan['W']} {run['id']} {run['regime']} n_seq={plan['n_seq']} L={plan['length']} "
          f"stages={plan['n_stages']} clamp={run['clamp']}: err={err:.3e} bar={bar:.1e} err/bar={ratio:.4f} (worst of this kernel so far "
          f"{_WORST[plan['kernel']][0]:.4f} {_WORST[plan['kernel']][1]}) at {loc}")
    assert err <= bar, (run["id"], "per-row", err, bar, ratio, loc, plan)
    return ratio


# --------------------------------------------------------------------------- #
# 4. the device tests                                                         #
# --------------------------------------------------------------------------- #

def device_numbers():
    """(CU count, LDS cap) as csrc/api_common.hip reads them, the CU count checked against aamd_device_info."""
    from audio_amd import _lib
    props = torch.cuda.get_device_properties(0)
    cu = int(props.multi_processor_count)
    name, cus, mem = C.create_string_buffer(128), C.c_int32(0), C.c_int64(0)
    _lib.check(_lib.lib().aamd_device_info(name, 128, C.byref(cus), C.byref(mem)))
    assert cus.value == cu and cu >= 8, (cus.value, cu)
    cap = int(getattr(props, "shared_memory_per_block_optin", 0) or LDS_CAP_DESIGN)
    return cu, cap


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from audio_amd import _lib
    _lib.lib()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def numbers(dev):
    return device_numbers()


def device_view(x, run, dev):
    """x (n_seq, L) as the (batch, channels, L) tensor the launcher gets: a contiguous view `offset` floats into a flat buffer."""
    flat = torch.empty(x.numel() + 4, dtype=torch.float32, device=dev)
    assert flat.data_ptr() % 16 == 0
    v = flat[run["offset"]:run["offset"] + x.numel()].view(run["batch"], run["channels"], run["L"])
    v.copy_(x.view(run["batch"], run["channels"], run["L"]))
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * run["offset"]
    return v


def lib_plan(xv, y, run):
    from audio_amd import _lib
    out = (C.c_int32 * 4)()
    _lib.check(_lib.lib().aamd_lfilter_plan(xv.data_ptr(), y.data_ptr(), run["batch"], run["channels"], run["L"], run["order"],
                                            run["stages"], out))
    return tuple(out)


def check_run(run, plan, dev, x=None):
    import audio_amd.functional as F
    fault = regime_fault(run, plan)
    assert fault is None, (run["id"], fault, "%d CUs" % plan["cu_count"], plan)
    x = make_inputs(run) if x is None else x
    xv = device_view(x, run, dev)
    assert (xv.data_ptr() % 16 != 0) == (run["offset"] != 0)
    a, b = torch.from_numpy(run["a"]).to(dev), torch.from_numpy(run["b"]).to(dev)
    with torch.no_grad():
        got = F._lfilter_launch(xv, a, b, run["clamp"], run["stages"])
        again = F._lfilter_launch(xv, a, b, run["clamp"], run["stages"])
    assert got.shape == xv.shape and got.is_contiguous() and got.data_ptr() % 16 == 0
    mine = (plan["kid"], plan["W"], plan["blocks"], plan["lds"])
    assert lib_plan(xv, got, run) == mine, (run["id"], lib_plan(xv, got, run), mine, plan)
    assert torch.equal(got, again), (run["id"], "a repeated call differs")
    got = got.view(run["n_seq"], run["L"]).cpu().numpy()
    ref = reference64(x, run["a"], run["b"], run["clamp"], run["channels"])
    n = min(run["L"], 3000)                                      # the reference form against the sequential oracle, first batch item
    pre = oracle64(x[:run["channels"], :n].double().numpy(), run["a"], run["b"], run["clamp"], run["channels"])
    assert float(np.abs(pre - ref[:run["channels"], :n]).max()) <= 1e-9, run["id"]
    return check_outputs(got, ref, plan, run, bar_of(run))


@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(len(CASES)), ids=CASE_IDS)
def test_fuzz_lfilter_kernels_in_multi_sequence_runs_vs_float64(idx, dev, numbers):
    run, plan = make_run(idx, *numbers)
    check_run(run, plan, dev)


def _tiny_run(L):
    case = _c("tiny-%d" % L, "tiny", WAVE8_VEC if L % 4 == 0 else WAVE8, 1, L, 2, (1, 3), rows=3)
    a, b = design_coeffs(case, 3)
    return dict(case, idx=-1, batch=1, channels=3, n_seq=3, crows=3, vec_ok=L % 4 == 0, a=a, b=b, seed=SEED_BASE + 5000 + L,
                scale=1.0, zero_seq=None)


@pytest.mark.gpu
def test_fuzz_lfilter_tiny_lengths_vs_oracle(dev, numbers):
    """Rows shorter than a lane's chunk, a wave's row of chunks and one block: 3 rows, per-channel 2-stage cascade, against the
    sequential oracle itself."""
    for L in TINY_LENGTHS:
        run = _tiny_run(L)
        plan = launch_plan(3, L, 3, 2, run["vec_ok"], 3, 3, *numbers)
        x = make_inputs(run)
        ratio = check_run(run, plan, dev, x)
        want = oracle64(x.double().numpy(), run["a"], run["b"], 1, 3)
        assert float(np.abs(want - reference64(x, run["a"], run["b"], 1, 3)).max()) <= 1e-12 and ratio <= 1.0


# --------------------------------------------------------------------------- #
# 5. no device: the mirror against lfw::pick, coverage, preconditions, bite   #
# --------------------------------------------------------------------------- #

def _against_header(n_seq, length, n_order, n_stages, vec_ok, cap, cu):
    import sim_util as S
    g = S.sim_lfw_pick(n_seq, length, n_order, n_stages, vec_ok, cap, cu)
    mine = pick(n_seq, length, n_order, n_stages, vec_ok, cap, cu)
    assert (g["kernel"], g["W"], g["blocks"], g["lds"]) == mine, (n_seq, length, n_order, n_stages, vec_ok, cap, cu, g, mine)
    return mine


def _sweep():
    r = np.random.default_rng(SEED_BASE)
    for n_seq in (1, 2, 6, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 3075, 4095, 4096, 4097, 5123, 70000):
        for length in (1, 100, 2047, 2048, 2049, 2052, 4096, 4097, 4100, 8192, 8193, 8196, 16384, 16385, 16388, 32768, 32772,
                       100000, 480000, (1 << 30) - 4, 1 << 30):
            yield n_seq, length, int(r.choice([1, 2, 3, 3, 4])), int(r.integers(1, 10)), bool(r.integers(0, 2))


def test_mirror_equals_lfw_pick():
    """pick() against lfw::pick itself for the shape of every case at 256, 64 and 8 CUs, and over a sweep of shapes on both sides
    of every threshold at four LDS caps."""
    n = 0
    for idx in range(len(CASES)):
        for cu in (CU_DESIGN, 64, 8):
            run, plan = make_run(idx, cu)
            assert cu != CU_DESIGN or regime_fault(run, plan) is None, (run["id"], regime_fault(run, plan))
            got = _against_header(plan["n_seq"], plan["length"], plan["n_order"], plan["n_stages"], plan["vec_ok"], LDS_CAP_DESIGN, cu)
            assert got == (plan["kid"], plan["W"], plan["blocks"], plan["lds"])
            n += 1
    for L in TINY_LENGTHS:
        _against_header(3, L, 3, 2, L % 4 == 0, LDS_CAP_DESIGN, CU_DESIGN)
    for n_seq, length, n_order, n_stages, vec_ok in _sweep():
        for cap, cu in ((LDS_CAP_DESIGN, 256), (64 * 1024, 304), (48 * 1024, 8), (20 * 1024, 64)):
            _against_header(n_seq, length, n_order, n_stages, vec_ok, cap, cu)
            n += 1
    assert n > 1500


def test_launch_plan_by_hand():
    """The mirror on numbers worked out by hand from csrc/lfilter_wave.h at 256 CUs and 160 KB."""
    assert lds_bytes(1, 1) == (2112 + 368 + 8 + 4) * 4 and pipe_lds_bytes(8, 8) == (8 * 4160 + 8 * 368 + 64 + 4) * 4 <= LDS_CAP_DESIGN
    assert pick(4096, 4100, 3, 4, True)[:3] == (WAVE8_VEC, 2, 2048) and pick(4097, 4100, 3, 4, True)[:3] == (WAVE8_VEC, 1, 2048)
    assert pick(4096, 2048, 3, 1, True)[1] == 1 and pick(2048, 4097, 3, 1, True)[1] == 4 and pick(2049, 4097, 3, 1, True)[1] == 2
    assert pick(1024, 8196, 3, 2, True)[:2] == (PIPE, 8) and pick(1025, 8196, 3, 2, True)[:2] == (WAVE8_VEC, 4)
    assert pick(1024, 8192, 3, 2, True)[:2] == (WAVE8_VEC, 4) and pick(1024, 8196, 3, 3, True)[:2] == (MOVER, 8)
    assert pick(512, 16388, 3, 3, False)[:2] == (WAVE16, 16) and pick(513, 16388, 3, 3, False)[:2] == (WAVE8, 8)
    assert pick(512, 16388, 3, 3, True) == (MOVER, 8, 512, pipe_lds_bytes(8, 3)) and pick(1, 16384, 3, 1, True)[:2] == (PIPE, 8)
    assert pick(6, 9000, 4, 1, True)[0] == GENERAL and pick(6, 9000, 3, 9, True)[0] == GENERAL and pick(1, 1 << 30, 3, 1, True)[0] == GENERAL
    assert pick(1, 70001, 3, 1, False, 64 * 1024)[:2] == (WAVE8, 4)            # a 64 KB device: 16 and 8 tiles do not fit, W halves to 4
    p = launch_plan(3075, 6148, 3, 4, True, 3, 3)
    assert (p["blocks"], p["n_blocks"], p["rebuilds"], p["kept"], p["seqs_per_wg_max"], p["seqs_per_wg_min"]) == (2048, 2, True, False, 2, 1)
    w = locate(p, 2050, 4096 + 40)
    assert (w["workgroup"], w["position"], w["run_length"], w["block"], w["wave"], w["lane"], w["crow"]) == (2, 1, 2, 1, 0, 1, 1)
    assert launch_plan(4096, 4100, 3, 2, True, 4, 4)["kept"] and not launch_plan(2048, 4100, 3, 2, True, 4, 4)["kept"]


def test_wave16_vec_is_never_picked():
    """lfilter_wave_kernel<0, 16, true> is unreachable at a 160 KB cap (and at any cap that holds the two-tile layout): aligned
    rows with W >= 8 take pipe or mover because pipe_lds_bytes(8, n) <= 160 KB for every n <= 8.  (the
    instantiation is still compiled.)"""
    assert all(pipe_lds_bytes(8, n) <= LDS_CAP_DESIGN for n in range(1, MAX_CASCADE + 1))
    seen = set()
    for n_seq, length, _, _, _ in _sweep():
        for n_order in (1, 2, 3):
            for n_stages in range(1, MAX_CASCADE + 1):
                for vec_ok in (False, True):
                    for cu in (8, 128, 256, 304):
                        seen.add(pick(n_seq, length, n_order, n_stages, vec_ok, LDS_CAP_DESIGN, cu)[0])
    assert seen == {GENERAL, WAVE8_VEC, WAVE8, WAVE16, PIPE, MOVER}


def test_pipe_and_mover_run_one_sequence_per_workgroup():
    """W >= 8 needs n_seq <= 1024 = 8 x 128: from 128 CUs on, a pipe / mover workgroup never starts a second sequence (their
    sequence loops run once; the many-sequence regime is the one-tile kernel's)."""
    for n_seq, length, _, _, _ in _sweep():
        for n_stages in (1, 2, 3, 8):
            for cu in (128, 256, 304):
                kid, W, blocks, _ = pick(n_seq, length, 3, n_stages, True, LDS_CAP_DESIGN, cu)
                assert kid not in (PIPE, MOVER) or (n_seq <= blocks and n_seq <= 1024), (n_seq, length, n_stages, cu)
    assert pick(1024, 8196, 3, 3, True, LDS_CAP_DESIGN, 64)[2] == 512       # (a 64-CU device would run two)


def test_cases_cover_the_gaps():
    """What the cases pin, from the mirror at 256 CUs; a change of a case, of the sizing or of the W rule cannot silently lose one."""
    assert len(set(CASE_IDS)) == len(CASES)
    every = [make_run(idx) for idx in range(len(CASES))]
    for r, p in every:
        assert regime_fault(r, p) is None, (r["id"], regime_fault(r, p))
        assert p["n_seq"] * p["length"] * 4 <= 76e6, (r["id"], p["n_seq"] * p["length"] * 4)
    assert {p["kernel"] for _, p in every} == KERNELS_WANTED and len(KERNELS_WANTED) == 5
    ms = [(r, p) for r, p in every if r["regime"] == "many-seq"]
    # gap 1: second sequences at W = 1 and W = 2, aligned and not, 1 / 2 / 4 stages, tables rebuilt (3 rows) and kept (1, 2, 4)
    assert {(p["W"], p["n_seq"], p["length"]) for _, p in ms} == {(1, 5123, 2085), (1, 5124, 2085), (1, 5124, 2088), (1, 5123, 2088), (1, 4097, 4096),
                                                                   (2, 4096, 4100), (2, 4096, 4101), (2, 3075, 6148), (2, 3075, 6150),
                                                                   (2, 3075, 6149)}
    for W in (1, 2):
        assert {(p["n_stages"], p["vec_ok"]) for _, p in ms if p["W"] == W} >= {(1, True), (2, True), (4, True), (2, False)} - \
            ({(1, True)} if W == 1 else set()), W
        assert {r["crows"] for r, p in ms if p["W"] == W} >= {1, 3} and any(p["rebuilds"] for _, p in ms if p["W"] == W)
    assert {r["crows"] for r, p in ms if p["kept"]} == {1, 2, 4} and {r["crows"] for r, p in ms if p["rebuilds"]} == {3}
    assert all(p["blocks"] == 2048 and p["n_blocks"] == 2 for _, p in ms)
    assert all(locate(p, 0, 4096)["wave"] == 0 and p["length"] - 4096 <= 5 for _, p in ms if p["n_seq"] == 4096)
    for r, p in every:
        z = r["zero_seq"]
        assert (z is not None) == (p["seqs_per_wg_max"] >= 2), r["id"]
        if z is not None:
            assert locate(p, z, 0)["position"] == 1 and GAINS[(z - p["blocks"]) % 4] == 1.0 and z - p["blocks"] != z
    # gap 2: rows that ARE unaligned: offsets 1, 2, 3 with L % 4 == 0, L % 4 != 0, W 4 / 8 / 16, 1 / 2 / 3 / 5 / 8 stages
    un = [(r, p) for r, p in every if r["regime"] == "unaligned"]
    assert {r["offset"] for r, p in un if p["length"] % 4 == 0} == {1, 2, 3} and any(r["offset"] == 0 and p["length"] % 4 for r, p in un)
    assert {p["W"] for _, p in un} == {4, 8, 16} and {p["n_stages"] for _, p in un} == {1, 2, 3, 5, 8}
    assert {p["n_blocks"] for _, p in un} == {3, 4} and all(p["length"] % p["block_len"] for _, p in un)
    assert {(p["kid"], p["n_stages"] > 1 and p["n_stages"] % 2 == 1) for _, p in un} >= {(WAVE8, True), (WAVE16, True)}
    # gap 3: slow poles on <0, 16, false>, pipe with 1 and 2 stages, mover with 3 and 4, W = 2 many-sequences
    slow = [(r, p) for r, p in every if r["regime"] in ("slow", "slow-many")]
    assert {(p["kid"], p["n_stages"]) for _, p in slow} == {(WAVE16, 1), (PIPE, 1), (PIPE, 2), (MOVER, 3), (MOVER, 4), (WAVE8_VEC, 1)}
    assert all(r["clamp"] == 0 and r["scale"] == 0.1 and p["n_blocks"] >= 3 for r, p in slow)
    assert all(len(set(r["design"])) == len(r["design"]) for r, _ in slow) and any(p["W"] == 2 and p["seqs_per_wg_max"] == 2 for _, p in slow)
    # gap 4: pipe / mover edges
    pm = [(r, p) for r, p in every if r["regime"] == "edges"]
    assert {p["length"] for _, p in pm} == {8196, 12292, 16384, 16388} and {p["n_seq"] for _, p in pm} == {1, 6, 1024, 1025}
    for kid in (PIPE, MOVER):
        mine = [(r, p) for r, p in pm if p["kid"] == kid]
        assert {r["clamp"] for r, _ in mine} == {0, 1, 2} and {p["n_blocks"] for _, p in mine} == {1, 2} and any(r["crows"] > 1 for r, _ in mine)
        assert any(p["n_seq"] == 1024 for _, p in mine) and {r["order"] for r, _ in mine} >= {3, 1 if kid == MOVER else 2}
        assert any(p["length"] == 8196 for _, p in mine)          # waves 5 .. 7 wholly past the end
    assert {p["n_stages"] for _, p in pm} == {1, 2, 3, 8} and {r["order"] for r, _ in pm} == {1, 2, 3}
    assert sum(r["design"] == "mixed" for r, _ in pm) == 2
    assert [(p["kid"], p["W"]) for r, p in pm if p["n_seq"] == 1025] == [(WAVE8_VEC, 4)]
    print("[fuzz-lfilter] gaps pinned: 5 kernels; second sequences at W = 1, 2 with tables rebuilt and kept; unaligned bases 1, 2, 3 at "
          "W = 4, 8, 16; slow poles on 4 kernels; pipe / mover edges; the zero row")


@pytest.mark.parametrize("idx", [i for i, c in enumerate(CASES) if c["regime"] in ("slow", "slow-many")],
                         ids=[c["id"] for c in CASES if c["regime"] in ("slow", "slow-many")])
def test_slow_pole_designs_meet_the_replay_bar(idx):
    """The precondition of the slow-pole device cases, on row 0 of the case's own input: the CPU replay of lfw's phase functions
    at the case's W stays <= 4e-5 of the float64 peak (the bar of test_sim_lfilter_wave_slowly_decaying_poles_across_waves)."""
    import sim_util as S
    run, plan = make_run(idx)
    run = dict(run, zero_seq=None)
    x = make_inputs(run)[:1]
    a, b = run["a"][:, :1], run["b"][:, :1]
    rc, got = S.sim_lfilter_wave(x.numpy()[None], a, b, 0, plan["W"])
    ref = reference64(x, a, b, 0, 1)
    err = float(row_errors(got[0], ref)[0].max())
    print(f"[fuzz-lfilter] replay {run['id']} W={plan['W']} r,t={[SLOW[i] for i in run['design']]}: err={err:.3e} bar={REPLAY_BAR:.1e}")
    assert rc == 0 and err <= REPLAY_BAR, (run["id"], err)


CONTEXT_CASES = ("ms-w2-ch3-4st-6148", "ms-w2-shared-4st-4101", "pm-6x12292-2st-c0", "pm-6x16384-3st-c2",
                 "slow-w16", "slow-pipe-1st", "slow-pipe-2st", "slow-mover-3st", "slow-mover-4st", "slow-w2-many")


@pytest.mark.parametrize("cid", CONTEXT_CASES)
def test_float32_sequential_recursion_context(cid):
    """A float32 sequential recursion on rows 0 .. 3 of the case against the same float64 reference: what plain float32 costs, to
    read the kernels' err / bar against.  On a slow-pole case it must itself meet the bar, else the design is too resonant."""
    run, plan = make_run(CASE_IDS.index(cid))
    run = dict(run, zero_seq=None)
    seqs = np.arange(min(4, run["n_seq"]))
    x = make_inputs(run)[:4]
    got = float32_sequential(x, run["a"], run["b"], run["clamp"], run["channels"], seqs)
    ref = reference64(x, run["a"], run["b"], run["clamp"], run["channels"], seqs)
    ratio = float(row_errors(got, ref)[0].max()) / bar_of(run)
    print(f"[fuzz-lfilter] float32 sequential {cid} ({plan['kernel']}): err/bar={ratio:.4f}")
    assert ratio <= 1.0, (cid, ratio)


# ---- bite: float64 models of a persistent workgroup on this file's inputs -----------------------------------------------------------

BITE_BLOCKS, BITE_SEQS, BITE_L = 4, 12, 300           # sequences 0, 4, 8 / 1, 5, 9 / 2, 6, 10 / 3, 7, 11 on four workgroups: 4 % 3 != 0
# measured with the shapes below: (peak of the all-zero row, err / bar of the rows behind the first of each workgroup: least .. worst)
BITE_MEASURED = {"carry": (0.0862, 1.58e3, 5.32e3), "tables": (0.0, 2.79e3, 1.86e4), "history": (0.0101, 10.8, 657.0)}


def _bite_run(stages=2, crows=3, clamp=1):
    case = _c("bite", "bite", WAVE8_VEC, 1, BITE_L, stages, (4, 3), clamp=clamp, rows=3 if crows == 3 else "shared")
    a, b = design_coeffs(case, 3)
    run = dict(case, idx=-2, batch=4, channels=3, n_seq=BITE_SEQS, crows=crows, vec_ok=True, a=a, b=b, seed=SEED_BASE + 9000, scale=1.0)
    plan = launch_plan(BITE_SEQS, BITE_L, 3, stages, True, 3, crows)
    plan.update(blocks=BITE_BLOCKS, seqs_per_wg_max=3, seqs_per_wg_min=3, kernel="model")
    run["zero_seq"] = zero_row_of(plan)
    assert run["zero_seq"] == BITE_BLOCKS and GAINS[0] == 1.0 and BITE_BLOCKS % 3 != 0
    return run, plan


def workgroup_model(x, run, fault=None):
    """The cascade in float64, sample by sample, as BITE_BLOCKS persistent workgroups run it.  fault "carry": a sequence behind the
    first of its workgroup starts every stage's recursion from the state the previous sequence left (the exchange area not
    zeroed); "tables": it is filtered with the coefficient row of the previous sequence (the fp64 tables not rebuilt); "history":
    stage 0 of every sequence behind the first reads the previous sequence's last two inputs as x[-1], x[-2] (the history row
    taken although nw0 == 0)."""
    ah, bh = normalised(run["a"], run["b"])
    n_stages, L = run["stages"], x.shape[1]
    out = np.zeros((run["n_seq"], L))
    for wg in range(BITE_BLOCKS):
        state = [(0.0, 0.0)] * n_stages
        prev = None
        for seq in range(wg, run["n_seq"], BITE_BLOCKS):
            crow = (seq % run["channels"]) if run["crows"] > 1 else 0
            if fault == "tables" and prev is not None:
                crow = (prev % run["channels"]) if run["crows"] > 1 else 0
            v = x[seq].astype(np.float64)
            for st in range(n_stages):
                a1, a2 = ah[st, crow, 1], ah[st, crow, 2]
                b0, b1, b2 = bh[st, crow]
                y1, y2 = state[st] if (fault == "carry" and prev is not None) else (0.0, 0.0)
                x1, x2 = (x[prev, -1], x[prev, -2]) if (fault == "history" and prev is not None and st == 0) else (0.0, 0.0)
                o = np.empty(L)
                for n in range(L):
                    w = b2 * x2 + b1 * x1 + b0 * v[n]
                    y = w - a2 * y2 - a1 * y1
                    o[n] = y
                    x2, x1, y2, y1 = x1, v[n], y1, y
                state[st] = (y1, y2)
                v = np.clip(o, -1.0, 1.0) if stage_clamps(run["clamp"], st, n_stages) else o
            out[seq] = v
            prev = seq
    return out


@pytest.mark.parametrize("fault,crows", [("carry", 1), ("tables", 3), ("history", 1)])
def test_bite_faults_of_the_second_sequence(fault, crows):
    """The honest model passes the checks of the device runs; each fault leaves the first sequence of every workgroup alone and puts
    every later non-zero row > 10 x the bar out ("carry" and "history" also make the all-zero row non-zero), and check_outputs
    raises."""
    run, plan = _bite_run(crows=crows)
    x = make_inputs(run).numpy()
    ref = reference64(x, run["a"], run["b"], run["clamp"], run["channels"])
    bar = bar_of(run)
    honest = workgroup_model(x, run)
    assert float(row_errors(honest, ref)[0].max()) <= 1e-12
    check_outputs(honest.astype(np.float32), ref, plan, run, bar)
    bad = workgroup_model(x, run, fault)
    rel = row_errors(bad, ref)[0]
    # (behind the all-zero row the carry and the history are zeros: that row is the model's blind spot, not the check's)
    later = [s for s in range(BITE_BLOCKS, BITE_SEQS) if s != run["zero_seq"] and (fault == "tables" or s - BITE_BLOCKS != run["zero_seq"])]
    zero_peak = float(np.abs(bad[run["zero_seq"]]).max())
    print(f"[fuzz-lfilter] bite {fault}: zero row peak {zero_peak:.3g}, later rows err/bar {min(rel[later]) / bar:.3g} .. "
          f"{max(rel[later]) / bar:.3g}")
    assert all(rel[s] <= 1e-12 for s in range(BITE_BLOCKS)) and min(rel[later]) >= 10.0 * bar, (fault, rel / bar)
    if fault == "tables":
        assert zero_peak == 0.0
        with pytest.raises(AssertionError, match="per-row"):
            check_outputs(bad.astype(np.float32), ref, plan, run, bar)
    else:
        assert zero_peak > 10.0 * bar
        with pytest.raises(AssertionError, match="all-zero row"):
            check_outputs(bad.astype(np.float32), ref, plan, run, bar)
        with pytest.raises(AssertionError, match="per-row"):
            check_outputs(bad.astype(np.float32), ref, plan, dict(run, zero_seq=None), bar)


def test_reference_forms_agree():
    """reference64 (scipy, rows of one coefficient row at a time) against the sequential oracle on whole short rows: shared and
    per-channel rows, every clamp mode, every n_order, zero-padded mixed stages."""
    for cid, L in (("pm-6x12292-2st-c0", 700), ("pm-6x16384-3st-c2", 500), ("pm-6x8196-8st-mixed-c0", 400), ("pm-6x12292-3st-gain", 300),
                   ("pm-6x16384-2st-order1", 300), ("slow-mover-4st", 900)):
        run, _ = make_run(CASE_IDS.index(cid))
        run = dict(run, L=L, zero_seq=1)
        x = make_inputs(run)
        have = reference64(x, run["a"], run["b"], run["clamp"], run["channels"])
        want = oracle64(x.double().numpy(), run["a"], run["b"], run["clamp"], run["channels"])
        assert have.shape == want.shape and float(np.abs(have - want).max()) <= 1e-12, cid
        assert float(np.abs(have[1]).max()) == 0.0
        part = reference64(x, run["a"], run["b"], run["clamp"], run["channels"], seqs=[2, 1, 3])
        assert np.array_equal(part, have[[2, 1, 3]])
