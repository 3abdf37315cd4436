"""Every FFT kernel behind F.fftconvolve (csrc/fftconv_fdr.h, csrc/fftconv_os.h, launched by aamd_fftconvolve_staged_f32 in
csrc/api_fftconv.hip) in MULTI-ITEM launches against float64: fdr::delay_line_kernel<1 | 2 | 3 | 4> (plan 3, 193 .. 32768 taps),
fco::overlap_save_kernel with 2 .. 4 partitions (plan 1 under POLICY_FFTCONV_NO_FDL) and with >= 5 (the DEFAULT above 32768 taps),
fco::overlap_save_fdl_kernel<2 | 3 | 4> (plan 2 under POLICY_FFTCONV_FDL) -- nine launch targets -- with the two spectrum_kernels
behind them on one tap row, on four and on one per output row, and fftconv_direct_kernel once at 192 taps next to 193.

Why: the workgroups are persistent -- the launcher starts blocks = min(cu_count, items) of them and each loops
`for (item = blockIdx.x; item < n_items; item += gridDim.x)` -- and the cost models cut few long rows into rows * segs <= cu_count
segments, so the shapes of the suite give a workgroup ONE item: delay_line_kernel<1> and <2> had never started a second item on a
device, <3> and <4> in one case each, the complex delay line only for NP = 3, and more than 32768 taps (n_part >= 5, a default
route of a public op) had never been compared with anything.  What only acts from the second item on: no barrier between an
item's last-pass reads and the next item's first-pass writes (a comment says why that is safe), pair_sync's arrival counters and
pair_gen growing across items, vin / vout flipping row by row when nx or out_len is odd, overlap_save_kernel fetching the NEXT
item's inputs (another row) during the current item's stores, zp0 / zp1 of the complex delay line zeroed once before the item loop
and its per-workgroup ring reused by every item with wslot reset.

launch_plan() is a host mirror of the launcher (operand swap, kFftConvMinTaps, fftconv_pick_fdr / _pick_fdl, fdr::plan, fco::plan,
fco::plan_fdl); every device run ASSERTS the regime it claims from the mirror with the device's own CU count (checked against
aamd_device_info) and the mirrored plan number against aamd_fftconvolve_plan: on another device a case is re-sized by the mirror
or fails loudly, it does not pass vacuously.  Regimes:

  many-rows  rows = 2.5 x blocks + 3 (643 at 256 CUs), nx just long enough for 2 .. 8 blocks: every workgroup runs >= 2 items,
             some >= 3, items % blocks != 0; one item per row where the mirror says segs == 1 (193 / 8192 taps: three one-block
             segments per row, 8 items per workgroup)
  segmented  rows in [CU / 2, CU), the shortest nx for which the mirror gives segs >= 2, seg_blocks >= 2, a shorter last segment
             and >= 2 items on every workgroup: a segment with j_lo > 0 warms its delay line up on real samples of the same row,
             consecutive items of a workgroup lie in different rows
  long-taps  32769 / 40000 / 49153 taps (n_part 5, 5, 7) on the default policy, valid / same / full, with 3 rows and with
             rows * n_pairs = 2.5 x blocks + 3 (the cross-item prefetch runs)
  policy     the many-rows shapes of NP 2, 3, 4 under POLICY_FFTCONV_FDL (plan 2) and POLICY_FFTCONV_NO_FDL (plan 1)
  boundary   192 taps: the time-domain kernel, one tile per workgroup
Layouts, spread over the cases (test_cases_cover_the_gaps lists what each pins): odd nx and out_len, odd `start` (the scalar
load_block path), both ends of every NP (193, 8192, 8193, 16384, 16385, 24576, 24577, 32768) and a partial last partition
(12345); shared taps, per-row taps once per kernel family, the broadcast maps x (R, 1, nx) / (R, 4, nx) against y (1, 4, ny),
the operand swap once, and in two cases a third call that runs RUN-only against the workspace kept with the tap tensor.

Inputs: standard normal float32 rows with gains cycling 1, 1e-3, 1e-2, 1; one all-zero row placed where the mirror shows it as the
second or third item of a workgroup behind a gain-1 row; taps 0.2 * randn, flat (late partitions weigh as much as the first).
Reference: the float64 linear convolution of the stored float32 operands -- torch.fft.rfft / irfft in float64 on the device at
n = the next power of two >= nx + ny - 1, slab by slab of rows (a slab's complex128 spectra <= 256 MB), sliced as the product
slices; test_reference_forms_agree holds it against oracle.dsp_oracle.fftconvolve (1e-12 of the peak).  Every output is compared.

Bars (none is new, none is derived from the product's output):
  2e-5 peak-relative (tests/test_gpu_fuzz.py::test_fuzz_fftconvolve_vs_fft, the same flat taps), PER OUTPUT ROW against that row's
      own reference peak: an item transforms one row's samples only, so its error scales with the row; a whole-tensor peak takes a
      quiet row's gain off the margin.  The CPU replay of the same headers stays <= 4.5e-7 per row (2 % of the bar) on every plan.
  the all-zero row: exactly 0.0 (transforms of zeros are zeros, the taps are finite)
  repeated and RUN-only calls: bit-equal
A failure prints the worst element's locate() record (item, workgroup, position in the workgroup's run, block in the segment,
first / last block, warm-up neighbour), err / bar and the mirrored plan.

Device-free tests: the mirror against fdr::plan / fco::plan / fco::plan_fdl themselves (sim_fdr_plan / sim_fco_plan of the CPU
replay) for every run's shape at 256, 8 and 5 CUs, the coverage at 256 CUs, the reference forms, and bite tests (BITE_MEASURED): float64
block-wise overlap-save models of a second item that starts from the previous item's delayed spectra (NP 2, 3, 4), of a delay
slot read one step out of order (NP 4) and of a next-item prefetch from the previous item's row (plan 1), each far above the bar.

Measured on an MI355X (256 CUs): MEASURED_DEVICE; wall time FILE_SECONDS.  No case found a kernel wrong: the worst per-row
err / bar is 0.021 among the nine FFT kernels (0.047 for the time-domain kernel at 192 taps), every all-zero row came out 0.0 and
every RUN-only call bit-equal.  The segmented cases of NP 3 and 4 run 136 rows, not the 160 .. 200 first thought of: at 160 rows
the cost model gives 3 segments (480 items: half the workgroups run ONE item), and with 4 segments on 256 workgroups every item
of a workgroup starts on a row of the same parity; 136 rows give 5 segments, 2 or 3 items on every workgroup and vin / vout
flipping between them.

That the DEVICE cases bite was checked once by hand against a library with two precision-only faults (in bounds; that build
is not committed): (1) delay_line_kernel started every item behind the first of its workgroup at j_lo, without the NP - 1
forward-only steps; (2) overlap_save_kernel took the next item's first inputs from the CURRENT item's row.  16 of the 28 device
tests failed and 12 passed, exactly as the faults predict: (1) every plan-3 case of NP >= 2 whose later items have samples in
front of them -- the six `same` / `valid` many-rows cases (err / bar 1.7e3 .. 4.8e4) and the three segmented ones (109 .. 4.5e4;
their first segments start on zeros) -- while NP 1 (no delay line) and the `full` many-rows cases (a row's warm-up blocks lie
in front of the signal: zeros either way) passed; (2) all seven plan-1 cases, the three beyond 32768 taps included, each at the
all-zero row (peaks of 53 .. 74 where 0.0 is asked, at the second or third item of a workgroup: items 256 .. 259).  The
complex delay line (plan 2) and the time-domain kernel were not touched and passed.
"""
import ctypes as C

import numpy as np
import pytest
import torch

CU_DESIGN = 256
BAR = 2e-5
MIN_TAPS = 192                                                      # csrc/api_fftconv.hip kFftConvMinTaps
FDR_N, FDR_HOP, FDR_MAX_PARTS = 16384, 8192, 4                      # csrc/fftconv_fdr.h kN, kHop, kMaxParts
FCO_N, FCO_MAX_PART_TAPS, FCO_HOP, FCO_MAX_FDL = 16384, 8192, 8192, 4     # csrc/fftconv_os.h kN, kMaxPartTaps, kHop, kMaxFdlParts
DIRECT_TILE = 1024                                                  # csrc/fftconv.h kFcTN
POLICY_GENERIC, POLICY_NO_FDL, POLICY_FDL, POLICY_COMPLEX = 1, 16, 32, 64     # audio_amd/_lib.py
GAINS = (1.0, 1e-3, 1e-2, 1.0)
SEED_BASE = 77300

# measured on an MI355X (256 CUs), one run of this file with -s: kernel -> (worst per-row err / bar, its case) from the
# "[fuzz-fftconv]" lines
MEASURED_DEVICE = {
    "fdr::delay_line_kernel<1>": (0.0182, "mr-193-same"), "fdr::delay_line_kernel<2>": (0.0200, "mr-12345-full"),
    "fdr::delay_line_kernel<3>": (0.0200, "mr-24576-same"), "fdr::delay_line_kernel<4>": (0.0190, "mr-32768-same"),
    "fco::overlap_save_kernel n_part 2..4": (0.0212, "os-32768-full"), "fco::overlap_save_kernel n_part >= 5": (0.0204, "lt-32769-valid"),
    "fco::overlap_save_fdl_kernel<2>": (0.0191, "fdl-8193-same"), "fco::overlap_save_fdl_kernel<3>": (0.0207, "fdl-16385-valid"),
    "fco::overlap_save_fdl_kernel<4>": (0.0195, "fdl-24577-same"), "fftconv_direct_kernel": (0.0467, "direct-192-same"),
}
# the 28 device tests of this file together: 8.0 s of pytest wall time (3.5 s for the first case, which loads the library; 0.5 .. 1 s
# for three cases of 20 .. 70 MB, under 0.1 s for every other: a launch and its float64 reference are milliseconds of device time)
# -- 2 % on top of the 425 s the device suite took at the parent commit (1 251 tests; with them 401 s on another day's machine,
# 1 279 tests)
FILE_SECONDS = 8.0


# --------------------------------------------------------------------------- #
# 1. the host mirror of the launch arithmetic                                 #
# --------------------------------------------------------------------------- #

def _cdiv(a, b):
    return -(-a // b)


def fdr_plan(rows, ny, out_len, cu):
    """fdr::plan: None when plan 3 does not serve the shape."""
    n_part = _cdiv(ny, FDR_HOP)
    if n_part < 1 or n_part > FDR_MAX_PARTS or ny < 2:
        return None
    skip = ny - 1 if n_part == 1 else FDR_HOP
    hop = FDR_N - skip
    n_blocks = _cdiv(out_len, hop)
    if rows < 1 or n_blocks < 1 or cu < 1:
        return None
    best, pick = -1, (1, n_blocks)
    for segs in range(1, min(1024, n_blocks) + 1):
        sb = _cdiv(n_blocks, segs)
        used = _cdiv(n_blocks, sb)
        cost = _cdiv(rows * used, cu) * (2 * sb + (n_part - 1))
        if best < 0 or cost < best:
            best, pick = cost, (used, sb)
    return dict(n_part=n_part, hop=hop, skip=skip, segs=pick[0], n_blocks=n_blocks, seg_blocks=pick[1])


def fco_plan(ny, out_len):
    """fco::plan."""
    n_part = _cdiv(ny, FCO_MAX_PART_TAPS)
    part_taps = _cdiv(ny, n_part)
    v = FCO_N - part_taps + 1
    n_blocks = _cdiv(out_len, v)
    return dict(n_part=n_part, part_taps=part_taps, v=v, n_blocks=n_blocks, n_pairs=(n_blocks + 1) // 2)


def fco_plan_fdl(rows, ny, out_len, cu):
    """fco::plan_fdl: (cheaper, dict(n_part, segs, n_blocks, seg_blocks))."""
    f = dict(n_part=_cdiv(ny, FCO_HOP), n_blocks=_cdiv(out_len, FCO_HOP), segs=1)
    f["seg_blocks"] = f["n_blocks"]
    if f["n_part"] < 2 or f["n_part"] > FCO_MAX_FDL or rows < 1 or f["n_blocks"] < 2 or cu < 1:
        return False, f
    g = fco_plan(ny, out_len)
    old_cost = _cdiv(rows * g["n_pairs"], cu) * (g["n_part"] + 1)
    best = -1
    segs = 1
    while segs <= 1024 and segs * 2 <= f["n_blocks"]:
        sb = _cdiv(f["n_blocks"], segs)
        hn = (sb + 1) // 2
        used = _cdiv(f["n_blocks"], sb)
        cost = _cdiv(rows * used, cu) * (2 * hn + f["n_part"] - 1)
        if best < 0 or cost < best:
            best, f["segs"], f["seg_blocks"] = cost, used, sb
        segs += 1
    return best > 0 and best * 10 <= old_cost * 9, f


def conv_slice(nx, ny, mode):
    """(start, out_len) of functional._fftconvolve_eager."""
    n_full = nx + ny - 1
    if mode == "full":
        return 0, n_full
    if mode == "valid":
        out_len = max(nx, ny) - min(nx, ny) + 1
        return (n_full - out_len) // 2, out_len
    assert mode == "same", mode
    return (n_full - nx) // 2, nx


def launch_plan(rows, nx, ny, mode, policy=0, cu_count=CU_DESIGN):
    """aamd_fftconvolve_staged_f32 for `rows` output rows of F.fftconvolve(x (.., nx), y (.., ny), mode) under `policy` on a
    device of `cu_count` CUs.  plan: 0 time-domain, 1 fco::overlap_save_kernel, 2 fco::overlap_save_fdl_kernel<np>,
    3 fdr::delay_line_kernel<np>.  An item is a (row, segment): `ipr` items per row, item = row * ipr + segment, a segment is
    `seg_blocks` blocks of `hop` outputs (plan 1: a pair of blocks; plan 0: one tile); workgroup w runs the items w, w + blocks, ..."""
    start, out_len = conv_slice(nx, ny, mode)
    swap = ny > nx
    nxa, taps = (ny, nx) if swap else (nx, ny)
    p = dict(rows=rows, nx=nx, ny=ny, mode=mode, policy=policy, cu_count=cu_count, start=start, out_len=out_len, swap=swap,
             nxa=nxa, taps=taps)
    fdr = fdr_plan(rows, taps, out_len, cu_count) if not policy & (POLICY_NO_FDL | POLICY_FDL | POLICY_COMPLEX) else None
    if taps <= MIN_TAPS or policy & POLICY_GENERIC:
        n_tiles = _cdiv(out_len, DIRECT_TILE)
        p.update(plan=0, np=0, hop=DIRECT_TILE, skip=0, n_blocks=n_tiles, segs=n_tiles, seg_blocks=1, ipr=n_tiles,
                 items=rows * n_tiles, blocks=rows * n_tiles, kernel="fftconv_direct_kernel")
    elif fdr is not None:
        p.update(plan=3, np=fdr["n_part"], hop=fdr["hop"], skip=fdr["skip"], n_blocks=fdr["n_blocks"], segs=fdr["segs"],
                 seg_blocks=fdr["seg_blocks"], ipr=fdr["segs"], kernel="fdr::delay_line_kernel<%d>" % fdr["n_part"])
    else:
        np_fdl = _cdiv(taps, FCO_HOP)
        if policy & POLICY_NO_FDL or np_fdl < 2 or np_fdl > FCO_MAX_FDL:
            np_fdl = 0
        cheaper, f = fco_plan_fdl(rows, taps, out_len, cu_count) if np_fdl else (False, None)
        if np_fdl and (cheaper or (policy & POLICY_FDL and f["n_blocks"] >= 2)):
            p.update(plan=2, np=f["n_part"], hop=FCO_HOP, skip=FCO_HOP, n_blocks=f["n_blocks"], segs=f["segs"],
                     seg_blocks=f["seg_blocks"], ipr=f["segs"], kernel="fco::overlap_save_fdl_kernel<%d>" % f["n_part"])
        else:
            g = fco_plan(taps, out_len)
            p.update(plan=1, np=g["n_part"], hop=g["v"], skip=g["part_taps"] - 1, n_blocks=g["n_blocks"], segs=g["n_pairs"],
                     seg_blocks=2, ipr=g["n_pairs"], part_taps=g["part_taps"],
                     kernel="fco::overlap_save_kernel n_part " + ("1" if g["n_part"] == 1 else "2..4" if g["n_part"] <= 4 else ">= 5"))
    if p["plan"]:
        p["items"] = rows * p["ipr"]
        p["blocks"] = min(cu_count, p["items"])
    p["items_per_wg_max"] = _cdiv(p["items"], p["blocks"]) if p["items"] else 0
    p["items_per_wg_min"] = p["items"] // p["blocks"] if p["items"] else 0
    return p


def items_on(plan, wg):
    return _cdiv(plan["items"] - wg, plan["blocks"])


def segment_of(plan, j):
    """(segment, j_lo, j_hi) of block j of a row."""
    seg = j // plan["seg_blocks"]
    j_lo = seg * plan["seg_blocks"]
    return seg, j_lo, min(j_lo + plan["seg_blocks"], plan["n_blocks"])


def block_s0(plan, j):
    """First input sample of block j (plan 3: fdr::seg_start; plan 2: fco::fdl_seg_start; plan 1: fco::block_s0, partition 0)."""
    return plan["start"] + j * plan["hop"] - plan["skip"]


def locate(plan, row, sample, sig_row=None):
    """Where the launch computes output `sample` of output row `row` (sig_row: the row of the streamed operand it reads)."""
    j = sample // plan["hop"]
    seg, j_lo, j_hi = segment_of(plan, j)
    item = row * plan["ipr"] + seg
    wg, pos = item % plan["blocks"], item // plan["blocks"]
    rec = dict(row=row, sample=sample, block=j, segment=seg, item=item, workgroup=wg, position=pos, run_length=items_on(plan, wg),
               block_in_segment=j - j_lo, first_block=j == j_lo, last_block=j == j_hi - 1, kernel=plan["kernel"])
    if plan["plan"] == 2:                      # two halves of the segment walk side by side: step s holds blocks j_lo + s, j_lo + hn + s
        hn = (j_hi - j_lo + 1) // 2
        rec.update(step=(j - j_lo) % hn, half=(j - j_lo) // hn)
        rec["warm_up_neighbour"] = rec["step"] < plan["np"] - 1
    elif plan["plan"] == 3:
        rec["warm_up_neighbour"] = j - j_lo < plan["np"] - 1          # a delayed spectrum of this block is a forward-only step's
        sr = row if sig_row is None else sig_row
        rec.update(vin=(sr * plan["nxa"]) % 2 == 0, vout=(row * plan["out_len"]) % 2 == 0, s0_odd=block_s0(plan, j) % 2 == 1)
    else:
        rec["warm_up_neighbour"] = False
    return rec


def regime_fault(run, plan):
    """None when `plan` is what `run` claims, else what it misses (every device run asserts this on the device's CU count)."""
    cu, regime = plan["cu_count"], run["regime"]
    if plan["kernel"] != run["kernel"]:
        return "kernel %s, not %s" % (plan["kernel"], run["kernel"])
    if plan["swap"] != (run["layout"] == "swap"):
        return "operand swap %s" % plan["swap"]
    if regime == "boundary":
        return None if plan["plan"] == 0 and plan["taps"] == MIN_TAPS else "plan %d at %d taps" % (plan["plan"], plan["taps"])
    if regime in ("many-rows", "policy", "long-many"):
        if plan["items"] < int(2.5 * cu) + 3 or plan["items"] % plan["blocks"] == 0:
            return "%d items on %d workgroups" % (plan["items"], plan["blocks"])
        if plan["items_per_wg_min"] < 2 or plan["items_per_wg_max"] < 3:
            return "items per workgroup %d .. %d" % (plan["items_per_wg_min"], plan["items_per_wg_max"])
        if regime != "long-many" and plan["plan"] in (2, 3) and not 2 <= plan["n_blocks"] <= 8:
            return "%d blocks" % plan["n_blocks"]
    if regime == "policy":
        want = 2 if run["policy"] == POLICY_FDL else 1
        if plan["plan"] != want or (want == 1 and plan["items"] != plan["rows"] * fco_plan(plan["taps"], plan["out_len"])["n_pairs"]):
            return "plan %d, %d items" % (plan["plan"], plan["items"])
    if regime == "segmented":
        if not cu // 2 <= plan["rows"] < cu:
            return "%d rows on %d CUs" % (plan["rows"], cu)
        if plan["segs"] < 2 or plan["seg_blocks"] < 2 or plan["n_blocks"] % plan["seg_blocks"] == 0:
            return "segs %d, seg_blocks %d, n_blocks %d" % (plan["segs"], plan["seg_blocks"], plan["n_blocks"])
        if plan["items_per_wg_min"] < 2 or plan["blocks"] < plan["segs"]:
            return "%d items on %d workgroups, segs %d" % (plan["items"], plan["blocks"], plan["segs"])
        # some segment behind the first warms up wholly on real samples of its row
        if plan["np"] > 1 and not any(0 <= block_s0(plan, s * plan["seg_blocks"] - (plan["np"] - 1))
                                      and block_s0(plan, s * plan["seg_blocks"] - 1) + FDR_N <= plan["nxa"]
                                      for s in range(1, plan["segs"])):
            return "no segment warms up on real samples"
    if regime in ("long-3", "long-many"):
        if plan["plan"] != 1 or plan["np"] < 5 or plan["swap"] or plan["taps"] <= 32768:
            return "plan %d, n_part %d" % (plan["plan"], plan["np"])
        if regime == "long-3" and plan["rows"] != 3:
            return "%d rows" % plan["rows"]
    return None


# --------------------------------------------------------------------------- #
# 2. the cases                                                                #
# --------------------------------------------------------------------------- #

def _k(plan, np_):
    return {3: "fdr::delay_line_kernel<%d>", 2: "fco::overlap_save_fdl_kernel<%d>"}[plan] % np_


OS_FEW, OS_MANY = "fco::overlap_save_kernel n_part 2..4", "fco::overlap_save_kernel n_part >= 5"
KERNELS_WANTED = {_k(3, n) for n in (1, 2, 3, 4)} | {_k(2, n) for n in (2, 3, 4)} | {OS_FEW, OS_MANY}


def _c(cid, regime, kernel, taps, mode, n=None, layout="shared", policy=0, rows_of_cu=None, rerun=False, parity=0):
    """n: length of the streamed operand (None: sized by the mirror); rows_of_cu: (num, den) for `segmented`; parity: of the
    sized out_len's offset (segmented)."""
    return dict(id=cid, regime=regime, kernel=kernel, taps=taps, mode=mode, n=n, layout=layout, policy=policy, rows_of_cu=rows_of_cu,
                rerun=rerun, parity=parity)


CASES = [
    # many rows on the default policy: both ends of every NP of the real-block delay line
    _c("mr-193-same", "many-rows", _k(3, 1), 193, "same", 33001),
    _c("mr-8192-valid", "many-rows", _k(3, 1), 8192, "valid", 24593, layout="bx1"),
    _c("mr-8193-same", "many-rows", _k(3, 2), 8193, "same", 17001, layout="perrow"),
    _c("mr-12345-full", "many-rows", _k(3, 2), 12345, "full", 20001, layout="bx4"),
    _c("mr-16384-full", "many-rows", _k(3, 2), 16384, "full", 20001, rerun=True),
    _c("mr-16384-valid", "many-rows", _k(3, 2), 16384, "valid", 33001),
    _c("mr-16385-valid", "many-rows", _k(3, 3), 16385, "valid", 25001),
    _c("mr-24576-same", "many-rows", _k(3, 3), 24576, "same", 24577),
    _c("mr-24577-same", "many-rows", _k(3, 4), 24577, "same", 30001),
    _c("mr-32768-full", "many-rows", _k(3, 4), 32768, "full", 32768),
    _c("mr-32768-same", "many-rows", _k(3, 4), 32768, "same", 32769),
    _c("mr-8193-swap", "many-rows", _k(3, 2), 8193, "full", 17001, layout="swap"),
    # few rows cut into segments
    _c("seg-8192", "segmented", _k(3, 1), 8192, "full", rows_of_cu=(25, 32), parity=0),
    _c("seg-8193", "segmented", _k(3, 2), 8193, "full", rows_of_cu=(25, 32), parity=0),
    _c("seg-16385", "segmented", _k(3, 3), 16385, "full", rows_of_cu=(17, 32), parity=0),
    _c("seg-24577", "segmented", _k(3, 4), 24577, "full", rows_of_cu=(17, 32), parity=0),
    # more than 32768 taps: the default route
    _c("lt-32769-valid", "long", OS_MANY, 32769, "valid", 52770, layout="bx1"),
    _c("lt-40000-same", "long", OS_MANY, 40000, "same", 44101, rerun=True),
    _c("lt-49153-full", "long", OS_MANY, 49153, "full", 50001, layout="bx4"),
    # the complex-block plans under policy, on the many-rows shapes
    _c("fdl-8193-same", "policy", _k(2, 2), 8193, "same", 17001, layout="perrow", policy=POLICY_FDL),
    _c("fdl-16385-valid", "policy", _k(2, 3), 16385, "valid", 25001, layout="bx4", policy=POLICY_FDL),
    _c("fdl-24577-same", "policy", _k(2, 4), 24577, "same", 30001, layout="bx1", policy=POLICY_FDL),
    _c("fdl-32768-full", "policy", _k(2, 4), 32768, "full", 32768, policy=POLICY_FDL),
    _c("os-8193-same", "policy", OS_FEW, 8193, "same", 17001, layout="perrow", policy=POLICY_NO_FDL),
    _c("os-16385-valid", "policy", OS_FEW, 16385, "valid", 25001, policy=POLICY_NO_FDL),
    _c("os-24577-same", "policy", OS_FEW, 24577, "same", 30001, layout="bx4", policy=POLICY_NO_FDL),
    _c("os-32768-full", "policy", OS_FEW, 32768, "full", 32768, policy=POLICY_NO_FDL),
    # the threshold between the time-domain kernel and the FFT plans
    _c("direct-192-same", "boundary", "fftconv_direct_kernel", 192, "same", 33001),
]
CASE_IDS = [c["id"] for c in CASES]


def _shapes(case, rows_target, n):
    """The operand shapes of a layout for about `rows_target` output rows: (x shape, y shape, output rows)."""
    taps, lay = case["taps"], case["layout"]
    if lay == "shared":
        return (rows_target, n), (1, taps), rows_target
    if lay == "perrow":
        return (rows_target, n), (rows_target, taps), rows_target
    if lay == "bx1":
        r = _cdiv(rows_target, 4)
        return (r, 1, n), (1, 4, taps), 4 * r
    if lay == "bx4":
        r = _cdiv(rows_target, 4)
        return (r, 4, n), (1, 4, taps), 4 * r
    assert lay == "swap", lay
    return (1, taps), (rows_target, n), rows_target


def sig_row_of(run, row):
    """The row of the streamed operand that output row `row` reads (functional._conv_slice's row maps)."""
    return row // 4 if run["layout"] == "bx1" else row


def tap_row_of(run, row):
    return {"shared": 0, "swap": 0, "perrow": row}.get(run["layout"], row % 4)


def _run(case, regime, rows_target, n, cu, j):
    xs, ys, rows = _shapes(case, rows_target, n)
    run = dict(case=case["id"], regime=regime, kernel=case["kernel"], layout=case["layout"], policy=case["policy"], mode=case["mode"],
               xs=xs, ys=ys, rows=rows, seed=SEED_BASE + 10 * CASE_IDS.index(case["id"]) + j, rerun=case["rerun"])
    plan = run_plan(run, cu)
    run["sig_rows"] = xs[0] * (xs[1] if len(xs) == 3 else 1) if case["layout"] != "swap" else ys[0]
    run["zero_sig_row"], run["zero_placed"] = _place_zero_row(run, plan)
    return run


def run_plan(run, cu):
    return launch_plan(run["rows"], run["xs"][-1], run["ys"][-1], run["mode"], run["policy"], cu)


def _place_zero_row(run, plan):
    """The streamed row to silence: the first whose item (the first of one of its output rows) is the second or third of its
    workgroup's run, directly behind an item of a gain-1 row.  (row, True), or (1, False) where no workgroup runs two items."""
    if plan["plan"] and plan["items_per_wg_max"] >= 2:
        for row in range(plan["rows"]):
            item = row * plan["ipr"]
            z = sig_row_of(run, row)
            prev = sig_row_of(run, (item - plan["blocks"]) // plan["ipr"]) if item >= plan["blocks"] else -1
            if item // plan["blocks"] in (1, 2) and prev >= 0 and prev != z and GAINS[prev % 4] == 1.0:
                return z, True
    return 1, False


def draw_runs(idx, cu=CU_DESIGN):
    """The runs of case `idx` on a device with `cu` CUs -- sized by the mirror, a function of (idx, cu) alone."""
    case = CASES[idx]
    many = int(2.5 * cu) + 3
    if case["regime"] in ("many-rows", "policy", "boundary"):
        for more in range(8):                                     # (a row count rounded up to the layout's 4 may divide evenly)
            run = _run(case, case["regime"], many + more, case["n"], cu, 0)
            if regime_fault(run, run_plan(run, cu)) is None:
                return [run]
        raise AssertionError((case["id"], regime_fault(run, run_plan(run, cu)), cu))
    if case["regime"] == "long":
        n_pairs = fco_plan(case["taps"], conv_slice(case["n"], case["taps"], case["mode"])[1])["n_pairs"]
        few = dict(case, layout="shared", rerun=False)
        for more in range(8):
            run = _run(case, "long-many", _cdiv(many, n_pairs) + more, case["n"], cu, 1)
            if regime_fault(run, run_plan(run, cu)) is None:
                return [_run(few, "long-3", 3, case["n"], cu, 0), run]
        raise AssertionError((case["id"], regime_fault(run, run_plan(run, cu)), cu))
    assert case["regime"] == "segmented" and case["mode"] == "full"
    rows = cu * case["rows_of_cu"][0] // case["rows_of_cu"][1]
    probe = launch_plan(rows, 10 ** 6, case["taps"], "full", 0, cu)
    for nb in range(3, 64):                                   # the shortest out_len of nb blocks (+ 9 or 10 samples), nx >= taps
        n = (nb - 1) * probe["hop"] + 9 + case["parity"] - case["taps"] + 1
        if n < case["taps"]:
            continue
        run = _run(case, "segmented", rows, n, cu, 0)
        if regime_fault(run, run_plan(run, cu)) is None:
            return [run]
    raise AssertionError((case["id"], "no segmented shape", cu))


# --------------------------------------------------------------------------- #
# 3. the reference and the checks (torch, on whatever device the tensors are) #
# --------------------------------------------------------------------------- #

SLAB_BYTES = 256 << 20


def reference64(sig, taps, start, out_len):
    """(r, n) x (r or 1, m) float32 or float64 -> (r, out_len) float64: rows of the full linear convolution from `start`, by
    rfft / irfft in float64 at the next power of two >= n + m - 1."""
    n_full = sig.shape[-1] + taps.shape[-1] - 1
    n = 1 << (n_full - 1).bit_length()
    full = torch.fft.irfft(torch.fft.rfft(sig.double(), n=n) * torch.fft.rfft(taps.double(), n=n), n=n)
    return full[:, start:start + out_len]


def slab_rows(n_full):
    n = 1 << (n_full - 1).bit_length()
    return max(1, SLAB_BYTES // ((n // 2 + 1) * 16))


def row_errors(got, ref):
    """(r, n) x 2 -> per row max|got - ref| / max|ref of that row| (the absolute error where the row's reference is all zero),
    and the index of each row's worst element."""
    d = (got.double() - ref).abs()
    e, where = d.max(1)
    peak = ref.abs().amax(1)
    return torch.where(peak > 0, e / peak.clamp_min(1e-300), e), where


def whole_tensor_error(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max())


def check_outputs(got, ref_of, zero_rows, plan, run, step=None, bar=BAR):
    """Every output of every row of `got` (rows, out_len) against ref_of(ra, rb) -> float64 (rb - ra, out_len), slab by slab:
    the rows of `zero_rows` exactly 0.0, every row within `bar` of its own reference peak.  Returns the worst err / bar."""
    rows = got.shape[0]
    step = step or rows
    rel, where = [], []
    for ra in range(0, rows, step):
        ref = ref_of(ra, min(rows, ra + step))
        e, w = row_errors(got[ra:ra + step], ref)
        rel.append(e)
        where.append(w)
    rel, where = torch.cat(rel), torch.cat(where)
    assert bool(torch.isfinite(got).all()), (run["case"], run["regime"], "non-finite output")
    for z in zero_rows:
        assert float(got[z].abs().max()) == 0.0, (run["case"], run["regime"], "the all-zero row", float(got[z].abs().max()),
                                                  locate(plan, z, int(got[z].abs().argmax()), sig_row_of(run, z)), plan)
    r = int(rel.argmax())
    err = float(rel[r])
    loc = locate(plan, r, int(where[r]), sig_row_of(run, r))
    _note(plan, run, err, bar, loc)
    assert err <= bar, (run["case"], run["regime"], "per-row", err, bar, err / bar, loc, plan)
    return err / bar


_WORST = {}


def _note(plan, run, err, bar, where):
    kernel, ratio = plan["kernel"], err / bar
    if ratio >= _WORST.get(kernel, (-1.0,))[0]:
        _WORST[kernel] = (ratio, run["case"], run["regime"])
    print(f"[fuzz-fftconv] {kernel} NP={plan['np']} {run['case']} {run['regime']} {run['layout']} x={run['xs']} y={run['ys']} "
          f"{run['mode']}: err={err:.3e} bar={bar:.1e} err/bar={ratio:.4f} (worst of this kernel so far {_WORST[kernel][0]:.4f} "
          f"{_WORST[kernel][1:]}) at {where}")


# --------------------------------------------------------------------------- #
# 4. the device tests                                                         #
# --------------------------------------------------------------------------- #

def device_cu():
    """The CU count as csrc/api_common.hip reads it (multiProcessorCount), checked against aamd_device_info."""
    from audio_amd import _lib
    cu = int(torch.cuda.get_device_properties(0).multi_processor_count)
    name, cus, mem = C.create_string_buffer(128), C.c_int32(0), C.c_int64(0)
    _lib.check(_lib.lib().aamd_device_info(name, 128, C.byref(cus), C.byref(mem)))
    assert cus.value == cu and cu >= 8, (cus.value, cu)
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


def make_operands(run, dev):
    """(x, y, sig (sig_rows, n), taps (tap_rows, m)): standard normal rows times GAINS[row % 4] with the run's zero row, taps
    0.2 * randn; x and y are the views F.fftconvolve gets, sig / taps the same memory as 2-D row tables."""
    gen = torch.Generator(device=dev).manual_seed(run["seed"])
    swap = run["layout"] == "swap"
    sshape, tshape = (run["ys"], run["xs"]) if swap else (run["xs"], run["ys"])
    sig = torch.randn(run["sig_rows"], sshape[-1], generator=gen, device=dev, dtype=torch.float32)
    sig.mul_(torch.tensor([GAINS[r % 4] for r in range(run["sig_rows"])], device=dev, dtype=torch.float32)[:, None])
    sig[run["zero_sig_row"]] = 0.0
    tap_rows = int(np.prod(tshape[:-1]))
    taps = torch.randn(tap_rows, tshape[-1], generator=gen, device=dev, dtype=torch.float32).mul_(0.2)
    xv, yv = (taps.view(tshape), sig.view(sshape)) if swap else (sig.view(sshape), taps.view(tshape))
    return xv, yv, sig, taps


def run_product(run, x, y):
    import audio_amd.functional as F
    from audio_amd import _lib
    with torch.no_grad():
        if run["policy"]:
            with _lib.kernel_policy(run["policy"]):
                return F.fftconvolve(x, y, run["mode"])
        return F.fftconvolve(x, y, run["mode"])


def check_run(run, cu, dev):
    """One run: the regime asserted on the mirror with the device's CU count, the plan number against the library's, the product
    against float64.  Returns the plan."""
    import audio_amd.functional as F
    from audio_amd import _lib
    plan = run_plan(run, cu)
    fault = regime_fault(run, plan)
    assert fault is None, (run, fault, f"{cu} CUs", plan)
    assert run["zero_placed"] == (plan["plan"] != 0 and plan["items_per_wg_max"] >= 2), (run, plan)
    nx, ny = run["xs"][-1], run["ys"][-1]
    if run["policy"]:
        with _lib.kernel_policy(run["policy"]):
            lib_plan = _lib.lib().aamd_fftconvolve_plan(run["rows"], nx, ny, plan["out_len"])
    else:
        lib_plan = _lib.lib().aamd_fftconvolve_plan(run["rows"], nx, ny, plan["out_len"])
    assert lib_plan == plan["plan"], (run, lib_plan, plan)
    x, y, sig, taps = make_operands(run, dev)
    assert x.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0
    got = run_product(run, x, y)
    assert got.shape[-1] == plan["out_len"] and got.numel() == run["rows"] * plan["out_len"], (got.shape, plan)
    assert got.is_contiguous() and got.data_ptr() % 16 == 0
    got = got.view(run["rows"], plan["out_len"])
    if run["rerun"]:
        # the second call with one tap tensor prepares a workspace that stays with it, the third runs RUN-only against it
        assert F.fftconvolve_held_taps(y) == 0
        second = run_product(run, x, y)
        assert F.fftconvolve_held_taps(y) == 1, (run, plan)
        third = run_product(run, x, y)
        assert torch.equal(second.view_as(got), got) and torch.equal(third.view_as(got), got), (run, "RUN-only call differs")
    rows = torch.arange(run["rows"], device=dev)
    smap = rows // 4 if run["layout"] == "bx1" else rows
    tmap = {"shared": None, "swap": None, "perrow": rows}.get(run["layout"], rows % 4)

    def ref_of(ra, rb):
        return reference64(sig[smap[ra:rb]], taps[:1] if tmap is None else taps[tmap[ra:rb]], plan["start"], plan["out_len"])

    zero_rows = [r for r in range(run["rows"]) if sig_row_of(run, r) == run["zero_sig_row"]]
    assert zero_rows and float(ref_of(zero_rows[0], zero_rows[0] + 1).abs().max()) == 0.0
    check_outputs(got, ref_of, zero_rows, plan, run, step=slab_rows(nx + ny - 1))
    return plan


@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(len(CASES)), ids=CASE_IDS)
def test_fuzz_fftconv_kernels_in_multi_item_runs_vs_float64(idx, dev, cu):
    for run in draw_runs(idx, cu):
        check_run(run, cu, dev)


# --------------------------------------------------------------------------- #
# 5. no device: the mirror against the headers' plans, coverage, bite         #
# --------------------------------------------------------------------------- #

def _against_headers(rows, taps, out_len, cu):
    import sim_util as S
    ok, g = S.sim_fdr_plan(rows, taps, out_len, cu)
    mine = fdr_plan(rows, taps, out_len, cu)
    assert ok == (mine is not None), (rows, taps, out_len, cu)
    if ok:
        assert g == mine, (rows, taps, out_len, cu, g, mine)
    cheaper, g1, f = S.sim_fco_plan(rows, taps, out_len, cu)
    assert g1 == fco_plan(taps, out_len), (rows, taps, out_len, cu)
    mc, mf = fco_plan_fdl(rows, taps, out_len, cu)
    assert (cheaper, f) == (mc, mf), (rows, taps, out_len, cu, cheaper, f, mc, mf)


def test_mirror_equals_the_headers_plans():
    """fdr_plan / fco_plan / fco_plan_fdl against fdr::plan / fco::plan / fco::plan_fdl themselves for the shapes of every run of every
    case at 256 CUs, at 8 and at 5, and over a sweep of shapes on both sides of every threshold."""
    n = 0
    for idx in range(len(CASES)):
        for run in draw_runs(idx):
            for cu in (CU_DESIGN, 8, 5):
                plan = run_plan(run, cu)
                assert cu != CU_DESIGN or regime_fault(run, plan) is None, (run, cu)
                _against_headers(plan["rows"], plan["taps"], plan["out_len"], cu)
                n += 1
    r = np.random.default_rng(SEED_BASE)
    for taps in (2, 193, 8191, 8192, 8193, 12345, 16384, 16385, 24576, 24577, 32768, 32769, 40000, 49153, 65537):
        for _ in range(12):
            rows, cu = int(r.choice([1, 3, 5, 200, 260, 643, 5000])), int(r.choice([1, 2, 8, 104, 256, 304]))
            _against_headers(rows, taps, int(r.integers(1, 400000)), cu)
            n += 1
    assert n > 200


def test_launch_plan_by_hand():
    """The mirror on numbers worked out by hand from csrc/api_fftconv.hip at 256 CUs."""
    p = launch_plan(643, 17001, 8193, "same")
    assert (p["plan"], p["np"], p["hop"], p["skip"], p["n_blocks"], p["segs"], p["seg_blocks"]) == (3, 2, 8192, 8192, 3, 1, 3)
    assert (p["start"], p["out_len"], p["items"], p["blocks"], p["items_per_wg_min"], p["items_per_wg_max"]) == (4096, 17001, 643, 256, 2, 3)
    w = locate(p, 259, 9000)
    assert (w["item"], w["workgroup"], w["position"], w["run_length"], w["block"], w["first_block"], w["last_block"]) == (259, 3, 1, 3, 1, False, False)
    assert w["warm_up_neighbour"] is False and locate(p, 259, 5)["warm_up_neighbour"] and not w["vin"] and not w["vout"] and not w["s0_odd"]
    p = launch_plan(643, 33001, 193, "same")                        # NP 1: three one-block segments a row, 8 items a workgroup
    assert (p["np"], p["hop"], p["skip"], p["segs"], p["seg_blocks"], p["items"], p["items_per_wg_max"]) == (1, 16192, 192, 3, 1, 1929, 8)
    p = launch_plan(200, 60010, 8192, "full")                       # the issue's segmented example
    assert (p["np"], p["segs"], p["seg_blocks"], p["n_blocks"], p["items"]) == (1, 5, 2, 9, 1000)
    p = launch_plan(256, 480000, 24000, "full")                     # BASELINE config 5b: one item a workgroup
    assert (p["plan"], p["np"], p["segs"], p["items"], p["items_per_wg_max"]) == (3, 3, 1, 256, 1)
    p = launch_plan(3, 50001, 49153, "full")
    assert (p["plan"], p["np"], p["part_taps"], p["hop"], p["n_blocks"], p["ipr"], p["kernel"]) == (1, 7, 7022, 9363, 11, 6, OS_MANY)
    assert launch_plan(3, 50001, 32769, "full")["plan"] == 1 and launch_plan(3, 50001, 32768, "full")["plan"] == 3
    assert launch_plan(3, 50001, 192, "full")["plan"] == 0 and launch_plan(3, 50001, 193, "full")["plan"] == 3
    assert launch_plan(3, 193, 50001, "full")["swap"] and launch_plan(3, 193, 50001, "full")["taps"] == 193
    p = launch_plan(643, 30001, 24577, "same", POLICY_FDL)
    assert (p["plan"], p["np"], p["segs"], p["n_blocks"], p["items"]) == (2, 4, 1, 4, 643)
    w = locate(p, 300, 8192 * 3 + 1)
    assert (w["step"], w["half"], w["position"], w["workgroup"]) == (1, 1, 1, 44)
    p = launch_plan(643, 30001, 24577, "same", POLICY_NO_FDL)
    assert (p["plan"], p["np"], p["kernel"]) == (1, 4, OS_FEW)
    assert launch_plan(643, 30001, 24577, "same", POLICY_GENERIC)["plan"] == 0


def test_cases_cover_the_gaps():
    """What the cases pin, from the mirror at 256 CUs; a change of a case or of the sizing cannot silently lose one."""
    assert len(set(CASE_IDS)) == len(CASES)
    every = [(CASES[idx], run, run_plan(run, CU_DESIGN)) for idx in range(len(CASES)) for run in draw_runs(idx)]
    for c, r, p in every:
        assert regime_fault(r, p) is None, (r, p)
        # sizes: inputs and outputs of at most 170 MB, workspaces (tap spectra + delay-line rings) of at most 200 MB
        tap_rows = int(np.prod((r["xs"] if p["swap"] else r["ys"])[:-1]))
        np_fdl = _cdiv(p["taps"], FCO_HOP) if p["taps"] <= 32768 and p["taps"] > 8192 and not p["policy"] & POLICY_NO_FDL else 0
        ws = 8 * FCO_N * (1 + tap_rows * max(np_fdl, fco_plan(p["taps"], p["out_len"])["n_part"]) + max(0, np_fdl - 2) * CU_DESIGN)
        assert r["sig_rows"] * p["nxa"] * 4 <= 170e6 and p["rows"] * p["out_len"] * 4 <= 170e6 and ws <= 200e6, (r, ws)
    # gap: the nine launch targets, each with >= 3 items on some workgroup; n_part >= 5 with rows * n_pairs > blocks
    assert {p["kernel"] for _, _, p in every} == KERNELS_WANTED | {"fftconv_direct_kernel"} and len(KERNELS_WANTED) == 9
    assert {p["kernel"] for _, _, p in every if p["items_per_wg_max"] >= 3 and p["items_per_wg_min"] >= 2} == KERNELS_WANTED
    assert any(p["kernel"] == OS_MANY and p["rows"] * p["ipr"] > p["blocks"] for _, _, p in every)
    # gap: both ends of every partition count, a partial last partition, the threshold of the time-domain kernel
    fdr_cases = [(c, r, p) for c, r, p in every if p["plan"] == 3]
    assert {p["taps"] for _, _, p in fdr_cases} >= {193, 8192, 8193, 12345, 16384, 16385, 24576, 24577, 32768}
    assert {(p["taps"], p["np"]) for _, _, p in fdr_cases} >= {(193, 1), (8192, 1), (8193, 2), (16384, 2), (16385, 3), (24576, 3),
                                                                 (24577, 4), (32768, 4)}
    assert {(p["taps"], p["plan"]) for _, _, p in every} >= {(192, 0), (193, 3)}
    # gap: more than 32768 taps on the default policy -- n_part 5, 5, 7; the three modes; 3 rows and many; nx >= ny
    longs = [(c, r, p) for c, r, p in every if c["regime"] == "long"]
    assert {(p["taps"], p["np"], p["mode"]) for _, _, p in longs} == {(32769, 5, "valid"), (40000, 5, "same"), (49153, 7, "full")}
    assert all(p["policy"] == 0 and p["plan"] == 1 and not p["swap"] for _, _, p in longs)
    assert {(c["id"], r["regime"]) for c, r, _ in longs} == {(c["id"], g) for c in CASES if c["regime"] == "long" for g in ("long-3", "long-many")}
    assert all(p["start"] >= 32768 and p["out_len"] < p["taps"] for _, _, p in longs if p["mode"] == "valid")      # short slice, deep start
    # gap: many-rows -- 643 rows, every workgroup >= 2 items, some 3 or more, 2 .. 8 blocks; NP 1: segs 3, 8 items a workgroup
    for c, r, p in every:
        if c["regime"] in ("many-rows", "policy"):
            assert p["rows"] in (643, 644) and p["items"] % p["blocks"] and p["items_per_wg_min"] >= 2 and p["items_per_wg_max"] >= 3, r
            if p["plan"] in (2, 3):
                assert 2 <= p["n_blocks"] <= 8 and (p["segs"] == 1 or p["np"] == 1), (r, p)
    assert {(p["taps"], p["segs"], p["seg_blocks"], p["items_per_wg_max"]) for _, _, p in fdr_cases if p["np"] == 1 and p["rows"] >= 643} == \
        {(193, 3, 1, 8), (8192, 3, 1, 8)}
    assert {p["n_blocks"] for c, _, p in fdr_cases if c["regime"] == "many-rows"} >= {2, 3, 4, 5, 8}
    # gap: segmented -- every NP; rows in [CU / 2, CU); a shorter last segment; a later segment warms up on real samples
    segd = [(c, r, p) for c, r, p in every if c["regime"] == "segmented"]
    assert {p["np"] for _, _, p in segd} == {1, 2, 3, 4}
    for c, r, p in segd:
        assert 128 <= p["rows"] < 256 and p["segs"] >= 2 and p["seg_blocks"] >= 2 and p["n_blocks"] % p["seg_blocks"], (r, p)
        assert p["items_per_wg_min"] >= 2 and p["blocks"] == 256 >= p["segs"], (r, p)
        last = locate(p, 0, p["out_len"] - 1)
        assert last["last_block"] and last["block_in_segment"] < p["seg_blocks"] - 1 and last["segment"] == p["segs"] - 1
        for item in range(0, p["items"] - p["blocks"]):                 # consecutive items of a workgroup: different rows
            assert item // p["ipr"] != (item + p["blocks"]) // p["ipr"]
    # gap: the policy plans on the many-rows shapes -- plan 2 for NP 2, 3, 4 and plan 1 with 2, 3, 4 partitions, items = rows * n_pairs
    pol = [(c, r, p) for c, r, p in every if c["regime"] == "policy"]
    assert {(p["plan"], p["np"]) for _, _, p in pol} == {(2, 2), (2, 3), (2, 4), (1, 2), (1, 3), (1, 4)}
    assert all(p["items"] == p["rows"] * fco_plan(p["taps"], p["out_len"])["n_pairs"] for _, _, p in pol if p["plan"] == 1)
    assert all(p["items_per_wg_max"] >= 3 for _, _, p in pol)
    shapes = {(r["xs"][-1], p["taps"], p["mode"]) for c, r, p in every if c["regime"] == "many-rows"}
    assert all((r["xs"][-1], p["taps"], p["mode"]) in shapes for _, r, p in pol)
    # gap: layouts -- per-row taps once per kernel family with NP <= 2; both broadcast maps; the swap once; two RUN-only reruns
    per = {(p["plan"], p["np"]) for _, r, p in every if r["layout"] == "perrow"}
    assert per == {(3, 2), (2, 2), (1, 2)}
    assert all(r["ys"][0] == p["rows"] for _, r, p in every if r["layout"] == "perrow")
    for lay, xlead, ylead in (("bx1", 1, 4), ("bx4", 4, 4)):
        mine = [(r, p) for _, r, p in every if r["layout"] == lay]
        assert {p["plan"] for _, p in mine} == {1, 2, 3} and all(r["xs"][1] == xlead and r["ys"][:2] == (1, ylead) for r, _ in mine), lay
    assert any(p["kernel"] == OS_MANY for _, r, p in every if r["layout"] == "bx4")      # a few tap rows beyond 32768 taps too
    swaps = [(r, p) for _, r, p in every if r["layout"] == "swap"]
    assert len(swaps) == 1 and swaps[0][1]["swap"] and swaps[0][0]["xs"][-1] < swaps[0][0]["ys"][-1] and swaps[0][1]["rows"] == 643
    assert all(not p["swap"] for _, r, p in every if r["layout"] != "swap")
    reruns = [(r, p) for _, r, p in every if r["rerun"]]
    assert {p["kernel"] for _, p in reruns} == {_k(3, 2), OS_MANY} and len(reruns) == 2
    assert all(not p["swap"] and r["layout"] == "shared" and p["items_per_wg_max"] >= 3 for r, p in reruns)
    # gap: alignment -- odd nx and odd out_len (vin / vout flip from item to item of a workgroup), an odd block start
    for np_ in (1, 2, 3, 4):
        mine = [(r, p) for _, r, p in fdr_cases if p["np"] == np_]
        assert any(p["nxa"] % 2 == 1 and p["out_len"] % 2 == 1 for _, p in mine), np_
        flips = False
        for r, p in mine:
            for item in range(p["blocks"], p["items"]):           # an item and the one before it on the same workgroup
                a, b = locate(p, item // p["ipr"], 0, sig_row_of(r, item // p["ipr"])), None
                prev_row = (item - p["blocks"]) // p["ipr"]
                b = locate(p, prev_row, 0, sig_row_of(r, prev_row))
                flips = flips or (a["vin"] != b["vin"] and a["vout"] != b["vout"])
        assert flips, np_
        assert any(locate(p, 0, 0)["s0_odd"] for _, p in mine), np_
    # gap: the all-zero row is the second or third item of a workgroup, behind a gain-1 row -- wherever a workgroup runs two items
    for c, r, p in every:
        assert r["zero_placed"] == (p["plan"] != 0 and r["regime"] != "long-3"), r
        if r["zero_placed"]:
            rows = [row for row in range(p["rows"]) if sig_row_of(r, row) == r["zero_sig_row"]]
            ok = False
            for row in rows:
                w = locate(p, row, 0)
                prev = sig_row_of(r, (w["item"] - p["blocks"]) // p["ipr"])
                ok = ok or (w["position"] in (1, 2) and GAINS[prev % 4] == 1.0 and prev != r["zero_sig_row"])
            assert ok, r
    print("[fuzz-fftconv] gaps pinned: 9 kernels with >= 3 items on a workgroup; many-rows / segmented / long-taps / policy / boundary; "
          "taps 192 .. 49153; shared / per-row / broadcast / swapped operands; RUN-only reruns; odd nx, out_len, start; the zero row")


def test_reference_forms_agree():
    """reference64 (power-of-two rfft, torch) against oracle.dsp_oracle.fftconvolve (numpy, n = nx + ny - 1) on small arrays."""
    from oracle import dsp_oracle as O
    g = torch.Generator().manual_seed(SEED_BASE)
    for nx, ny, mode in ((1000, 193, "same"), (777, 300, "valid"), (513, 512, "full"), (300, 777, "full"), (2049, 1025, "same")):
        x, y = torch.randn(3, nx, generator=g), 0.2 * torch.randn(3, ny, generator=g)
        x[1] *= 1e-3
        want = O.fftconvolve(x.numpy().astype(np.float64), y.numpy().astype(np.float64), mode)
        start, out_len = conv_slice(nx, ny, mode)
        sig, taps = (y, x) if ny > nx else (x, y)
        have = reference64(sig, taps, start, out_len).numpy()
        assert have.shape == want.shape
        for r in range(3):
            assert np.abs(have[r] - want[r]).max() <= 1e-12 * np.abs(want[r]).max(), (nx, ny, mode, r)
        shared = reference64(sig, taps[:1], start, out_len).numpy()          # one tap row against every row
        x1, y1 = (x[:1], y) if ny > nx else (x, y[:1])
        want1 = O.fftconvolve(x1.numpy().astype(np.float64), y1.numpy().astype(np.float64), mode)
        assert np.abs(shared - want1).max() <= 1e-12 * np.abs(want1).max(), (nx, ny, mode)
    assert slab_rows(17001 + 8193 - 1) * (32768 // 2 + 1) * 16 <= SLAB_BYTES < (slab_rows(17001 + 8193 - 1) + 1) * (32768 // 2 + 1) * 16


# ---- bite: small arrays, float64 block-wise overlap-save models -------------------------------------------------------------------

# err / bar of the worst row (and, where it says so, the absolute peak of the all-zero row), measured on the CPU with the shapes below
BITE_MEASURED = {"float32-rounded honest model": 0.0025,
                 "stale delay line NP 2: zero row peak / 1e-3 row / worst row": (1.15, 9.5e4, 1.62e6),
                 "stale delay line NP 3: zero row peak / 1e-3 row / worst row": (3.86, 2.64e5, 3.18e6),
                 "stale delay line NP 4: zero row peak / 1e-3 row / worst row": (4.32, 2.96e5, 1.91e6),
                 "delay slots 2 and 3 exchanged, NP 4: worst row / best non-zero row": (4.01e4, 2.75e4),
                 "prefetch from the previous item's row, n_part 5: zero row peak / worst row / whole-tensor": (0.0232, 2.24e7, 2.07e4),
                 "50 bars in the 1e-3 row: per-row / whole-tensor": (50.0, 0.05)}
BITE_B, BITE_CU, BITE_ROWS = 64, 3, 9          # blocks of 2 x 64 samples; rows 0, 3, 6 / 1, 4, 7 / 2, 5, 8 on three workgroups
BITE_ZERO = 7                                    # third item of workgroup 1, behind row 4 (gain 1)


def _segment(x, s0, n):
    out = np.zeros(n)
    lo, hi = max(s0, 0), min(s0 + n, x.shape[0])
    if hi > lo:
        out[lo - s0:hi - s0] = x[lo:hi]
    return out


def delay_line_model(sig, taps, start, out_len, cu, fault=None, B=BITE_B):
    """The delay-line plans in float64: blocks of 2 B samples at hop B, NP = ceil(ny / B) partitions of B taps,
    Y_j = sum_p H_p Z_(j - p); one item per row, workgroup w runs rows w, w + cu, ...  fault "stale": an item behind the first of
    its workgroup skips its NP - 1 forward-only steps and starts from the delayed spectra the previous item left; "slot": Z_(j-2)
    and Z_(j-3) change places in the sum."""
    rows, ny = sig.shape[0], taps.shape[0]
    NP, N = _cdiv(ny, B), 2 * B
    H = [np.fft.fft(_segment(taps, p * B, B), n=N) for p in range(NP)]
    n_blocks = _cdiv(out_len, B)
    out = np.zeros((rows, n_blocks * B))
    for w in range(min(cu, rows)):
        z = None
        for pos, row in enumerate(range(w, rows, cu)):
            if not (fault == "stale" and pos >= 1):
                z = [np.zeros(N, dtype=complex) for _ in range(NP - 1)]
                for j in range(-(NP - 1), 0):
                    z = ([np.fft.fft(_segment(sig[row], start + j * B - B, N))] + z)[:NP - 1]
            for j in range(n_blocks):
                zs = [np.fft.fft(_segment(sig[row], start + j * B - B, N))] + z
                if fault == "slot":
                    zs[2], zs[3] = zs[3], zs[2]
                out[row, j * B:(j + 1) * B] = np.fft.ifft(sum(H[p] * zs[p] for p in range(NP))).real[B:]
                z = zs[:NP - 1]
    return out[:, :out_len]


def recompute_model(sig, taps, start, out_len, cu, n_part, fault=None, B=BITE_B):
    """Plan 1 in float64: blocks of N = 2 B samples, n_part partitions of pt taps, v = N - pt + 1 outputs a block,
    Y = sum_p H_p FFT(x[s0 - p pt ..)); an item is a (row, block), workgroup w runs the items w, w + cu, ...  fault "prefetch": the
    partition-0 inputs of an item behind the first of its workgroup come from the PREVIOUS item's row (the fetch issued during
    that item's stores took its row)."""
    rows, ny = sig.shape[0], taps.shape[0]
    N = 2 * B
    pt = _cdiv(ny, n_part)
    v = N - pt + 1
    H = [np.fft.fft(_segment(taps, p * pt, pt), n=N) for p in range(n_part)]
    n_blocks = _cdiv(out_len, v)
    out = np.zeros((rows, n_blocks * v))
    for item in range(rows * n_blocks):
        row, j = divmod(item, n_blocks)
        Y = 0
        for p in range(n_part):
            src = (item - cu) // n_blocks if (fault == "prefetch" and p == 0 and item >= cu) else row
            Y = Y + H[p] * np.fft.fft(_segment(sig[src], start - p * pt + j * v - (pt - 1), N))
        out[row, j * v:(j + 1) * v] = np.fft.ifft(Y).real[pt - 1:]
    return out[:, :out_len]


def _bite_inputs(ny, nx=700):
    g = torch.Generator().manual_seed(SEED_BASE + ny)
    sig = torch.randn(BITE_ROWS, nx, generator=g) * torch.tensor([GAINS[r % 4] for r in range(BITE_ROWS)])[:, None]
    sig[BITE_ZERO] = 0.0
    taps = 0.2 * torch.randn(1, ny, generator=g)
    assert GAINS[(BITE_ZERO - BITE_CU) % 4] == 1.0 and BITE_ZERO // BITE_CU == 2
    start, out_len = conv_slice(nx, ny, "same")
    return sig, taps, start, out_len, reference64(sig, taps, start, out_len)


def _bite_plan(ny, out_len, n_blocks, np_, hop):
    """A stand-in for the mirror's plan on the models' small blocks: one item per row (or per block), BITE_CU workgroups."""
    return dict(plan=9, kernel="model", hop=hop, seg_blocks=n_blocks, n_blocks=n_blocks, ipr=1, blocks=BITE_CU, items=BITE_ROWS,
                np=np_, out_len=out_len)


_BITE_RUN = dict(case="bite", regime="bite", layout="shared", xs=(BITE_ROWS, 700), ys=(1, 0), mode="same")


@pytest.mark.parametrize("np_", [2, 3, 4])
def test_bite_second_item_starts_from_the_previous_items_spectra(np_):
    """The honest model passes the checks the device runs use; with the stale delay line the all-zero row is not zero, the 1e-3
    row (second item of workgroup 2, behind the 1e-2 row) misses the bar by far, and check_outputs raises."""
    ny = BITE_B * (np_ - 1) + 17                                     # a partial last partition
    sig, taps, start, out_len, ref = _bite_inputs(ny)
    plan = _bite_plan(ny, out_len, _cdiv(out_len, BITE_B), np_, BITE_B)
    honest = torch.from_numpy(delay_line_model(sig.double().numpy(), taps[0].double().numpy(), start, out_len, BITE_CU))
    assert float(row_errors(honest, ref)[0].max()) <= 1e-12 and float(honest[BITE_ZERO].abs().max()) == 0.0
    check_outputs(honest.float(), lambda a, b: ref[a:b], [BITE_ZERO], plan, _BITE_RUN)
    bad = torch.from_numpy(delay_line_model(sig.double().numpy(), taps[0].double().numpy(), start, out_len, BITE_CU, "stale")).float()
    rel = row_errors(bad, ref)[0]
    zero_peak, quiet = float(bad[BITE_ZERO].abs().max()), float(rel[5]) / BAR
    print(f"[fuzz-fftconv] bite stale delay line NP {np_}: zero row peak {zero_peak:.3g}, 1e-3 row err/bar {quiet:.3g}, worst row "
          f"{float(rel.max()) / BAR:.3g}; rows at fault {[r for r in range(BITE_ROWS) if float(rel[r]) > BAR]}")
    assert zero_peak > 1e-3 and quiet >= 100.0 and GAINS[5 % 4] == 1e-3
    assert all(float(rel[r]) <= 1e-6 for r in range(BITE_CU))         # the first item of every workgroup is untouched
    with pytest.raises(AssertionError, match="all-zero row"):
        check_outputs(bad, lambda a, b: ref[a:b], [BITE_ZERO], plan, _BITE_RUN)
    with pytest.raises(AssertionError, match="per-row"):
        check_outputs(bad, lambda a, b: ref[a:b], [], plan, _BITE_RUN)


def test_bite_delay_slot_read_out_of_order():
    ny = BITE_B * 3 + 17
    sig, taps, start, out_len, ref = _bite_inputs(ny)
    plan = _bite_plan(ny, out_len, _cdiv(out_len, BITE_B), 4, BITE_B)
    bad = torch.from_numpy(delay_line_model(sig.double().numpy(), taps[0].double().numpy(), start, out_len, BITE_CU, "slot")).float()
    rel = row_errors(bad, ref)[0]
    print(f"[fuzz-fftconv] bite delay slots 2 and 3 exchanged, NP 4: worst row err/bar {float(rel.max()) / BAR:.3g}, "
          f"best non-zero row {min(float(rel[r]) for r in range(BITE_ROWS) if r != BITE_ZERO) / BAR:.3g}")
    assert min(float(rel[r]) for r in range(BITE_ROWS) if r != BITE_ZERO) >= 100.0 * BAR
    with pytest.raises(AssertionError, match="per-row"):
        check_outputs(bad, lambda a, b: ref[a:b], [BITE_ZERO], plan, _BITE_RUN)


def test_bite_next_item_prefetch_from_the_wrong_row():
    ny, n_part = 5 * 23, 5
    sig, taps, start, out_len, ref = _bite_inputs(ny)
    v = 2 * BITE_B - 23 + 1
    plan = _bite_plan(ny, out_len, _cdiv(out_len, v), n_part, v)
    plan.update(seg_blocks=1, ipr=_cdiv(out_len, v), items=BITE_ROWS * _cdiv(out_len, v))
    honest = torch.from_numpy(recompute_model(sig.double().numpy(), taps[0].double().numpy(), start, out_len, BITE_CU, n_part))
    assert float(row_errors(honest, ref)[0].max()) <= 1e-12 and float(honest[BITE_ZERO].abs().max()) == 0.0
    check_outputs(honest.float(), lambda a, b: ref[a:b], [BITE_ZERO], plan, _BITE_RUN)
    bad = torch.from_numpy(recompute_model(sig.double().numpy(), taps[0].double().numpy(), start, out_len, BITE_CU, n_part, "prefetch")).float()
    rel = row_errors(bad, ref)[0]
    zero_peak = float(bad[BITE_ZERO].abs().max())
    print(f"[fuzz-fftconv] bite prefetch from the previous item's row, n_part {n_part}: zero row peak {zero_peak:.3g}, worst row err/bar "
          f"{float(rel.max()) / BAR:.3g}, whole-tensor err/bar {whole_tensor_error(bad, ref) / BAR:.3g}")
    assert float(rel.max()) >= 100.0 * BAR
    with pytest.raises(AssertionError):
        check_outputs(bad, lambda a, b: ref[a:b], [BITE_ZERO], plan, _BITE_RUN)


def test_bite_whole_tensor_metric_loses_the_rows_gain():
    """Why the bar is applied per row: a fault confined to the 1e-3 row, 50 x ITS bar, is 0.05 x the bar of a whole-tensor peak."""
    sig, taps, start, out_len, ref = _bite_inputs(BITE_B + 17)
    got = ref.float().clone()
    got[5, 100:164] += 50 * BAR * float(ref[5].abs().max())
    per_row, whole = float(row_errors(got, ref)[0].max()) / BAR, whole_tensor_error(got, ref) / BAR
    gain = float(ref[5].abs().max() / ref.abs().max())
    print(f"[fuzz-fftconv] bite fault of 50 bars in the 1e-3 row: per-row err/bar {per_row:.3g}, whole-tensor err/bar {whole:.3g}")
    assert 49.0 <= per_row <= 51.0 and whole < 1.0 and gain < 2e-3
