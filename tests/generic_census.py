"""The census of the generic mixed-radix kernels (csrc/stft_generic.h stft_generic_kernel, csrc/istft.h ola_kernel,
csrc/kaldi_generic.h kaldi_generic_kernel): which n_fft run, with which radix plan, pairs per block and LDS layout, and the
cases, inputs, float64 references and per-row judges built on it.  Shared by the device-free layer
(tests/test_generic_census.py: the CPU replay of the same phase functions) and the device layer
(tests/test_gpu_fuzz_generic.py: the public API on an MI355X).  torch on the CPU only; nothing here touches a device.

The host mirror restates the launchers' arithmetic (api_stft.hip launch_generic, api_istft.hip, api_f64.hip, api_kaldi.hip)
on top of plan_radices / gen_pairs_per_block / gen_lds_floats(_long) / kgen::pairs_per_block / kgen::lds_floats(_long);
tests/test_generic_census.py holds it against those functions themselves.  Every boundary size is computed by the mirror
from the 160 KB LDS opt-in of the device, none is a literal.
"""
import functools
import math

import numpy as np
import torch

LDS_OPTIN = 160 * 1024          # bytes: hipDeviceAttributeMaxSharedMemoryPerBlock of gfx950 as api_common.hip reads it
KALDI_MAX = 8192                # api_kaldi.hip: d->n_fft > 8192 is refused
FWD_MAX = 8192                  # api_common.hip validate_desc (every forward entry point): n_fft > 8192 is refused before the LDS is
                                # looked at -- the forward's LONG layout would fit up to 9 930, as the inverse's does and is served
BAR = 2e-5                      # forward, mel, adjoint: of each row's float64 peak (test_fuzz_spectrogram_family_vs_aten_stft)
BAR_F64 = 1e-12                 # test_fuzz_float64_spectrogram_vs_aten
ENV_CONDITION = 0.1             # inverse: min / max of the envelope sum w^2 over the row's samples
GAINS = (1.0, 1e-3, 0.0, 1e-2, 1.0, 0.0)       # rows 2 and 5 are all-zero; row 5 sits directly behind a gain-1 row
SEED = 77100


# --------------------------------------------------------------------------- #
# 1. the host mirror                                                          #
# --------------------------------------------------------------------------- #

def plan_radices(n):
    """stft_generic.h plan_radices: 8s, then 4s, a lone 2 only when n = 2 * odd, then 3, 5 and the remaining primes."""
    out, e = [], 0
    while n % 2 == 0:
        n //= 2
        e += 1
    n4 = 2 if (e % 3 == 1 and e >= 4) else (1 if e % 3 == 2 else 0)
    n2 = 1 if e == 1 else 0
    n8 = (e - 2 * n4 - n2) // 3
    out += [8] * n8 + [4] * n4 + [2] * n2
    p = 3
    while n > 1:
        if n % p == 0:
            out.append(p)
            n //= p
        else:
            p += 2
            if p * p > n and n > 1:
                out.append(n)
                n = 1
    return out if len(out) <= 16 else None


def gen_pad(i):
    return i + (i >> 5)


def seq_len(n):
    return gen_pad(n - 1) + 1


def pairs_per_block(n):
    return max(1, min(8, 1024 // n))


def lds_full(n, n_freq, pb):
    """gen_lds_floats: twiddles | two ping-pong buffers | power rows."""
    return 2 * n + 4 * pb * seq_len(n) + 2 * pb * n_freq


def lds_long(n, pb):
    return 4 * pb * seq_len(n)


def lds_inverse(n, pb):
    """api_istft.hip / api_f64.hip: the inverse has no power rows."""
    return 2 * n + 4 * pb * seq_len(n)


def kaldi_pairs_per_block(n):
    return 2 if n <= 2400 else 1


def kaldi_lds(n, pb):
    return 2 * n + 4 * pb * seq_len(n) + 2 * pb * (n // 2 + 2) + 256 + 8 * pb


def kaldi_lds_long(n, pb):
    return 4 * pb * seq_len(n) + 256 + 8 * pb


def launch(kernel, dtype, n, n_frames=1 << 20, rows=1, onesided=True):
    """What the launcher does with (n_fft, n_frames): dict(plan, pb, bpr, blocks, layout, lds) with layout `full`, `long` or
    `refused`.  kernel: fwd (spectrogram and mel epilogue alike), inv (inverse and adjoint), kaldi."""
    plan = plan_radices(n)
    out = dict(n_fft=n, plan=plan, kernel=kernel, dtype=dtype)
    if kernel == "kaldi":
        assert dtype == "f32" and n % 2 == 0
        pb = kaldi_pairs_per_block(n)
        lds, layout = 4 * kaldi_lds(n, pb), "full"
        if plan is None or n > KALDI_MAX:
            layout = "refused"
        elif lds > LDS_OPTIN:
            lds, layout = 4 * kaldi_lds_long(n, pb), "long"
            if lds > LDS_OPTIN:
                layout = "refused"
        bpr = -(-n_frames // (2 * pb))
        return dict(out, pb=pb, bpr=bpr, blocks=bpr * rows, layout=layout, lds=lds)
    pairs = (n_frames + 1) // 2
    pb = min(pairs_per_block(n), pairs)
    n_freq = n // 2 + 1 if onesided else n
    full = (lambda p: lds_full(n, n_freq, p)) if kernel == "fwd" else (lambda p: lds_inverse(n, p))
    if dtype == "f64":
        while 8 * full(pb) > LDS_OPTIN and pb > 1:
            pb //= 2
        lds = 8 * full(pb)
        layout = "full" if lds <= LDS_OPTIN else "refused"
    else:
        lds, layout = 4 * full(pb), "full"
        if lds > LDS_OPTIN:
            lds, layout = 4 * lds_long(n, pb), "long"
            if lds > LDS_OPTIN:
                layout = "refused"
    if plan is None or (kernel == "fwd" and n > FWD_MAX):
        layout = "refused"
    bpr = -(-pairs // pb)
    return dict(out, pb=pb, bpr=bpr, blocks=bpr * rows, layout=layout, lds=lds)


@functools.lru_cache(maxsize=None)
def last_size(kernel, dtype, layout, step=1):
    """The largest n_fft (a multiple of `step`) that `kernel` serves with `layout`."""
    best = None
    for n in range(2 * step if step > 1 else 2, 12000, step):
        if launch(kernel, dtype, n)["layout"] == layout:
            best = n
    assert best is not None, (kernel, dtype, layout)
    return best


MAX_PRIME = 600                 # a prime radix r is ONE work item's r^2 complex MACs per butterfly: sizes that RUN keep r under this


def _smooth(n):
    return max(plan_radices(n)) <= MAX_PRIME


@functools.lru_cache(maxsize=None)
def limits():
    """The exact last size of each layout, as the mirror computes it: {(kernel, dtype, layout): n_fft}."""
    out = {(k, "f32", lay): last_size(k, "f32", lay) for k in ("fwd", "inv") for lay in ("full", "long")}
    out.update({(k, "f64", "full"): last_size(k, "f64", "full") for k in ("fwd", "inv")})
    out[("kaldi", "f32", "full")] = last_size("kaldi", "f32", "full", 2)
    out[("kaldi", "f32", "long")] = last_size("kaldi", "f32", "long", 2)
    return out


def _pair(n_last, step=1):
    """The sizes that run on the two sides of the boundary behind n_last: the nearest whose largest prime factor is <= MAX_PRIME
    (the forward's last full-layout size and the inverse's first long-layout size are primes near 6 000: 3e7 MACs in one work item)."""
    lo = next(m for m in range(n_last, 1, -step) if _smooth(m))
    hi = next(m for m in range(n_last + step, 12000, step) if _smooth(m))
    return lo, hi


@functools.lru_cache(maxsize=None)
def boundaries():
    """Both sides of every layout boundary, from the mirror.  `x|refused`: (last size that runs, FIRST size past the limit)."""
    lim, b = limits(), {}
    for kernel in ("fwd", "inv"):
        b[kernel + "-f32-full|long"] = _pair(lim[(kernel, "f32", "full")])
        b[kernel + "-f32-long|refused"] = (_pair(lim[(kernel, "f32", "long")])[0], lim[(kernel, "f32", "long")] + 1)
        b[kernel + "-f64-full|refused"] = (_pair(lim[(kernel, "f64", "full")])[0], lim[(kernel, "f64", "full")] + 1)
    b["kaldi-full|long"] = _pair(lim[("kaldi", "f32", "full")], 2)
    n = max(m for m in range(2, KALDI_MAX + 1, 2) if kaldi_pairs_per_block(m) == 2)
    b["kaldi-pb2|pb1"] = (n, n + 2)
    b["kaldi-long|refused"] = (lim[("kaldi", "f32", "long")], lim[("kaldi", "f32", "long")] + 2)
    return b


def kernel_name(kernel, dtype, layout, epi="SPEC", mode=0):
    long_ = int(layout == "long")
    if kernel == "fwd":
        return "stft_generic_kernel<%s, EPI_%s, %d>" % ("float" if dtype == "f32" else "double", epi, long_)
    if kernel == "inv":
        return "ola_kernel<float, %d>" % long_ if dtype == "f32" else "ola_kernel<double>"
    return "kaldi_generic_kernel<%d, %d>" % (mode, long_)


KERNELS_WANTED = ({"stft_generic_kernel<float, EPI_%s, %d>" % (e, l) for e in ("SPEC", "MEL") for l in (0, 1)}
                  | {"stft_generic_kernel<double, EPI_SPEC, 0>", "ola_kernel<float, 0>", "ola_kernel<float, 1>", "ola_kernel<double>"}
                  | {"kaldi_generic_kernel<%d, %d>" % (m, l) for m in (0, 1) for l in (0, 1)})

# the census: radix plans written out by hand from reading plan_radices (the mirror and the C++ function are held against them)
PLANS = {
    2: [2], 4: [4], 8: [8], 16: [4, 4], 32: [8, 4], 64: [8, 8], 128: [8, 4, 4], 4096: [8, 8, 8, 8], 8192: [8, 8, 8, 4, 4],
    6: [2, 3], 10: [2, 5], 98: [2, 7, 7], 202: [2, 101], 250: [2, 5, 5, 5],
    15: [3, 5], 225: [3, 3, 5, 5], 243: [3, 3, 3, 3, 3], 125: [5, 5, 5], 441: [3, 3, 7, 7], 1001: [7, 11, 13], 49: [7, 7],
    97: [97], 251: [251], 509: [509], 201: [3, 67], 1102: [2, 19, 29], 1200: [4, 4, 3, 5, 5], 12: [4, 3], 3000: [8, 3, 5, 5, 5],
    400: [4, 4, 5, 5], 512: [8, 8, 8], 2400: [8, 4, 3, 5, 5], 2402: [2, 1201],
}
FAST_PATH = (256, 400, 512, 1024, 2048)     # sizes another kernel would take: the device layer forces the generic one there
PLANS_WANTED = [[2], [4], [8], [4, 4], [8, 4], [8, 8], [8, 4, 4], [8, 8, 8, 8], [8, 8, 8, 4, 4], [2, 3], [2, 5], [2, 7, 7], [2, 101],
                [2, 5, 5, 5], [3, 5], [3, 3, 5, 5], [3, 3, 3, 3, 3], [5, 5, 5], [3, 3, 7, 7], [7, 11, 13], [97], [251], [509], [3, 67],
                [2, 19, 29], [4, 4, 3, 5, 5]]


def between_8192_and_long_limit():
    """Only the inverse serves such a size (FWD_MAX)."""
    n = (8192 + last_size("inv", "f32", "long")) // 2
    return n - n % 2                        # an even size half way: 8 and small odd factors keep the case quick


# --------------------------------------------------------------------------- #
# 2. the cases                                                                #
# --------------------------------------------------------------------------- #

PAD_MODES = ("reflect", "constant", "replicate", "circular")
POWERS = (None, 1.0, 2.0, 0.5)
NORMS = (False, "window", "frame_length")
LAYOUTS = ("contig", "strided", "offset")


def full_frames(n, kernel="fwd", dtype="f32"):
    """2 * (2 pb) + 3: two full workgroups and an odd tail."""
    pb = launch(kernel, dtype, n)["pb"]
    return 2 * (2 * pb) + 3


def _fwd_sizes():
    b = boundaries()
    return sorted((set(PLANS) - {2400, 2402}) | set(b["fwd-f32-full|long"]) | {b["fwd-f32-long|refused"][0]})


def _fwd_case(n, i, **over):
    c = dict(family="fwd", n_fft=n, hop=max(1, n // 4), wl=n, center=True, pad_mode=PAD_MODES[i % 4], pad=0, power=POWERS[(i // 2) % 4],
             norm=NORMS[i % 3], onesided=True, layout=LAYOUTS[i % 3], rows=len(GAINS), shape="full", dtype="f32", epi="SPEC")
    v = i % 5
    if v == 1:
        c["center"] = False
    elif v == 2:
        c["pad"] = 5
    elif v == 3 and n >= 4:
        c["wl"] = max(2, 3 * n // 4)
    if i % 7 == 3:
        c["hop"] = max(1, n // 3)
    c.update(over)
    return c


def _finish(c):
    """n_frames, the signal length that gives them, the launch the mirror expects and the id."""
    n, hop = c["n_fft"], c["hop"]
    fam = c["family"]
    kernel = "inv" if fam in ("inv", "adj") else "fwd"
    T = {"full": full_frames(n, kernel, c["dtype"]), "short": 3, "many": 5}[c["shape"]]
    if fam == "inv":
        L = hop * (T - 1) + n % 2                 # aten::istft's natural length: n_fft + hop (T - 1) - 2 (n_fft // 2)
        c["length_arg"] = L - min(hop - 1, 37) if c["cut"] and hop > 1 else None
        c["length"] = c["length_arg"] if c["length_arg"] is not None else L
    else:
        L = (T - 1) * hop + (hop - 1) // 2 + n % 2 - 2 * c["pad"] + (0 if c["center"] else n - n % 2)
        if c["center"] and c["pad_mode"] == "reflect":
            L = max(L, n // 2 + 1 - 2 * c["pad"])
        L = max(L, 2)
        c["length"] = L
        l1 = L + 2 * c["pad"] + (2 * (n // 2) if c["center"] else 0)
        T = 1 + (l1 - n) // hop
    c["n_frames"] = T
    c["launch"] = launch(kernel, c["dtype"], n, T, c["rows"], c.get("onesided", True))
    c["kernel"] = kernel_name(kernel, c["dtype"], c["launch"]["layout"], c.get("epi", "SPEC"))
    return c


@functools.lru_cache(maxsize=None)
def forward_cases():
    out = []
    for i, n in enumerate(_fwd_sizes()):
        out.append(_fwd_case(n, i))
    k = len(out)
    for j, n in enumerate((6, 15, 49, 98, 243, 251, 1001, 4096)):                       # two-sided output: n_freq = n_fft
        out.append(_fwd_case(n, k + j, onesided=False, tag="twosided"))
    k = len(out)
    for j, n in enumerate((10, 97, 225, 1102, boundaries()["fwd-f32-full|long"][1])):     # hop > n_fft: gaps between frames
        out.append(_fwd_case(n, k + j, hop=n + n // 3 + 1, tag="gap"))
    k = len(out)
    for j, n in enumerate((4, 12, 16, 64, 125, 250, 509)):                               # 3 frames: pb clamped to pairs_per_row = 2
        out.append(_fwd_case(n, k + j, shape="short", tag="short"))
    out.append(_fwd_case(12, 1, shape="many", rows=300, center=True, pad=0, tag="many"))   # row = blockIdx.x / blocks_per_row
    # every pad mode at an odd composite and at 2 * odd, every power at a prime (the cycling above does not promise the cross product)
    for j, pm in enumerate(PAD_MODES):
        out.append(_fwd_case(225, 5 * j, pad_mode=pm, tag="pm-" + pm))
        out.append(_fwd_case(202, 5 * j + 2, pad_mode=pm, tag="pm-" + pm))
    for j, p in enumerate(POWERS):
        out.append(_fwd_case(97, 3 * j, power=p, tag="pw-%s" % p))
    for c in out:
        _finish(c)
        c["id"] = "fwd-%d-%s" % (c["n_fft"], c.get("tag", "census"))
    assert len({c["id"] for c in out}) == len(out)
    return out


@functools.lru_cache(maxsize=None)
def mel_cases():
    b = boundaries()
    sizes = [98, 225, 250, 441, 509, 1001, 1102, 1200, 3000, b["fwd-f32-full|long"][0], b["fwd-f32-full|long"][1], b["fwd-f32-long|refused"][0]]
    out = []
    for i, n in enumerate(sizes):
        c = _fwd_case(n, i, family="mel", epi="MEL", power=(2.0, 1.0)[i % 2], onesided=True, wl=n,
                      n_mels=20 if n < 400 else (40 if n < 3000 else 64), sample_rate=(16000, 22050, 44100)[i % 3])
        c["norm"] = (False, "window")[i % 2]       # MelSpectrogram's `normalized` is a bool
        _finish(c)
        c["id"] = "mel-%d" % n
        out.append(c)
    return out


def envelope_ratio(c):
    """min / max of the envelope sum_t w^2 over the row's samples, from the float64 window: the conditioning of the inverse."""
    n, hop, T = c["n_fft"], c["hop"], c["n_frames"]
    w2 = torch.hann_window(n, dtype=torch.float64).pow(2).view(1, 1, n)
    env = torch.nn.functional.conv_transpose1d(torch.ones(1, 1, T, dtype=torch.float64), w2, stride=hop).view(-1)
    env = env[n // 2: n // 2 + c["length"]]
    return float(env.min() / env.max())


@functools.lru_cache(maxsize=None)
def inverse_cases():
    b = boundaries()
    sizes = sorted((set(PLANS) - {2402, 2400, 2, 3000, 4096}) | set(b["inv-f32-full|long"]) | {b["inv-f32-long|refused"][0], between_8192_and_long_limit()})
    out = []
    for i, n in enumerate(sizes):
        hops = [max(1, n // 4), max(1, n // 3)] + ([n // 2] if n % 2 == 0 else [])
        c = _finish(dict(family="inv", n_fft=n, hop=hops[i % len(hops)], cut=bool(i % 2), rows=len(GAINS), shape="full", dtype="f32",
                         norm=NORMS[i % 3], pad=0, center=True))
        c["id"] = "inv-%d-hop%d%s" % (n, c["hop"], "-cut" if c["length_arg"] is not None else "")
        out.append(c)
    # odd n_fft at hop = n_fft // 2: the envelope of a periodic Hann window stays within [0.5, 1] of its peak as long as the row ends
    # at or before the last frame's centre (every `length` here does), so ENV_CONDITION holds and the yardstick applies unchanged;
    # a row that runs on into the last frame's taper fails the condition (test_generic_census.py shows both) and is not a case
    for n in (225, 1001):
        c = _finish(dict(family="inv", n_fft=n, hop=n // 2, cut=n == 225, rows=len(GAINS), shape="full", dtype="f32", norm=False, pad=0, center=True))
        c["id"] = "inv-%d-half" % n
        out.append(c)
    for n, hop in ((12, 3), (125, 31), (250, 125)):
        c = _finish(dict(family="inv", n_fft=n, hop=hop, cut=False, rows=len(GAINS), shape="short", dtype="f32", norm=False, pad=0, center=True))
        c["id"] = "inv-%d-short" % n
        out.append(c)
    c = _finish(dict(family="inv", n_fft=12, hop=3, cut=True, rows=300, shape="many", dtype="f32", norm=False, pad=0, center=True))
    c["id"] = "inv-12-many"
    out.append(c)
    return [c for c in out if envelope_ratio(c) >= ENV_CONDITION]


@functools.lru_cache(maxsize=None)
def adjoint_cases():
    b = boundaries()
    out = []
    for i, (n, tag) in enumerate(((225, "odd"), (250, "2odd"), (251, "prime"), (1001, "primes"), (b["inv-f32-full|long"][1], "long"))):
        c = _fwd_case(n, i, family="adj", power=(None, 2.0)[i % 2], onesided=True, layout="contig")
        _finish(c)
        c["id"] = "adj-%d-%s" % (n, tag)
        out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def f64_cases():
    b = boundaries()
    out = []
    for i, n in enumerate((15, 98, 251, 441, 1102, b["fwd-f64-full|refused"][0])):
        c = _fwd_case(n, i, dtype="f64", power=(None, 2.0, 1.0)[i % 3], layout="contig", onesided=True)
        _finish(c)
        c["id"] = "f64-fwd-%d" % n
        out.append(c)
    for i, n in enumerate((15, 98, 251, 441, 1102, b["inv-f64-full|refused"][0])):
        c = _finish(dict(family="inv", n_fft=n, hop=max(1, n // 4), cut=bool(i % 2), rows=len(GAINS), shape="full", dtype="f64", norm=False,
                         pad=0, center=True))
        c["id"] = "f64-inv-%d" % n
        assert envelope_ratio(c) >= ENV_CONDITION
        out.append(c)
    return out


def ms_for(samples, sr=16000.0):
    """A duration in milliseconds that compliance.kaldi turns into exactly `samples` (int(sr * ms * 0.001))."""
    ms = samples * 1000.0 / sr
    while int(sr * ms * 0.001) < samples:
        ms = math.nextafter(ms, math.inf)
    assert int(sr * ms * 0.001) == samples
    return ms


@functools.lru_cache(maxsize=None)
def kaldi_cases():
    b = boundaries()
    sizes = [6, 10, 16, 32, 64, 98, 128, 202, 250, 1102, 1200, b["kaldi-pb2|pb1"][0], b["kaldi-pb2|pb1"][1], 4096,
             b["kaldi-full|long"][0], b["kaldi-full|long"][1], 8192]
    out = []
    for i, n in enumerate(sizes):
        fns = ["spectrogram"] if n < 98 else (["spectrogram", "fbank"] if n not in (250, 1102) else ["fbank", "mfcc"])
        if n in b["kaldi-full|long"] or n == 8192:
            fns = ["spectrogram", "fbank"]
        for fn in fns:
            shift = max(1, n // 4) if n < 640 else 160 + 7 * (i % 3)
            kw = dict(sample_frequency=16000.0, frame_length=ms_for(n), frame_shift=ms_for(shift), round_to_power_of_two=False, dither=0.0,
                      remove_dc_offset=bool(i % 2), preemphasis_coefficient=(0.97, 0.0)[i % 2], energy_floor=0.0, snip_edges=bool((i + len(fn)) % 2),
                      raw_energy=bool(i % 3), window_type=("povey", "hamming", "hanning")[i % 3])
            if fn != "spectrogram":
                kw.update(num_mel_bins=23 if n < 1000 else 40, use_energy=bool(i % 2), htk_compat=bool(i % 4 == 1))
            if fn == "mfcc":
                kw.update(num_ceps=13, cepstral_lifter=22.0)
            la = launch("kaldi", "f32", n)
            T = 2 * (2 * la["pb"]) + 3
            n_samples = n + (T - 1) * shift + 3 if kw["snip_edges"] else T * shift - shift // 2 + min(3, shift // 2)
            n_samples = max(n_samples, n)
            frames_of = lambda k: (1 + (k - n) // shift) if kw["snip_edges"] else (k + shift // 2) // shift      # noqa: E731
            if frames_of(n_samples) % (2 * la["pb"]) == 0:       # the tail block must be partial
                n_samples += shift
            m = frames_of(n_samples)
            out.append(dict(id="kaldi-%d-%s" % (n, fn), family="kaldi", dtype="f32", n_fft=n, fn=fn, kw=kw, shift=shift, n_utt=3, length=n_samples, n_frames=m,
                            launch=launch("kaldi", "f32", n, m, 3), kernel=kernel_name("kaldi", "f32", la["layout"], mode=int(fn != "spectrogram"))))
    return out


def refusal_cases():
    """(id, entry point, n_fft, the launcher's message): the first size past each limit."""
    b = boundaries()
    return [("fwd-f32", "spectrogram", b["fwd-f32-long|refused"][1], "audio_amd: n_fft > 8192 not supported"),
            ("inv-f32", "inverse", b["inv-f32-long|refused"][1], "audio_amd: n_fft too large for the LDS"),
            ("fwd-f64", "spectrogram_f64", b["fwd-f64-full|refused"][1], "audio_amd: n_fft too large for the LDS (float64)"),
            ("inv-f64", "inverse_f64", b["inv-f64-full|refused"][1], "audio_amd: n_fft too large for the LDS (float64)"),
            ("kaldi", "kaldi", b["kaldi-long|refused"][1], "audio_amd: padded window too long / too many prime factors for the Kaldi front-end")]


def all_cases():
    return forward_cases() + mel_cases() + inverse_cases() + adjoint_cases() + f64_cases() + kaldi_cases()


# --------------------------------------------------------------------------- #
# 3. inputs and float64 references (CPU)                                      #
# --------------------------------------------------------------------------- #

def _seed(c):
    return SEED + sum(ord(ch) * (i + 1) for i, ch in enumerate(c["id"]))


def gains(rows):
    return torch.tensor([GAINS[r % len(GAINS)] for r in range(rows)], dtype=torch.float32)


def zero_rows(rows):
    return [r for r in range(rows) if GAINS[r % len(GAINS)] == 0.0]


def make_wave(c, rows=None, width=None):
    """(rows, length) float32 in the case's memory layout: standard normal clamped to [-1, 1] times the row gain.  `strided` is a
    view of rows 5 samples further apart with non-zero samples in the gaps, `offset` starts 4 bytes behind an allocation."""
    rows, L = rows or c["rows"], width or c["length"]
    g = torch.Generator().manual_seed(_seed(c))
    dt = torch.float64 if c.get("dtype") == "f64" else torch.float32
    x = torch.randn(rows, L, generator=g, dtype=torch.float32).clamp_(-1.0, 1.0).mul_(gains(rows).view(-1, 1)).to(dt)
    layout = c.get("layout", "contig")
    if layout == "strided":
        base = torch.full((rows, L + 5), 0.75, dtype=dt)
        base[:, :L] = x
        return base[:, :L]
    if layout == "offset":
        flat = torch.full((rows * L + 1,), 0.75, dtype=dt)
        flat[1:] = x.reshape(-1)
        return flat[1:].view(rows, L)
    return x


def place(x, dev):
    """The same values in the same layout on `dev`."""
    if x.is_contiguous() and x.storage_offset() == 0:
        return x.to(dev)
    base = torch.empty(x.untyped_storage().nbytes() // x.element_size(), dtype=x.dtype).set_(x.untyped_storage()).to(dev)
    return base.as_strided(x.shape, x.stride(), x.storage_offset())


def make_spectrum(c):
    """(rows, T, F) complex, frame-major: the row gains, zero rows, DC and Nyquist imaginary parts zero."""
    rows, T, F = c["rows"], c["n_frames"], c["n_fft"] // 2 + 1
    g = torch.Generator().manual_seed(_seed(c) + 1)
    s = torch.randn(rows, T, F, 2, generator=g, dtype=torch.float32).clamp_(-1.0, 1.0).mul_(gains(rows).view(-1, 1, 1, 1))
    s[:, :, 0, 1] = 0.0
    if c["n_fft"] % 2 == 0:
        s[:, :, -1, 1] = 0.0
    s = torch.view_as_complex(s)
    return s.to(torch.complex128) if c.get("dtype") == "f64" else s


def window(c, dtype=torch.float32):
    """The module's window: hann, periodic, in the call's precision."""
    return torch.hann_window(c.get("wl", c["n_fft"]), dtype=dtype)


def scale_of(c):
    """The normalisation factor as functional._stft_desc forms it, from the window in the call's precision."""
    w = window(c, torch.float64 if c.get("dtype") == "f64" else torch.float32).double()
    return {False: 1.0, "window": 1.0 / float(w.pow(2).sum().sqrt()), "frame_length": 1.0 / math.sqrt(c["n_fft"])}[c["norm"]]


def ref_stft(c, x):
    """(rows, L) -> (rows, F, T) complex128: zero padding, torch.stft, normalisation (functional.spectrogram's composition)."""
    xd = x.double().contiguous()
    if c["pad"]:
        xd = torch.nn.functional.pad(xd, (c["pad"], c["pad"]))
    w = window(c, torch.float64 if c["dtype"] == "f64" else torch.float32).double()
    X = torch.stft(xd, c["n_fft"], c["hop"], c["wl"], w, c["center"], c["pad_mode"], False, c["onesided"], return_complex=True)
    return X * scale_of(c)


def power_domain(got, ref, power):
    """(got, ref) as the forward fuzz compares them: complex as (re, im); powers in the power-spectrum domain, because a
    fractional power amplifies the rounding of a near-zero bin without bound."""
    if power is None:
        return torch.view_as_real(got.to(torch.complex128)), torch.view_as_real(ref)
    return got.double().pow(2.0 / power), ref.abs().pow(2.0)


def ref_istft(c, spec_fm, dtype):
    """(rows, T, F) -> (rows, length): torch.istft in `dtype` (complex128: the reference; complex64: the yardstick)."""
    n = c["n_fft"]
    w = window(c, torch.float64 if (dtype == torch.complex128 and c["dtype"] == "f64") else torch.float32)
    w = w.double() if dtype == torch.complex128 else w.float()
    s = spec_fm.transpose(-1, -2).to(dtype)
    # InverseSpectrogram undoes the module's normalisation before aten::istft (functional.py:203-209): linear, so applied behind
    undo = {False: 1.0, "window": float(window(c).double().pow(2).sum().sqrt()), "frame_length": math.sqrt(n)}[c["norm"]]
    return torch.istft(s, n, c["hop"], n, w, True, False, True, c["length_arg"], False) * undo


def ref_adjoint(c, x, r_fm):
    """dL/dx of L = Re sum(Y conj r) (power None) or sum(Y r.real) (a real power) through torch.stft in float64."""
    xr = x.double().contiguous().clone().requires_grad_()
    X = ref_stft(c, xr)
    r = r_fm.transpose(-1, -2).to(torch.complex128)
    if c["power"] is None:
        (X * r.conj()).real.sum().backward()
    else:
        (X.abs().pow(c["power"]) * r.real).sum().backward()
    return xr.grad


# --------------------------------------------------------------------------- #
# 4. the per-row judges                                                       #
# --------------------------------------------------------------------------- #

WORST = {}


def locate(c, row, frame):
    la = c["launch"]
    chunk = frame // (2 * la["pb"])
    return dict(n_fft=c["n_fft"], plan=la["plan"], row=row, frame=frame, workgroup=row * la["bpr"] + chunk, chunk_in_row=chunk,
                pb=la["pb"], layout=la["layout"], kernel=c["kernel"])


def judge_rows(c, got, ref, bars, frame_of, label="gpu"):
    """got, ref: real (rows, ...); bars: per-row fraction of the row's float64 peak (a float or a (rows,) tensor).  All-zero rows
    must come out exactly 0.0; every other row needs a finite non-zero reference peak.  Prints the achieved fraction of the bar."""
    assert got.shape == ref.shape, (c["id"], got.shape, ref.shape)
    rows = ref.shape[0]
    got, ref = got.double().reshape(rows, -1), ref.double().reshape(rows, -1)
    assert bool(torch.isfinite(got).all()), (c["id"], "non-finite output")
    bars = torch.as_tensor(bars, dtype=torch.float64).expand(rows).clone()
    err, where = (got - ref).abs().max(1)
    peak = ref.abs().amax(1)
    zr = zero_rows(rows)
    for r in zr:
        assert float(peak[r]) == 0.0, (c["id"], "the reference of an all-zero row", r)
        w = int(got[r].abs().argmax())
        assert float(got[r].abs().max()) == 0.0, (c["id"], "the all-zero row is not exactly 0", float(got[r].abs().max()), locate(c, r, frame_of(w)))
    live = torch.ones(rows, dtype=torch.bool)
    live[zr] = False
    assert bool((torch.isfinite(peak) & (peak > 0))[live].all()), (c["id"], "a row without a reference peak")
    ratio = torch.where(live, err / peak.clamp_min(1e-300) / bars, torch.zeros_like(err))
    r = int(ratio.argmax())
    worst = float(ratio[r])
    key = (label, c["kernel"])
    if worst >= WORST.get(key, (-1.0,))[0]:
        WORST[key] = (worst, c["id"])
    loc = locate(c, r, frame_of(int(where[r])))
    print("[generic-census] %s %s %s plan=%s pb=%d blocks=%d layout=%s err/bar=%.4f (bar %.3g; worst of this kernel so far %.4f %s) at row %d frame %d"
          % (label, c["kernel"], c["id"], loc["plan"], loc["pb"], c["launch"]["blocks"], loc["layout"], worst, float(bars[r]),
             WORST[key][0], WORST[key][1], r, loc["frame"]))
    assert worst <= 1.0, (c["id"], "per-row err / bar", worst, "err", float(err[r] / peak[r]), "bar", float(bars[r]), loc)
    return worst


def forward_frame_of(c, comp):
    """flat index within a row of a (cols, T[, 2]) output -> frame."""
    return lambda flat: (flat // comp) % c["n_frames"]


def inverse_frame_of(c):
    return lambda flat: min(c["n_frames"] - 1, (flat + c["hop"] // 2) // c["hop"])


def judge_forward(c, got, x, label):
    """got: (rows, F, T) as the module returns it, on the CPU."""
    ref = ref_stft(c, x)
    bar = BAR_F64 if c["dtype"] == "f64" else BAR
    g, r = power_domain(got, ref, c["power"])
    return judge_rows(c, g, r, bar, forward_frame_of(c, 2 if c["power"] is None else 1), label)


def judge_mel(c, got, x, fb, label):
    """got: (rows, n_mels, T); fb: the module's own (F, n_mels) filterbank."""
    ref = ref_stft(c, x)
    ref = torch.matmul(ref.abs().pow(c["power"]).transpose(-1, -2), fb.double()).transpose(-1, -2)
    return judge_rows(c, got, ref, BAR, forward_frame_of(c, 1), label)


def judge_inverse(c, got, spec_fm, label):
    """The suite's yardstick per row: max(2e-5, 4 x the error of aten's own float32 istft); float64 calls: 1e-12."""
    ratio = envelope_ratio(c)
    assert ratio >= ENV_CONDITION, (c["id"], "ill-conditioned: envelope min / max", ratio)
    ref = ref_istft(c, spec_fm, torch.complex128)
    if c["dtype"] == "f64":
        bars = BAR_F64
    else:
        e32 = (ref_istft(c, spec_fm, torch.complex64).double() - ref).abs().amax(1)
        bars = torch.clamp_min(4.0 * e32 / ref.abs().amax(1).clamp_min(1e-300), BAR)
        bars[zero_rows(c["rows"])] = BAR
    return judge_rows(c, got, ref, bars, inverse_frame_of(c), label)


def judge_adjoint(c, got, x, r_fm, label):
    return judge_rows(c, got, ref_adjoint(c, x, r_fm), BAR, inverse_frame_of(c), label)


def kaldi_tolerance(ref, fn, kw):
    """kaldi_fuzz_cases.judge's tolerance, restated for the err / bar record and for locating a failure; the assertion is judge's."""
    if fn == "mfcc":
        return np.full(ref.shape, 2e-2)
    under = ref.max(axis=1, keepdims=True) - ref
    if fn == "fbank" and not kw.get("use_power", True):
        under = 2.0 * under
    return 3e-3 + 2.0 * 3e-7 * np.exp(np.minimum(0.5 * under, 30.0))


def judge_kaldi(c, got, x, label):
    """got: (n_utt, m, cols) numpy; x: (n_utt, n) numpy float32.  kaldi_fuzz_cases.judge against oracle/kaldi_oracle.py."""
    import kaldi_fuzz_cases as KC
    from oracle import kaldi_oracle as KO
    ref = np.concatenate([getattr(KO, c["fn"])(u, **c["kw"]) for u in x], axis=0)
    got = np.asarray(got, dtype=np.float64).reshape(ref.shape[0], -1)
    assert got.shape == ref.shape and np.isfinite(got).all(), (c["id"], got.shape, ref.shape)
    ratio = np.abs(got - ref) / kaldi_tolerance(ref, c["fn"], c["kw"])
    flat = int(ratio.argmax())
    fr = flat // ref.shape[1]
    loc = dict(locate(c, fr // c["n_frames"], fr % c["n_frames"]), column=flat % ref.shape[1])
    key = (label, c["kernel"])
    worst = float(ratio.max())
    if worst >= WORST.get(key, (-1.0,))[0]:
        WORST[key] = (worst, c["id"])
    print("[generic-census] %s %s %s plan=%s pb=%d blocks=%d layout=%s err/tolerance=%.4f (worst of this kernel so far %.4f %s) at %s"
          % (label, c["kernel"], c["id"], loc["plan"], loc["pb"], c["launch"]["blocks"], loc["layout"], worst, WORST[key][0], WORST[key][1], loc))
    try:
        KC.judge(got, ref, c["fn"], c["kw"], ref)
    except AssertionError as e:
        raise AssertionError((c["id"], str(e), "err / tolerance", worst, loc)) from e
    return worst
