"""Device-free layer of the generic-kernel census (tests/generic_census.py): the CPU replay of stft_generic_kernel, its mel
epilogue, ola_kernel (inverse and adjoint) and kaldi_generic_kernel (tests/cpu_sim/sim.cpp runs the SAME phase functions as the
device, csrc/stft_generic.h / istft.h / kaldi_generic.h) on the census the device layer (tests/test_gpu_fuzz_generic.py) runs,
against the same float64 references with the same per-row judges -- so the cases, the references and the judges are tested where
no GPU is, and a wrong butterfly, twiddle index or Hermitian edge rule fails here first.  Also here: the host mirror of the
launch arithmetic against the C++ functions themselves, and the census assertions (every radix plan, every kernel instantiation,
both sides of every boundary).

What the replay cannot show is what only the device has: the LDS carving of the LONG layout (the replay uses plain arrays for
both layouts), barriers, atomics and alignment.  That is the device layer's job.

Checked once by hand on a copy (nothing of it is committed) that this file fails under each of three mutations, of its 137 tests:
the generic-prime branch of gen_stage reading tw[nb * k] for tw[nb * e]: 60 fail (every case with a prime factor >= 7, in the
forward, mel, inverse, adjoint and Kaldi replays); ola_conj_z taking kk == N / 2 as its edge rule: 17 fail (the odd-n_fft inverse
and adjoint cases, and only those); the sign of C2 in bfly5: 41 fail (every case with a factor 5).
"""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import generic_census as G
import sim_util as S
from audio_amd import _host, _lib

LABEL = "replay"


# --------------------------------------------------------------------------- #
# the mirror against the headers, the census                                  #
# --------------------------------------------------------------------------- #

def test_mirror_equals_the_headers_planning_functions():
    """plan_radices, pairs per block, sequence length and every LDS formula of the mirror against the C++ functions themselves,
    on the census, around every boundary and over a sweep."""
    sizes = set(G.PLANS) | {n for pair in G.boundaries().values() for n in pair} | set(range(2, 700)) | set(range(2390, 2410))
    for lim in G.limits().values():
        sizes |= set(range(lim - 3, lim + 4))
    sizes |= {int(v) for v in np.random.default_rng(G.SEED).integers(2, 12000, 300)}
    for n in sorted(sizes):
        assert S.sim_plan_radices(n) == G.plan_radices(n), n
        h = S.sim_generic_sizes(n)
        assert h["pb"] == G.pairs_per_block(n) and h["seq_len"] == G.seq_len(n), n
        for pb in {1, 2, h["pb"]}:
            for n_freq in (n // 2 + 1, n):
                assert h["lds_full"](pb, n_freq) == G.lds_full(n, n_freq, pb), (n, pb, n_freq)
            assert h["lds_long"](pb) == G.lds_long(n, pb), (n, pb)
            # the inverse's formula (api_istft.hip, api_f64.hip) is the forward's without the power rows
            assert G.lds_inverse(n, pb) == h["lds_full"](pb, 0), (n, pb)
        assert h["kaldi_pb"] == G.kaldi_pairs_per_block(n), n
        assert h["kaldi_full"] == G.kaldi_lds(n, h["kaldi_pb"]) and h["kaldi_long"] == G.kaldi_lds_long(n, h["kaldi_pb"]), n
    for n, plan in G.PLANS.items():
        assert S.sim_plan_radices(n) == plan == G.plan_radices(n) and int(np.prod(plan)) == n, (n, plan)
    assert S.sim().sim_gen_lds_bytes(6000, 1, 1) == 4 * G.lds_long(6000, 1)       # the export test_long_windows.py uses


def test_boundaries_come_from_the_lds_opt_in():
    """Each limit is the last size whose layout fits 160 KB, the next size takes the next layout; the pair of sizes that RUN lies
    on the two sides of it, as near as a largest prime factor <= MAX_PRIME allows."""
    lim, b = G.limits(), G.boundaries()
    for (kernel, dtype, layout), n in lim.items():
        step = 2 if kernel == "kaldi" else 1
        nxt = {"full": "long" if dtype == "f32" else "refused", "long": "refused"}[layout]
        assert G.launch(kernel, dtype, n)["layout"] == layout and G.launch(kernel, dtype, n + step)["layout"] == nxt, (kernel, dtype, n)
        assert G.launch(kernel, dtype, n)["lds"] <= G.LDS_OPTIN, (kernel, dtype, n)
    # the neighbourhoods the kernels' comments name: ~5 745 / ~6 690 / ~9 900 / ~2 870 / ~3 340
    assert 5700 < lim[("fwd", "f32", "full")] < 5800 and 6650 < lim[("inv", "f32", "full")] < 6720
    assert lim[("fwd", "f32", "long")] == G.FWD_MAX == 8192 and 9800 < lim[("inv", "f32", "long")] < 10000
    assert 2850 < lim[("fwd", "f64", "full")] < 2900 and 3300 < lim[("inv", "f64", "full")] < 3380
    assert lim[("kaldi", "f32", "long")] == 8192 and b["kaldi-pb2|pb1"] == (2400, 2402)
    for name, (lo, hi) in b.items():
        kernel, dtype = name.split("-")[0], "f64" if "f64" in name else "f32"
        if name == "kaldi-pb2|pb1":
            continue
        a, z = name.split("-")[-1].split("|")
        assert G.launch(kernel, dtype, lo)["layout"] == a and G.launch(kernel, dtype, hi)["layout"] == z, name
        assert max(G.plan_radices(lo)) <= G.MAX_PRIME and (z == "refused" or max(G.plan_radices(hi)) <= G.MAX_PRIME), name
        assert lo > 0.99 * hi, name
    assert 8192 < G.between_8192_and_long_limit() < lim[("inv", "f32", "long")]


def test_census_draws_every_plan_layout_and_instantiation():
    cases = G.all_cases()
    assert len({c["id"] for c in cases}) == len(cases)
    by_kernel = {}
    for c in cases:
        assert c["launch"]["layout"] in ("full", "long"), c["id"]
        assert c["launch"]["plan"] == G.plan_radices(c["n_fft"]), c["id"]
        by_kernel.setdefault(c["kernel"], []).append(c)
    assert set(by_kernel) == G.KERNELS_WANTED, set(by_kernel) ^ G.KERNELS_WANTED
    fwd_plans = [c["launch"]["plan"] for c in G.forward_cases()]
    inv_plans = [c["launch"]["plan"] for c in G.inverse_cases()]
    for plan in G.PLANS_WANTED:
        assert plan in fwd_plans, plan
        if plan not in ([2], [8, 8, 8, 8]):          # n_fft = 2: the envelope condition fails; 4096: the forward and Kaldi run it
            assert plan in inv_plans, plan
    kaldi_plans = [c["launch"]["plan"] for c in G.kaldi_cases()]
    for plan in ([2, 3], [2, 5], [4, 4], [8, 4], [8, 8], [8, 4, 4], [2, 7, 7], [2, 101], [2, 5, 5, 5], [2, 19, 29], [4, 4, 3, 5, 5],
                 [8, 4, 3, 5, 5], [2, 1201], [8, 8, 8, 8], [8, 8, 8, 4, 4]):
        assert plan in kaldi_plans, plan
    b = G.boundaries()
    ran = lambda fam, dtype: {c["n_fft"] for c in cases if c["family"] in fam and c["dtype"] == dtype}        # noqa: E731
    assert set(b["fwd-f32-full|long"]) | {b["fwd-f32-long|refused"][0]} <= ran(("fwd",), "f32")
    assert set(b["fwd-f32-full|long"]) <= ran(("mel",), "f32")
    assert set(b["inv-f32-full|long"]) | {b["inv-f32-long|refused"][0], G.between_8192_and_long_limit()} <= ran(("inv",), "f32")
    assert b["fwd-f64-full|refused"][0] in ran(("fwd",), "f64") and b["inv-f64-full|refused"][0] in ran(("inv",), "f64")
    kal = {c["n_fft"] for c in G.kaldi_cases()}
    assert set(b["kaldi-full|long"]) | set(b["kaldi-pb2|pb1"]) | {8192} <= kal
    # call shapes: two-sided, hop > n_fft, clamped pb, many rows, every layout, pad mode, power and normalisation, both `length`s
    f = G.forward_cases()
    assert any(not c["onesided"] for c in f) and any(c["hop"] > c["n_fft"] for c in f) and any(not c["center"] for c in f)
    assert any(c["pad"] > 0 for c in f) and any(c["wl"] < c["n_fft"] for c in f)
    assert any(c["shape"] == "short" and c["launch"]["pb"] < G.pairs_per_block(c["n_fft"]) for c in f)
    assert any(c["rows"] >= 300 and c["n_fft"] == 12 and c["n_frames"] == 5 and c["launch"]["blocks"] >= 300 for c in f)
    for key, values in (("layout", G.LAYOUTS), ("pad_mode", G.PAD_MODES), ("power", G.POWERS), ("norm", G.NORMS)):
        assert {c[key] for c in f} == set(values), key
    for c in f + G.mel_cases():
        if c["shape"] == "full":
            assert c["n_frames"] == 2 * 2 * c["launch"]["pb"] + 3 and c["n_frames"] % 2 == 1, (c["id"], c["n_frames"])
    inv = G.inverse_cases()
    assert any(c["length_arg"] is None for c in inv) and any(c["length_arg"] is not None for c in inv)
    assert any(c["n_fft"] % 2 and c["n_fft"] > 200 for c in inv)
    assert any(c["launch"]["layout"] == "long" for c in G.mel_cases()) and any(c["launch"]["layout"] == "long" for c in G.adjoint_cases())
    for c in G.kaldi_cases():
        assert c["launch"]["bpr"] > 1 and c["n_frames"] % (2 * c["launch"]["pb"]) != 0 and c["n_utt"] > 1, c["id"]
    assert max(c["rows"] * c["length"] * 4 for c in cases if c["family"] != "kaldi") < 4 << 20


def test_measured_record_names_every_instantiation():
    """The device file's record of measured worst fractions has one entry per instantiation, each an existing case under its bar."""
    import test_gpu_fuzz_generic as D
    ids = {c["id"]: c for c in G.all_cases()}
    assert set(D.MEASURED_DEVICE) == G.KERNELS_WANTED
    for kernel, (ratio, case) in D.MEASURED_DEVICE.items():
        assert 0.0 < ratio < 1.0 and ids[case]["kernel"] == kernel, (kernel, ratio, case)


def test_envelope_condition_holds_for_every_case_and_bites_in_a_taper():
    """min / max of sum w^2 over the row's samples, from the float64 window, is >= 0.1 for every inverse case (hop n // 4 and
    n // 3 of any n_fft, n // 2 of even and of the two odd sizes drawn: a periodic Hann window at half overlap stays in [0.5, 1]),
    and it falls under 0.1 as soon as a row runs on into the last frame's taper -- the shapes where aten's own float32 istft is
    1e-4 off: such a row is not a case."""
    for c in G.inverse_cases() + [c for c in G.f64_cases() if c["family"] == "inv"]:
        assert G.envelope_ratio(c) >= G.ENV_CONDITION, c["id"]
    for n in (15, 225, 441, 1001, 250):
        hop, T = n // 2, 11
        natural = hop * (T - 1) + n % 2
        assert G.envelope_ratio(dict(n_fft=n, hop=hop, n_frames=T, length=natural)) >= 0.5 - 1e-9, n
        assert G.envelope_ratio(dict(n_fft=n, hop=hop, n_frames=T, length=natural + n // 2 - 1)) < G.ENV_CONDITION, n


# --------------------------------------------------------------------------- #
# the census through the CPU replay                                           #
# --------------------------------------------------------------------------- #

def _desc(c, x):
    rows, L = x.shape
    return _lib.StftDesc(rows, L, x.stride(0), c["n_fft"], c["hop"], c["pad"], int(c["center"]), _lib.PAD_MODES[c["pad_mode"]],
                         int(c["onesided"]), c["n_frames"], G.scale_of(c), 0.0 if c["power"] is None else float(c["power"]))


def _wp(c):
    return np.ascontiguousarray(_host.center_pad_window(G.window(c), c["n_fft"]).numpy())


def _base(x):
    """The numpy array over x's whole storage and the element offset of x in it (row-strided and offset views keep their layout)."""
    flat = torch.empty(0, dtype=x.dtype).set_(x.untyped_storage())
    return flat.numpy(), x.storage_offset()


def replay_forward(c, x, bands=None):
    """sim_stft_generic on x in ITS layout: (rows, F or n_mels, T), complex for power None."""
    assert x.dtype == torch.float32
    desc = _desc(c, x)
    flat, off = _base(x)
    n_freq = c["n_fft"] // 2 + 1 if c["onesided"] else c["n_fft"]
    comp = 2 if (bands is None and c["power"] is None) else 1
    width = bands.n_mels if bands is not None else n_freq * comp
    out = np.zeros((desc.rows, desc.n_frames, width), dtype=np.float32)
    tw = np.ascontiguousarray(_host.twiddle_table(c["n_fft"]))
    wp = _wp(c)
    f = S.sim().sim_stft_generic
    f.argtypes = [C.c_void_p] * 5 + [C.POINTER(_lib.StftDesc), C.c_int]
    rc = f(flat.ctypes.data + 4 * off, S.fptr(wp), S.fptr(tw), None if bands is None else C.cast(C.byref(bands.struct), C.c_void_p),
           S.fptr(out), C.byref(desc), int(bands is not None))
    assert rc == 0, c["id"]
    out = torch.from_numpy(out)
    if comp == 2:
        out = torch.view_as_complex(out.view(desc.rows, desc.n_frames, n_freq, 2))
    return out.transpose(-1, -2)


@pytest.mark.parametrize("c", G.forward_cases(), ids=[c["id"] for c in G.forward_cases()])
def test_census_forward_replay_vs_float64(c):
    x = G.make_wave(c)
    got = replay_forward(c, x)
    assert got.shape[-1] == c["n_frames"]
    G.judge_forward(c, got, x, LABEL)


def mel_bank(c):
    """The MelSpectrogram module of a mel case (CPU) -- its filterbank is what both sides use."""
    import audio_amd.transforms as T
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")         # (narrow filters at the low end have no bin at small n_fft: the reference warns too)
        return T.MelSpectrogram(sample_rate=c["sample_rate"], n_fft=c["n_fft"], hop_length=c["hop"], win_length=c["wl"], n_mels=c["n_mels"],
                                pad=c["pad"], power=c["power"], normalized=c["norm"] == "window", center=c["center"], pad_mode=c["pad_mode"])


@pytest.mark.parametrize("c", G.mel_cases(), ids=[c["id"] for c in G.mel_cases()])
def test_census_mel_replay_vs_float64(c):
    m = mel_bank(c)
    x = G.make_wave(c)
    got = replay_forward(c, x, S.HostBands(m.mel_scale.fb.numpy()))
    G.judge_mel(c, got, x, m.mel_scale.fb, LABEL)


def inverse_envelope(c):
    """1 / sum_t w^2 over the output samples, as functional.inverse_spectrogram builds it."""
    n, hop, T = c["n_fft"], c["hop"], c["n_frames"]
    w2 = torch.from_numpy(_wp(c)).double().pow(2).view(1, 1, n)
    env = torch.nn.functional.conv_transpose1d(torch.ones(1, 1, T, dtype=torch.float64), w2, stride=hop).view(-1)
    env = env[n // 2: n // 2 + c["length"]]
    return (1.0 / env).float().numpy()


@pytest.mark.parametrize("c", G.inverse_cases(), ids=[c["id"] for c in G.inverse_cases()])
def test_census_inverse_replay_vs_float64(c):
    spec = G.make_spectrum(c)
    undo = {False: 1.0, "window": float(G.window(c).double().pow(2).sum().sqrt()), "frame_length": float(np.sqrt(c["n_fft"]))}[c["norm"]]
    got = S.sim_istft(spec.numpy(), _wp(c), c["length"], c["n_fft"], c["hop"], center=True, pad_mode="constant", scale=undo,
                      inv_env=inverse_envelope(c))
    G.judge_inverse(c, torch.from_numpy(got), spec, LABEL)


@pytest.mark.parametrize("c", G.adjoint_cases(), ids=[c["id"] for c in G.adjoint_cases()])
def test_census_adjoint_replay_vs_float64_autograd(c):
    """What _SpectrogramFunction.backward launches: G = r (complex output) or dP p |X|^(p-2) X with X recomputed, then ola_kernel with
    adjoint = 1 and the forward's padding map."""
    x = G.make_wave(c)
    r = G.make_spectrum(c)
    if c["power"] is None:
        g = r
    else:
        assert c["power"] == 2.0
        X = replay_forward(dict(c, power=None), x).transpose(-1, -2)
        g = (2.0 * r.real * X).to(torch.complex64)
    got = S.sim_istft(g.numpy(), _wp(c), c["length"], c["n_fft"], c["hop"], center=c["center"], pad_mode=c["pad_mode"], pad=c["pad"],
                      scale=G.scale_of(c), adjoint=True)
    G.judge_adjoint(c, torch.from_numpy(got), x, r, LABEL)


# (the replay has no DCT stage: the device layer runs mfcc)
KALDI_REPLAY = [c for c in G.kaldi_cases() if c["fn"] != "mfcc" and (c["n_fft"] in (6, 98, 250, 1102, 2402) or c["launch"]["layout"] == "long")]


@pytest.mark.parametrize("c", KALDI_REPLAY, ids=[c["id"] for c in KALDI_REPLAY])
def test_census_kaldi_replay_vs_oracle(c):
    """kaldi_generic_kernel's replay, utterance by utterance, against oracle/kaldi_oracle.py with kaldi_fuzz_cases.judge."""
    kw, n = c["kw"], c["n_fft"]
    x = G.make_wave(c, rows=c["n_utt"]).numpy()
    w = np.asarray(_host.kaldi_window(kw["window_type"], n, 0.42).numpy(), dtype=np.float32)
    bands, cols = None, {}
    if c["fn"] == "fbank":
        nb = kw["num_mel_bins"]
        bins, _ = _host.kaldi_get_mel_banks(nb, n, 16000.0, 20.0, 0.0, 100.0, -500.0, 1.0)
        bands = S.HostBands(torch.nn.functional.pad(bins.float(), (0, 1)).T.contiguous().numpy())
        if kw["use_energy"]:
            cols = dict(energy_col=nb if kw["htk_compat"] else 0, first_col=0 if kw["htk_compat"] else 1, n_cols=nb + 1)
    got = np.stack([S.sim_kaldi_features(u, w, n, c["shift"], n, snip_edges=kw["snip_edges"], preemph=kw["preemphasis_coefficient"],
                                         remove_dc=kw["remove_dc_offset"], raw_energy=kw["raw_energy"], energy_floor=kw["energy_floor"],
                                         bands=bands, force_generic=True, **cols) for u in x])
    assert got.shape[1] == c["n_frames"], (got.shape, c["n_frames"])
    G.judge_kaldi(c, got, x, LABEL)
