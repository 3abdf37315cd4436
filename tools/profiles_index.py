#!/usr/bin/env python
"""Regenerate profiles/INDEX.md: one row per kept file -- what it is and which claim of DESIGN.md / HISTORY.md it supports."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DESC = [
    (r'r0\d_.*stoi_kernel_stats.*', "rocprofv3 --kernel-trace --stats of 10 STOI and 10 ESTOI calls of F.stoi on (256, 100000) float32 white noise at 10 kHz (every frame kept, the most work a row can have): calls, total and mean time of the five kernels of csrc/stoi.h; the segment kernel's mean is over both modes, its minimum is STOI and its maximum ESTOI", "DESIGN 4.27"),
    (r'r0\d_.*bench_stoi.*', "tools/bench_stoi.py: F.stoi, STOI and ESTOI, on (256, 160000) at 16 kHz, (32, 40000) at 10 kHz and (8, 441000) at 44.1 kHz, float32: the measure at 10 kHz, both F.resample calls on their own and the whole call, time per call and per frame, beside the definition restated in torch on the same device (unfold, argsort, rfft, band matrix), both by one protocol in alternating rounds, and the float64 numpy definition on the host scaled from two rows", "DESIGN 4.27, README kernel table"),
    (r'r0\d_.*bench_edit_distance.*', "tools/bench_edit_distance.py: F.edit_distance_batch, with and without the error counts, on (32, 10, 1500) int32 hypotheses of 100-300 tokens against (32, 300) references, (256, 1, 400) against (256, 400) and (8, 1, 4000) against (8, 4096), time per call and per DP cell, beside the row recurrence restated in torch on the same device (arange + cummin), both by one protocol in alternating rounds, and the reference's Python loop on the host scaled from two pairs", 'DESIGN 4.26, README kernel table'),
    (r'r0\d_.*fuzz_generic_census.*', "pytest tests/test_gpu_fuzz_generic.py -s on an MI355X: per case the kernel instantiation, radix plan, pairs per block, blocks, LDS layout and the achieved fraction of its per-row bar (Kaldi: of `kaldi_fuzz_cases.judge`'s tolerance), the worst fraction per instantiation, 168 passed in 4.1 s", 'DESIGN 2 (generic-kernel census)'),
    (r'r0\d_.*bench_bark_chroma.*', "tools/bench_bark_chroma.py: T.ChromaScale (the dense projection of csrc/dense_fbank.h, 12 chroma) on the frame-major spectrogram of (256, 160000) at n_fft 400 / hop 200 and of (32, 441000) at n_fft 2048 / hop 512, float32, inputs rotating over more than twice the Infinity Cache, beside matmul(spec^T, fb) restated in torch on the same tensors, both by one protocol in alternating rounds, with the spectrogram's bytes at 8 TB/s as the roofline; T.ChromaSpectrogram end to end beside Spectrogram + the restated matmul; T.BarkSpectrogram beside T.MelSpectrogram of the same shape", 'DESIGN 4.25, README kernel table'),
    (r'r0\d_.*bench_dsp_grad.*', "tools/bench_dsp_grad.py: forward + backward (every input requiring grad) of F.oscillator_bank on (16, 64000, 64) and (256, 16000, 1) and of F.filter_waveform on (64, 160000) with 1000 filters of 513 and of 65 taps and on (4, 16000) with 16000 filters of 65 taps, float32, rotating over two draws of the inputs, beside the differentiable torch compositions of audio_amd._diff on the same device, both by one protocol in alternating rounds, with the allocator's peak of one call of each side and the largest relative difference of their gradients; a composition that cannot allocate is recorded as that", 'DESIGN 4.23.1, README kernel table'),
    (r'r0\d_.*bench_dsp.*',"tools/bench_dsp.py: F.oscillator_bank on (16, 64000, 64) and (256, 16000, 1) and F.filter_waveform on (64, 160000) with 1000 filters of 513 and of 65 taps and on (4, 16000) with 16000 filters of 65 taps, float32, rotating over three draws of the inputs, beside the reference's compositions restated in torch on the same device (remainder, float64 cumsum cast back unreduced, sin, sum; unfold, per-chunk FFT convolution, overlap-add, crop), both by one protocol in alternating rounds, with the bytes and multiply-adds of each call as rates", 'DESIGN 4.23, README kernel table'),
    (r'r0\d_.*bench_ray.*', "tools/bench_ray.py: F.ray_tracing_batch on 256 rooms x 4 microphones x 10 000 rays, one band, time_thres 1.0, with scattering 0 and 0.2, and on 1 room x 8 microphones x 100 000 rays x 7 bands, float32, rotating over two draws of rooms, beside the definition restated in torch on the same device (all rays in lockstep under masks, index_add_, float64; 8 rooms scaled to 256), both by one protocol in alternating rounds, with the number of 8-byte atomic adds and their rate", 'DESIGN 4.24, README kernel table'),
    (r'r0\d_.*bench_rir.*', "tools/bench_rir.py: F.simulate_rir_ism_batch on 256 rooms x 4 microphones at order 17 with 8192 samples and on 1 room x 8 microphones at order 10 with 4096 samples, float32, rotating over three draws of rooms, beside the reference's scatter form restated in torch on the same device (4 rooms scaled to 256), both by one protocol in alternating rounds, with the number of taps inside the output", 'DESIGN 4.22, README kernel table'),
    (r'r0\d_.*bench_spectral_pointwise.*', "tools/bench_spectral_pointwise.py: F.gain, T.Vol, F.contrast, F.DB_to_amplitude, the mu-law pair, T.Fade, F.spectral_centroid (whole and per launch, n_fft 400 / 512 / 480) and T.LFCC on (256, 160000) float32 (float16 for two rows), inputs rotating over more than twice the Infinity Cache, beside the reference's compositions restated in torch and torch.clone of the same tensors, alternating rounds", 'DESIGN 4.20, 4.21, README kernel table'),
    (r'r0\d_.*bench_inverse_mel.*', 'tools/bench_inverse_mel.py: F.inverse_mel_scale on (256, 80, 1001) -> 201 and (32, 80, 800) -> 513, float32, time-major and frame-major inputs rotating over more than twice the Infinity Cache, beside relu(matmul(P, x)) restated in torch on the same device, both by one protocol in alternating rounds', 'DESIGN 4.18, README kernel table'),
    (r'r0\d_.*bench_vad.*', "tools/bench_vad.py: F.vad_start on (256, 160000) float32 at 16 kHz and (8, 441000) at 44.1 kHz, inputs rotating over more than twice the Infinity Cache, beside the reference's loop over measurements and channels restated in torch on 2 rows x 20 measurements and scaled, the device time of each launch from a profiled run of its own, and one read of the waveform at 8 TB/s", 'DESIGN 4.19, README kernel table'),
    (r'r0\d_.*bench_effects.*', 'tools/bench_effects.py: F.overdrive, F.phaser and F.flanger (regen = 0 and 50) on (256, 160000) float32 beside the reference\'s per-sample loops restated in torch on 2 000 samples and scaled, and the copy floor of the streaming flanger', 'DESIGN 4.16, README kernel table'),
    (r'r0\d_.*bench_forced_align.*', 'tools/bench_forced_align.py: F.forced_align on 32 x 1500 x 32 with 200 labels and 1 x 30000 x 32 with 2000 labels, float32, beside the reference\'s per-step algorithm restated in torch, alternating rounds', 'DESIGN 4.15, README kernel table'),
    (r'r0\d_.*bench_rnnt_loss.*', 'tools/bench_rnnt_loss.py: F.rnnt_loss forward and forward + backward on 32 x 300 x 100 x 1024 and x 29 float32 beside the reference restated in torch, alternating rounds', 'DESIGN 4.14, README kernel table'),
    (r'r0\d_.*bench_beamform.*', 'tools/bench_beamform.py: T.PSD, F.mvdr_weights_souden, F.apply_beamforming and T.MVDR on 32 x 8 ch x 257 x 1001 complex64 beside the reference restated in torch, alternating rounds', 'DESIGN 4.13, README kernel table'),
    (r'r0\d_.*bench_wave_augment.*', 'tools/bench_wave_augment.py: F.add_noise (with and without lengths) and F.preemphasis on (256, 160000) float32 beside the reference restated in torch, alternating rounds', 'DESIGN 4.12, README kernel table'),
    (r'r0\d_.*bench_spec_augment.*', 'tools/bench_spec_augment.py: the SpecAugment masking kernel beside a device copy and the reference restated in torch, interleaved', 'DESIGN 4.11, README kernel table'),
    (r'r0\d_.*bench_pitch.*', 'tools/bench_pitch.py: F.detect_pitch_frequency beside the reference restated in torch, same device', 'DESIGN 4.10, README kernel table'),
    (r'pmc_traffic_melspec400.json', 'HBM traffic per launch of the headline kernel (fallback of bench.py when rocprofv3 is absent)', 'DESIGN 5, `roofline.traffic`'),
    (r'r0\d_.*bench_driver_flags\.json', "bench.py with the DRIVER's flags (--gpus 1 --steps 20 --warmup 5)", 'the driver-run line reproduces on a builder box'),
    (r'r0\d_.*bench.*\.json', 'one JSON line of bench.py (headline metric, roofline, cpu_baseline; round 4: + `configs`, box probe)', 'DESIGN 0 / 5: the headline number of that build'),
    (r'r0\d_.*configs.*\.jsonl', 'tools/bench_configs.py: one line per BASELINE config (per-GPU shard)', 'DESIGN 0 table, 4.2-4.5'),
    (r'r0\d_.*rocprof.*kernel_stats.*|r0\d_.*configs_kernel_stats.*|r0\d_.*rocprof_configs_stats.*', 'rocprofv3 --kernel-trace --stats summary (tools/prof_summary.py)', 'kernel average durations behind the bench lines (DESIGN 5)'),
    (r'r0\d_.*pmc_.*', 'rocprofv3 --pmc counter summaries (separate passes; FETCH x2 per the guide)', 'traffic = 1.002 x algorithmic bytes; VALU / LDS instruction counts, LDS-active and conflict cycles (DESIGN 4.x)'),
    (r'r0\d_.*gpu_pytest.*|r0\d_.*pytest_gpu.*', '`pytest -m gpu` log on an MI355X (full suite unless the name says otherwise; _reverse / _serialize: reversed order, AMD_SERIALIZE_KERNEL=3)', 'parity green on the GPU at that commit'),
    (r'r0\d_.*smoke.*', '__graft_entry__.smoke() log', 'smoke, stage by stage'),
    (r'r0\d_.*mel400_pool.*', 'tools/bench_pool_ab.py: tail pools of the n_fft = 400 kernel vs static tile runs, through the product API (a -DAAMD_M400_POOLS=1 build)', 'DESIGN 4.1 round 5: built, bit-identical, - 0.8 %, compiled out'),
    (r'r0\d_.*rsm_lab.*', 'tools/rsm_lab.py: A/B of resampler variants (csrc/resample_mfma.h compiled alone per -D variant)', 'DESIGN 4.3 round 5: 8-byte operand reads, priorities, conversion placement'),
    (r'r0\d_.*bench_trim_ab.*', 'bench.py JSON lines, parent and trimmed headline kernel alternating on one box (2000 / 500 and 20 / 5 steps)', 'DESIGN 4.1'),
    (r'r0\d_.*mel400_tile_census.*', 'headline kernel: instruction census of the tile loop per phase from the ISA, before and after the bookkeeping trim', 'DESIGN 4.1'),
    (r'r0\d_.*mel400.*', 'tools/mel400_lab.py A/B runs of headline-kernel variants (interleaved, rotating buffers)', 'DESIGN 4.1 / HISTORY: what moved the headline kernel and what did not'),
    (r'r0\d_.*fuzz_kaldi.*', 'tools/fuzz_campaign.py --only kaldi_front: the device against oracle/kaldi_oracle.py on random Kaldi configurations', 'DESIGN 2: 1 500 seeds, 0 failed; the oracle against the reference itself on the same seeds'),
    (r'r0\d_.*launch_modes.*', 'bench.py --launch graph | eager on one box', 'DESIGN 5: the K steps as a HIP graph run 83-90 us apart, eager launches 70-71: eager stays the default'),
    (r'r0\d_.*lfw_lab.*', 'tools/lfw_ab.py: A/B of biquad-cascade variants (csrc/lfilter_wave.h compiled alone per -D variant)', 'DESIGN 4.4 round 6: slot 0, split passes; response table / 12 filter waves / mover priority left off'),
    (r'r0\d_.*valu_vgpr_banks.*', 'tools/lab/valu_bank.hip: fp32 VALU rate against the register banks of the sources', 'DESIGN 4.4: no difference'),
    (r'r0\d_.*lfilter.*', 'lfilter kernels: ISA notes, lab ablations, shape sweeps, general-order scans', 'DESIGN 4.4'),
    (r'r0\d_.*mfcc.*', 'MFCC paths: one-kernel vs two-kernel timings, epilogue ablation', 'DESIGN 4.2'),
    (r'r0\d_.*resample.*', 'Resample: f16 kernel census, rate-pair sweep', 'DESIGN 4.3'),
    (r'r0\d_.*fftconv.*|r0\d_.*fdr.*', 'fftconvolve: plan A/Bs (recompute / complex-block delay line / round 4: real-block delay line, its pipelined walk)', 'DESIGN 4.5'),
    (r'r0\d_.*ubench.*|r0\d_.*valu_issue.*|r0\d_.*streams.*', 'micro-benchmarks of the chip (VALU / LDS issue rates, streams)', 'HISTORY round 3: 2-2.8 cycles per instruction at 2-3 waves per SIMD'),
    (r'r0\d_.*microbench.*|r0\d_.*shapes.*|r0\d_.*istft.*|r0\d_.*pitchshift.*|r0\d_.*stft.*', 'tools/gpu_microbench.py / shape sweeps of the widening ops (iSTFT, autograd, RNN-T, PitchShift, STFT sizes)', 'DESIGN 4.6-4.8, 7'),
]


def main():
    d = os.path.join(ROOT, "profiles")
    out = ['# profiles/ index\n',
           'Every file here was produced on an MI355X through `gpurun` (scratch under `gpurun_out/`, copied here to be judged).  Names are',
           '`rNN_<step>_<what>`: round, step within the round (alphabetical = chronological; `zz` / `end` / `z` = the last verification',
           'of a round), content.  Intermediate re-runs that a later file of the same round supersedes were removed in round 4 (git',
           'history has them).  Regenerate with `python tools/profiles_index.py`.\n',
           '| file | what it is | claim it supports |', '|---|---|---|']
    for f in sorted(os.listdir(d)):
        if f == "INDEX.md":
            continue
        for pat, what, claim in DESC:
            if re.fullmatch(pat, f):
                out.append(f"| `{f}` | {what} | {claim} |")
                break
        else:
            out.append(f"| `{f}` | (see name) | |")
    with open(os.path.join(d, "INDEX.md"), "w") as fh:
        fh.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
