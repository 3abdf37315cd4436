"""Oracle of F.overdrive / F.phaser / F.flanger: torchaudio/functional/filtering.py (2.x) restated as literal per-sample
loops in numpy.  `dt` is the compute type (np.float32 or np.float64): every Python scalar is rounded to it before use and
every product and sum is rounded on its own (numpy never contracts).  The modulation tables are float64 on the host.
Nothing here is derived from the kernels."""
import math

import numpy as np


def table(wave, kind, n, mn, mx, phase):
    """_generate_wave_table: wave "SINE" / "TRIANGLE", kind "INT" (int32) / "FLOAT" (float32)."""
    off = int(phase / math.pi / 2 * n + 0.5)
    p = (np.arange(n, dtype=np.int64) + off) % n
    if wave == "SINE":
        d = (np.sin(p.astype(np.float64) / n * 2 * math.pi) + 1) / 2
    else:
        d = p.astype(np.float64) * 2 / n
        v = (4 * p) // n
        d = np.where(v == 0, d + 0.5, np.where((v == 1) | (v == 2), 1.5 - d, d - 1.5))
    d = d * (mx - mn) + mn
    if kind == "INT":
        return np.where(d < 0, d - 0.5, d + 0.5).astype(np.int32)
    return d.astype(np.float32)


def _rows(x, dt):
    x = np.asarray(x)
    return x.reshape(-1, x.shape[-1]).astype(dt), x.shape


def overdrive(x, gain=20.0, colour=20.0, dt=np.float64, return_state=False):
    """return_state: also the recurrence's output y (last_out) of every sample, before the mix and the clamp."""
    x2, shape = _rows(x, dt)
    g, c = dt(math.exp(gain * math.log(10) / 20.0)), dt(colour / 200)
    with np.errstate(invalid="ignore", over="ignore"):
        t = x2 * g + c
        t = np.where(t < -1, dt(-2.0 / 3), np.where(t > 1, dt(2.0 / 3), t - (t * t * t) * dt(1.0 / 3)))
        out = np.empty_like(x2)
        y = np.empty_like(x2)
        last_in = np.zeros(x2.shape[0], dt)
        last_out = np.zeros(x2.shape[0], dt)
        for i in range(x2.shape[1]):
            last_out = (t[:, i] - last_in) + dt(0.995) * last_out
            last_in = t[:, i]
            y[:, i] = last_out
            out[:, i] = x2[:, i] * dt(0.5) + last_out * dt(0.75)
    out = np.clip(out, -1, 1).reshape(shape)
    return (out, y.reshape(shape)) if return_state else out


def overdrive_saturated_share(x, gain=20.0, colour=20.0, dt=np.float64):
    x2, _ = _rows(x, dt)
    t = x2 * dt(math.exp(gain * math.log(10) / 20.0)) + dt(colour / 200)
    return float(np.mean((t < -1) | (t > 1)))


def phaser_plan(sr, delay_ms=3.0, mod_speed=0.5, sinusoidal=True):
    """(L, M, modulation table)"""
    L = int(delay_ms * 0.001 * sr + 0.5)
    M = int(sr / mod_speed + 0.5)
    return L, M, table("SINE" if sinusoidal else "TRIANGLE", "INT", M, 1.0, float(L), math.pi / 2)


def phaser_pre_gain(x, sr, gain_in=0.4, delay_ms=3.0, decay=0.4, mod_speed=0.5, sinusoidal=True, dt=np.float64, form="lag"):
    """The phaser before the output gain and the clamp, as (rows, T).  form "ring": the reference's delay buffer, step for
    step; "lag": t[i] = x[i] gain_in + t[i - (L + 1 - m[i mod M])] decay, samples before the start being zero."""
    x2, _ = _rows(x, dt)
    L, M, m = phaser_plan(sr, delay_ms, mod_speed, sinusoidal)
    R, T = x2.shape
    t = np.zeros((R, T), dt)
    with np.errstate(invalid="ignore", over="ignore"):
        if form == "ring":
            buf = np.zeros((R, L), dt)
            delay_pos = mod_pos = 0
            for i in range(T):
                idx = int((delay_pos + m[mod_pos]) % L)
                mod_pos = (mod_pos + 1) % M
                delay_pos = (delay_pos + 1) % L
                temp = x2[:, i] * dt(gain_in) + buf[:, idx] * dt(decay)
                buf[:, delay_pos] = temp
                t[:, i] = temp
        else:
            zero = np.zeros(R, dt)
            for i in range(T):
                j = i - (L + 1 - int(m[i % M]))
                # the reference multiplies the zero of its fresh buffer by decay as well
                t[:, i] = x2[:, i] * dt(gain_in) + (t[:, j] if j >= 0 else zero) * dt(decay)
    return t


def phaser(x, sr, gain_in=0.4, gain_out=0.74, delay_ms=3.0, decay=0.4, mod_speed=0.5, sinusoidal=True, dt=np.float64,
           form="lag"):
    t = phaser_pre_gain(x, sr, gain_in, delay_ms, decay, mod_speed, sinusoidal, dt, form)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.clip(t * dt(gain_out), -1, 1).reshape(np.asarray(x).shape)


def phaser_clamped_share(x, sr, gain_in=0.4, gain_out=0.74, delay_ms=3.0, decay=0.4, mod_speed=0.5, sinusoidal=True,
                         dt=np.float64):
    t = phaser_pre_gain(x, sr, gain_in, delay_ms, decay, mod_speed, sinusoidal, dt) * dt(gain_out)
    return float(np.mean(np.abs(t) > 1))


def flanger_plan(sr, C, delay=0.0, depth=2.0, regen=0.0, width=71.0, speed=0.5, phase=25.0, modulation="sinusoidal"):
    """(L, N, lfo, cph, feedback gain, in gain, delay gain)"""
    fg, dg, cp = regen / 100, width / 100, phase / 100
    ig = 1.0 / (1 + dg)
    dg = dg / (1 + dg)
    dg = dg * (1 - abs(fg))
    L = int((delay / 1000 + depth / 1000) * sr + 0.5) + 2
    N = int(sr / speed)
    lfo = table("SINE" if modulation == "sinusoidal" else "TRIANGLE", "FLOAT", N, float(math.floor(delay / 1000 * sr + 0.5)),
                L - 2.0, 3 * math.pi / 2)
    cph = ((np.arange(C) * N).astype(np.float32) * np.float32(cp) + np.float32(0.5)).astype(np.int64)   # float32 arithmetic
    return L, N, lfo, cph, fg, ig, dg


def _interp(d0, d1, d2, fr, dt, interpolation):
    if interpolation == "linear":
        return d0 + (d1 - d0) * fr
    d2 = d2 - d0
    d1 = d1 - d0
    a = d2 * dt(0.5) - d1
    b = d1 * dt(2) - d2 * dt(0.5)
    return d0 + (a * fr + b) * fr


def flanger_unclamped(x, sr, delay=0.0, depth=2.0, regen=0.0, width=71.0, speed=0.5, phase=25.0, modulation="sinusoidal",
                      interpolation="linear", dt=np.float64):
    """x: (..., C, T), C <= 4; the reference's loop before the clamp, as (B, C, T)."""
    x = np.asarray(x)
    x3 = x.reshape(-1, x.shape[-2], x.shape[-1]).astype(dt)
    B, C, T = x3.shape
    L, N, lfo, cph, fg, ig, dg = flanger_plan(sr, C, delay, depth, regen, width, speed, phase, modulation)
    bufs = np.zeros((B, C, L), dt)
    last = np.zeros((B, C), dt)
    out = np.empty_like(x3)
    ch = np.arange(C)
    pos = lp = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(T):
            pos = (pos + L - 1) % L
            dtab = lfo[(lp + cph) % N]                              # float32, one per channel
            fr = (dtab - np.floor(dtab)).astype(dt)                 # float32 arithmetic, widened for float64 data
            k = np.floor(dtab).astype(np.int64)
            bufs[:, :, pos] = x3[:, :, i] + last * dt(fg)           # written BEFORE the reads
            d0 = bufs[:, ch, (pos + k) % L]
            d1 = bufs[:, ch, (pos + k + 1) % L]
            d2 = bufs[:, ch, (pos + k + 2) % L]
            d = _interp(d0, d1, d2, fr, dt, interpolation)
            last = d
            out[:, :, i] = x3[:, :, i] * dt(ig) + d * dt(dg)
            lp = (lp + 1) % N
    return out


def flanger(x, sr, delay=0.0, depth=2.0, regen=0.0, width=71.0, speed=0.5, phase=25.0, modulation="sinusoidal",
            interpolation="linear", dt=np.float64):
    out = flanger_unclamped(x, sr, delay, depth, regen, width, speed, phase, modulation, interpolation, dt)
    return np.clip(out, -1, 1).reshape(np.asarray(x).shape)


def flanger_gather(x, sr, delay=0.0, depth=2.0, width=71.0, speed=0.5, phase=25.0, modulation="sinusoidal",
                   interpolation="linear", dt=np.float64):
    """regen == 0 in closed form: the ring holds x itself, out[i] = x[i] ig + interp(x[i - k], x[i - k - 1], x[i - k - 2]) dg
    with zero before the start and a lag of L aliased to 0."""
    x = np.asarray(x)
    x3 = x.reshape(-1, x.shape[-2], x.shape[-1]).astype(dt)
    B, C, T = x3.shape
    L, N, lfo, cph, fg, ig, dg = flanger_plan(sr, C, delay, depth, 0.0, width, speed, phase, modulation)
    out = np.empty_like(x3)
    i = np.arange(T)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(C):
            dtab = lfo[(i + cph[c]) % N]
            fr = (dtab - np.floor(dtab)).astype(dt)
            k = np.floor(dtab).astype(np.int64)

            def tap(q):
                j = i - q % L
                return np.where(j >= 0, x3[:, c, np.maximum(j, 0)], dt(0))
            d = _interp(tap(k), tap(k + 1), tap(k + 2), fr, dt, interpolation)
            out[:, c, :] = x3[:, c, :] * dt(ig) + d * dt(dg)
    return np.clip(out, -1, 1).reshape(x.shape)
