"""float64 / complex128 oracle of the MVDR beamforming group, every function written two independent ways: an einsum form and
an explicit per-bin loop with numpy.linalg.solve.  The einsum forms of the two sums (psd, apply_beamforming) accumulate
in extended precision (numpy.clongdouble, a 64-bit significand) so that their own summation error stays far below the
4 * 2^-52 * sum|terms| bound of the complex128 tests; `wide=True` returns that sum unrounded, the default rounds it to
complex128 once.  The formulas are the specification (torchaudio 2.x functional):
specgram (..., C, F, T), masks (..., F, T), PSD (..., F, C, C), weights and RTF (..., F, C)."""
import numpy as np


def _c128(a):
    return np.asarray(a, dtype=np.complex128)


def _bins(lead_shape):
    return list(np.ndindex(*lead_shape))


# ---- psd ------------------------------------------------------------------------------------------------------------------------
def _narrow(a, wide):
    return a if wide else a.astype(np.complex128)


def psd(specgram, mask=None, normalize=True, eps=1e-10, wide=False):
    x = np.asarray(specgram).astype(np.clongdouble)
    if mask is None:
        return _narrow(np.einsum("...cft,...eft->...fce", x, x.conj()), wide)
    m = np.asarray(mask).astype(np.longdouble)
    if normalize:
        m = m / (m.sum(-1, keepdims=True) + np.longdouble(eps))
    return _narrow(np.einsum("...ft,...cft,...eft->...fce", m.astype(np.clongdouble), x, x.conj()), wide)


def psd_loop(specgram, mask=None, normalize=True, eps=1e-10):
    x = _c128(specgram)
    C, F, T = x.shape[-3:]
    out = np.zeros(x.shape[:-3] + (F, C, C), dtype=np.complex128)
    for b in _bins(x.shape[:-3]):
        for f in range(F):
            w = np.ones(T) if mask is None else np.asarray(mask, dtype=np.float64)[b + (f,)]
            if mask is not None and normalize:
                w = w / (w.sum() + eps)
            for t in range(T):
                v = x[b + (slice(None), f, t)]
                out[b + (f,)] += w[t] * np.outer(v, v.conj())
    return out


def psd_abs_terms(specgram, mask=None, normalize=True, eps=1e-10):
    """sum_t |m'| |x_c| |x_e|: the size of what is summed, for the summation bound of the GPU tests."""
    a = np.abs(_c128(specgram))
    if mask is None:
        return np.einsum("...cft,...eft->...fce", a, a)
    m = np.asarray(mask, dtype=np.float64)
    if normalize:
        m = m / (m.sum(-1, keepdims=True) + eps)
    return np.einsum("...ft,...cft,...eft->...fce", np.abs(m), a, a)


# ---- loading / reference ----------------------------------------------------------------------------------------------------------
def loaded(psd_n, diag_eps=1e-7, loading=True):
    a = _c128(psd_n)
    if not loading:
        return a
    tr = np.einsum("...cc->...", a).real
    return a + (tr * diag_eps + 1e-8)[..., None, None] * np.eye(a.shape[-1])


def condition(psd_n, diag_eps=1e-7, loading=True):
    """The largest 2-norm condition number over the bins of the (loaded) noise PSD."""
    return float(np.max(np.linalg.cond(loaded(psd_n, diag_eps, loading))))


def _times_ref(m, ref):
    if isinstance(ref, (int, np.integer)):
        return m[..., :, ref]
    return np.einsum("...fec,...c->...fe", m, _c128(ref))


# ---- weights ----------------------------------------------------------------------------------------------------------------------
def mvdr_weights_souden(psd_s, psd_n, ref, loading=True, diag_eps=1e-7, eps=1e-8):
    a = loaded(psd_n, diag_eps, loading)
    n = np.linalg.solve(a, _c128(psd_s))
    w = n / (np.einsum("...cc->...", n)[..., None, None] + eps)
    return _times_ref(w, ref)


def mvdr_weights_souden_loop(psd_s, psd_n, ref, loading=True, diag_eps=1e-7, eps=1e-8):
    s, nn = _c128(psd_s), _c128(psd_n)
    C = s.shape[-1]
    out = np.zeros(s.shape[:-1], dtype=np.complex128)
    for b in _bins(s.shape[:-2]):
        a = nn[b].copy()
        if loading:
            a = a + (np.trace(a).real * diag_eps + 1e-8) * np.eye(C)
        n = np.linalg.solve(a, s[b])
        w = n / (np.trace(n) + eps)
        u = np.eye(C)[ref] if isinstance(ref, (int, np.integer)) else _c128(ref)[b[:-1]]
        out[b] = w @ u
    return out


def mvdr_weights_rtf(rtf, psd_n, ref=None, loading=True, diag_eps=1e-7, eps=1e-8):
    r = _c128(rtf)
    a = loaded(psd_n, diag_eps, loading)
    n = np.linalg.solve(a, r[..., None])[..., 0]
    w = n / (np.einsum("...c,...c->...", r.conj(), n).real[..., None] + eps)
    if ref is None:
        return w
    if isinstance(ref, (int, np.integer)):
        return w * r[..., ref, None].conj()
    return w * np.einsum("...fc,...c->...f", r.conj(), _c128(ref))[..., None]


def mvdr_weights_rtf_loop(rtf, psd_n, ref=None, loading=True, diag_eps=1e-7, eps=1e-8):
    r, nn = _c128(rtf), _c128(psd_n)
    C = r.shape[-1]
    out = np.zeros(r.shape, dtype=np.complex128)
    for b in _bins(r.shape[:-1]):
        a = nn[b].copy()
        if loading:
            a = a + (np.trace(a).real * diag_eps + 1e-8) * np.eye(C)
        n = np.linalg.solve(a, r[b])
        w = n / (np.vdot(r[b], n).real + eps)
        if ref is not None:
            u = np.eye(C)[ref] if isinstance(ref, (int, np.integer)) else _c128(ref)[b[:-1]]
            w = w * np.vdot(r[b], u)
        out[b] = w
    return out


def rtf_power(psd_s, psd_n, ref, n_iter=3, loading=True, diag_eps=1e-7):
    assert n_iter > 0
    s = _c128(psd_s)
    a = loaded(psd_n, diag_eps, loading)
    phi = np.linalg.solve(a, s)
    r = _times_ref(phi, ref)[..., None]
    if n_iter >= 2:
        for _ in range(n_iter - 2):
            r = phi @ r
        r = s @ r
    else:
        r = a @ r
    return r[..., 0]


def rtf_power_loop(psd_s, psd_n, ref, n_iter=3, loading=True, diag_eps=1e-7):
    s, nn = _c128(psd_s), _c128(psd_n)
    C = s.shape[-1]
    out = np.zeros(s.shape[:-1], dtype=np.complex128)
    for b in _bins(s.shape[:-2]):
        a = nn[b].copy()
        if loading:
            a = a + (np.trace(a).real * diag_eps + 1e-8) * np.eye(C)
        phi = np.linalg.solve(a, s[b])
        u = np.eye(C)[ref] if isinstance(ref, (int, np.integer)) else _c128(ref)[b[:-1]]
        r = phi @ u
        for _ in range(max(n_iter - 2, 0)):
            r = phi @ r
        out[b] = (s[b] if n_iter >= 2 else a) @ r
    return out


# ---- apply ------------------------------------------------------------------------------------------------------------------------
def apply_beamforming(w, specgram, wide=False):
    return _narrow(np.einsum("...fc,...cft->...ft", np.asarray(w).astype(np.clongdouble).conj(),
                             np.asarray(specgram).astype(np.clongdouble)), wide)


def apply_beamforming_loop(w, specgram):
    w, x = _c128(w), _c128(specgram)
    C, F, T = x.shape[-3:]
    out = np.zeros(x.shape[:-3] + (F, T), dtype=np.complex128)
    for b in _bins(x.shape[:-3]):
        for f in range(F):
            for c in range(C):
                out[b + (f,)] += np.conj(w[b + (f, c)]) * x[b + (c, f)]
    return out


def apply_abs_terms(w, specgram):
    return np.einsum("...fc,...cft->...ft", np.abs(_c128(w)), np.abs(_c128(specgram)))


def mvdr(specgram, mask_s, mask_n, ref=0, solution="ref_channel", loading=True, diag_eps=1e-7):
    """T.MVDR: PSD with eps 1e-15, Souden weights or rtf_power + mvdr_weights_rtf, apply."""
    ps, pn = psd(specgram, mask_s, True, 1e-15), psd(specgram, mask_n, True, 1e-15)
    if solution == "ref_channel":
        w = mvdr_weights_souden(ps, pn, ref, loading, diag_eps, 1e-8)
    else:
        w = mvdr_weights_rtf(rtf_power(ps, pn, ref, 3, loading, diag_eps), pn, ref, loading, diag_eps, 1e-8)
    return apply_beamforming(w, specgram)
