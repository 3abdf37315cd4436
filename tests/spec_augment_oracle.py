"""Oracle for the SpecAugment masking ops (helper module, not a pytest file).

Three independent pieces:
  bounds()            the mask bounds of F.mask_along_axis_iid from explicit draws, evaluated by torch on the CPU with the
                      tensor dtype's roundings (value = r0 * mask_param, min_value = r1 * (size - value),
                      start = long(min_value), end = start + long(value));
  apply()             the masking itself as plain loops over examples, masks and masked rows / columns, on bit views;
  torch_reference_*   the reference's functions and SpecAugment.forward restated in torch for any device (torchaudio 2.x
                      functional/functional.py: _get_mask_param, mask_along_axis, mask_along_axis_iid; transforms:
                      SpecAugment).  `rand` can be injected; the default torch.rand makes a seeded call comparable with
                      the package's on the same device.
Axis tags: 0 = frequency (dim -2), 1 = time (dim -1).
"""
import numpy as np
import torch

FREQ, TIME = 0, 1
BITS = {2: torch.int16, 4: torch.int32, 8: torch.int64}


def get_mask_param(mask_param, p, axis_length):
    if p == 1.0:
        return mask_param
    return min(mask_param, int(axis_length * p))


def bounds(draws, mask_param, size, dtype):
    """draws: (2, ...) tensor (any float dtype; cast to `dtype`) -> (start, end) int64 numpy arrays of shape draws.shape[1:].

    The arithmetic is the device's: aten's element-wise kernels there compute float16 / bfloat16 in float32 and round each
    result to the type, and take the Python scalars mask_param and size as float32 without rounding them to the type first
    (aten's CPU kernels round `size` to the type before the subtraction, which differs only where the type does not hold
    size: float16 axes beyond 2048, bfloat16 axes beyond 256)."""
    d = torch.as_tensor(draws).detach().cpu().to(dtype)
    if dtype in (torch.float16, torch.bfloat16):
        def rnd(t):
            return t.to(dtype).to(torch.float32)
        r = d.to(torch.float32)
        value = rnd(r[0] * torch.tensor(float(mask_param), dtype=torch.float32))
        min_value = rnd(r[1] * rnd(torch.tensor(float(size), dtype=torch.float32) - value))
    else:
        value = d[0] * mask_param
        min_value = d[1] * (size - value)
    start = min_value.long()
    end = min_value.long() + value.long()
    return start.numpy(), end.numpy()


def bit_view(t):
    """CPU integer view of a tensor's elements (NaN payloads and -0.0 count)."""
    t = t.detach().cpu().contiguous()
    return t.view(BITS[t.element_size()])


def value_bits(value, dtype):
    if isinstance(value, torch.Tensor):
        t = value.detach().cpu().to(dtype).reshape(())
    else:
        t = torch.full((), value, dtype=dtype)
    return int(t.view(BITS[t.element_size()]).item())


def apply(x, mask_bounds, axes, value):
    """x: (..., freq, time) tensor; mask_bounds: per mask (start, end), scalars (shared) or arrays over x.shape[:-2];
    axes: per mask FREQ / TIME; value: number or one-element tensor.  -> integer bit view of the result, x's shape."""
    xb = bit_view(x).numpy().copy()
    shape = xb.shape
    n_freq, n_time = shape[-2], shape[-1]
    out = xb.reshape(-1, n_freq, n_time)
    vb = value_bits(value, x.dtype)
    for e in range(out.shape[0]):
        for (start, end), axis in zip(mask_bounds, axes):
            s = int(np.asarray(start).reshape(-1)[e]) if np.ndim(start) else int(start)
            t = int(np.asarray(end).reshape(-1)[e]) if np.ndim(end) else int(end)
            size = n_time if axis == TIME else n_freq
            for i in range(max(s, 0), min(t, size)):
                if axis == TIME:
                    out[e, :, i] = vb
                else:
                    out[e, i, :] = vb
    return out.reshape(shape)


# ---- the reference, restated ------------------------------------------------------------------------------------------------

def torch_reference_mask_along_axis_iid(specgrams, mask_param, mask_value, axis, p=1.0, rand=None):
    rand = rand or torch.rand
    dim = specgrams.dim()
    if dim < 3:
        raise ValueError(f"Spectrogram must have at least three dimensions ({dim} given).")
    if axis not in [dim - 2, dim - 1]:
        raise ValueError("Only Frequency and Time masking are supported"
                         f" (axis {dim - 2} and axis {dim - 1} supported; {axis} given).")
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"The value of p must be between 0.0 and 1.0 ({p} given).")
    mask_param = get_mask_param(mask_param, p, specgrams.shape[axis])
    if mask_param < 1:
        return specgrams
    device, dtype = specgrams.device, specgrams.dtype
    value = rand(specgrams.shape[: (dim - 2)], device=device, dtype=dtype) * mask_param
    min_value = rand(specgrams.shape[: (dim - 2)], device=device, dtype=dtype) * (specgrams.size(axis) - value)
    mask_start = min_value.long()[..., None, None]
    mask_end = (min_value.long() + value.long())[..., None, None]
    # (the index ramp in int64: "element i is masked iff start <= i < end" for every dtype and axis length)
    mask = torch.arange(0, specgrams.size(axis), device=device)
    specgrams = specgrams.transpose(axis, -1)
    specgrams = specgrams.masked_fill((mask >= mask_start) & (mask < mask_end), mask_value)
    return specgrams.transpose(axis, -1)


def torch_reference_mask_along_axis(specgram, mask_param, mask_value, axis, p=1.0, rand=None):
    rand = rand or torch.rand
    dim = specgram.dim()
    if dim < 2:
        raise ValueError(f"Spectrogram must have at least two dimensions (time and frequency) ({dim} given).")
    if axis not in [dim - 2, dim - 1]:
        raise ValueError("Only Frequency and Time masking are supported"
                         f" (axis {dim - 2} and axis {dim - 1} supported; {axis} given).")
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"The value of p must be between 0.0 and 1.0 ({p} given).")
    mask_param = get_mask_param(mask_param, p, specgram.shape[axis])
    if mask_param < 1:
        return specgram
    shape = specgram.size()
    specgram = specgram.reshape([-1] + list(shape[-2:]))
    value = rand(1) * mask_param
    min_value = rand(1) * (specgram.size(axis - dim) - value)
    mask_start = (min_value.long()).squeeze()
    mask_end = (min_value.long() + value.long()).squeeze()
    mask = torch.arange(0, specgram.shape[axis - dim], device=specgram.device)
    mask = (mask >= mask_start.to(specgram.device)) & (mask < mask_end.to(specgram.device))
    if axis == dim - 2:
        mask = mask.unsqueeze(-1)
    if mask_end - mask_start >= mask_param:
        raise ValueError("Number of columns to be masked should be less than mask_param")
    specgram = specgram.masked_fill(mask, mask_value)
    return specgram.reshape(shape[:-2] + specgram.shape[-2:])


def torch_reference_spec_augment(specgram, n_time_masks, time_mask_param, n_freq_masks, freq_mask_param, iid_masks=True,
                                 p=1.0, zero_masking=False, rand=None):
    if zero_masking:
        mask_value = 0.0
    else:
        mask_value = specgram.mean()
    time_dim = specgram.dim() - 1
    freq_dim = time_dim - 1
    fn = torch_reference_mask_along_axis_iid if specgram.dim() > 2 and iid_masks is True else torch_reference_mask_along_axis
    for _ in range(n_time_masks):
        specgram = fn(specgram, time_mask_param, mask_value, time_dim, p=p, rand=rand)
    for _ in range(n_freq_masks):
        specgram = fn(specgram, freq_mask_param, mask_value, freq_dim, p=p, rand=rand)
    return specgram


def injected(draws):
    """A `rand` that hands out the given tensors in order (each reshaped to the requested size, moved to the device)."""
    it = iter(draws)

    def rand(size, device=None, dtype=None):
        t = next(it)
        size = (size,) if isinstance(size, int) else tuple(size)
        return t.reshape(size).to(device=device or "cpu", dtype=dtype or t.dtype)
    return rand
