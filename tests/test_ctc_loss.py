"""F.ctc_loss / T.CTCLoss without a GPU: the host-side checks (raised before any device work), the refusal of CPU tensors,
the public names, and the C ABI's own argument checks."""
import pytest
import torch

import audio_amd.functional as F
import audio_amd.transforms as T
from audio_amd import _lib

X, TG = torch.randn(6, 2, 5), torch.tensor([[1, 2], [3, 4]])
IL, TL = torch.tensor([6, 6]), torch.tensor([2, 2])


@pytest.mark.parametrize("args, kwargs, err, text", [
    ((X, TG, IL, TL), dict(reduction="avg"), ValueError, "reduction should be one of"),
    ((X[0, 0], TG, IL, TL), {}, ValueError, "logits must be 3-D"),
    ((X, TG[None], IL, TL), {}, ValueError, "targets must be 2-D"),
    ((X[:, 0], TG, IL[:1], TL[:1]), {}, ValueError, "targets must be 1-D"),
    ((X, TG[:1], IL, TL), {}, ValueError, "batch sizes differ"),
    ((X, TG, IL[:1], TL), {}, ValueError, "input_lengths must hold one length per example"),
    ((X, TG, IL, (2, 2, 2)), {}, ValueError, "target_lengths must hold one length per example"),
    ((X, TG, IL, TL), dict(blank=5), ValueError, r"blank must lie in \[0, 5\)"),
    ((X, TG, IL, TL), dict(blank=-1), ValueError, "blank must lie in"),
    ((X.long(), TG, IL, TL), {}, TypeError, "logits must be float32, float64, float16 or bfloat16"),
    ((X, TG.float(), IL, TL), {}, TypeError, "targets must be int32 or int64"),
    ((X, TG, IL.float(), TL), {}, TypeError, "input_lengths must be int32 or int64"),
    ((X, torch.ones(2, F.CTC_MAX_TARGET + 1, dtype=torch.long), IL, TL), {}, NotImplementedError, "CTC_MAX_TARGET = 2047"),
    ((X, TG, IL, TL), {}, RuntimeError, r"must be on an MI355X \(ROCm\) device.*no CPU fallback"),
    ((X, TG, (6, 6), (2, 2)), dict(fused_log_softmax=False), RuntimeError, "no CPU fallback"),
])
def test_host_side_errors(args, kwargs, err, text):
    with pytest.raises(err, match=text):
        F.ctc_loss(*args, **kwargs)
    if "reduction" not in kwargs:
        with pytest.raises(err, match=text):
            T.CTCLoss(**kwargs)(*args)


def test_public_names_and_tiles():
    assert {"ctc_loss", "ctc_loss_tiles", "CTC_MAX_TARGET"} <= set(F.__all__) and "CTCLoss" in T.__all__
    configs, prefetch, widths, largest = F.ctc_loss_tiles()
    assert F.ctc_loss_tiles()[-1] == largest == F.CTC_MAX_TARGET == configs[-1][0]
    assert prefetch >= 1 and all(2 * s + 1 <= ks * nt for s, ks, nt in configs) and widths == F.rnnt_tiles()[0]


@pytest.mark.parametrize("name, tail", [("aamd_ctc_loss_forward", (None, None, None)),
                                        ("aamd_ctc_loss_backward", (None, None, 0, None, 0, 0, None))])
def test_c_abi_refuses_an_unknown_element_type(name, tail):
    rc = getattr(_lib.lib(), name)(9, None, 0, 0, None, 0, 0, 0, None, None, 0, 1, 1, 2, 0, 0, 1, 0, 0, *tail)
    assert rc != 0 and "ctc_loss: unknown element type" in _lib.lib().aamd_last_error().decode()
