"""Every compile-time switch of the kernel sources has an owner.

A switch is an AAMD_* macro that a preprocessor conditional of audio_amd/csrc/*.h or *.hip tests.  Rounds 2-6 left about 35 of
them behind that no tool, test or build script named (retired: HISTORY.md, "Retired compile-time switches"); a reader of the
four hot kernels had to follow every one.  SWITCHES below is the whole list: a new switch lands with the file that sets or
documents it, a removed one takes its entry along.  No GPU, no compiler: macro names only."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name: (a file of the tree that sets or documents the switch, what it is for)
SWITCHES = {
    "AAMD_LAB": ("audio_amd/_build.py", "the lab library: tools-only kernel instantiations and their environment switches"),
    # (no file outside csrc/ sets this one: the header that defines it is its only documentation)
    "AAMD_UNROLL": ("audio_amd/csrc/rnnt_loss.h", "portability guard: the unroll pragma of the device compiler, nothing under g++"),
    "AAMD_M400_POOLS": ("tools/bench_pool_ab.py", "tail pools of the n_fft = 400 kernel (A/B builds; off in the product)"),
    "AAMD_M400_PK_BAND": ("tests/test_melspec400_packed.py", "headline kernel: band reduction as packed fp32"),
    "AAMD_M400_PK_TW": ("tests/test_melspec400_packed.py", "headline kernel: twiddle multiplies as packed fp32"),
    "AAMD_M400_PK_POW": ("tests/test_melspec400_packed.py", "headline kernel: power as packed fp32"),
    "AAMD_MFCC_FIXUP_RETURNS": ("tools/mfcc_fixup_cost.py", "timing only: the MFCC fix-up grid returns at once (its bare launch)"),
    "AAMD_RSM_LAB_NOMFMA": ("tools/rsm_lab.py", "timing only: the resampler's 8-byte loop without matrix instructions"),
    "AAMD_RSM_LAB_NOPERM": ("tools/rsm_lab.py", "timing only: ... without the regrouping instructions"),
    "AAMD_RSM_LAB_NOREAD": ("tools/rsm_lab.py", "timing only: ... operand tiles read once per round"),
    "AAMD_RSM_LAB_T1MASK": ("tools/rsm_lab.py", "timing only: ... steps that issue hi x hi alone"),
    "AAMD_FDR_LAB_NOBAR": ("tools/fdr_lab.py", "timing only: fftconvolve's workgroup barriers as wave-local fences"),
    "AAMD_FDR_LAB_NOH": ("tools/fdr_lab.py", "timing only: fftconvolve without the tap-spectrum reads"),
}

CONDITIONAL = re.compile(r"^[ \t]*#[ \t]*(?:if|ifdef|ifndef|elif)\b((?:.*\\\n)*.*)$", re.M)


def tested_macros():
    found = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "audio_amd", "csrc", "*.h")) + glob.glob(os.path.join(ROOT, "audio_amd", "csrc", "*.hip"))):
        with open(path, encoding="utf-8") as f:
            text = f.read()
        for m in CONDITIONAL.finditer(text):
            condition = re.sub(r"/\*.*?\*/|//.*", "", m.group(1), flags=re.S)
            for name in re.findall(r"\bAAMD_[A-Z0-9_]+\b", condition):
                found.setdefault(name, os.path.relpath(path, ROOT))
    return found


def test_the_registry_lists_exactly_the_switches_the_sources_test():
    found = tested_macros()
    assert len(found) >= 5, found                       # the scan found the sources at all
    unowned = {n: p for n, p in found.items() if n not in SWITCHES}
    assert not unowned, "switches without an entry in SWITCHES (who sets them?): %r" % unowned
    stale = sorted(set(SWITCHES) - set(found))
    assert not stale, "entries of SWITCHES that no conditional tests any more: %r" % stale


def test_every_owner_exists_and_names_its_switch():
    for name, (owner, purpose) in SWITCHES.items():
        path = os.path.join(ROOT, owner)
        assert os.path.isfile(path), (name, owner)
        with open(path, encoding="utf-8") as f:
            named = re.findall(r"AAMD_[A-Z0-9_]+\*?", f.read())         # (-DNAME counts; NAME_* names its whole family)
        assert any(name == n or (n.endswith("*") and name.startswith(n[:-1])) for n in named), "%s does not mention %s" % (owner, name)
        assert purpose.strip(), name
