"""The product sources hold no experiment switches (CPU only, reads text).

A JA_X_* macro selected a measured-and-rejected variant of a kernel, several of them with wrong pixels or coefficients: one
stray -D built a silently wrong library.  They live in tools/exp_patches/ablation_switches.diff now (tools/build_exp.py applies
it to a copy of the sources); these tests keep them, and new ones, out of jpeg_amd/csrc/ and include/."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Every JA_* macro a preprocessor conditional of the product sources may name, and why it may.
# Switches the product build never defines; a build that defines one still computes the same results:
SWITCHES = {
    "JA_PHASE_PROFILE": "per-phase cycle counters of k_quad420 (tools/phase_profile.py); results unchanged",
    "JA_GEN_PHASE": "per-phase cycle counters of k_generic_fused (tools/phase_generic.py, timeline_generic.py); results unchanged",
    "JA_ENC_TIMELINE": "start / end time of every k_encode_fused workgroup (tools/timeline_encode.py); results unchanged",
    "JA_DEBUG_ASSERTS": "traps on a violated lane precondition (lds_arrive, the DPP transposes); results unchanged",
    "JA_CHAIN_BITS": "host tunable of entropy.cpp: the size of a lookup table, range-checked by a static_assert; results unchanged",
}
# Not switches: the file that tests them defines them itself, to 0 or 1, from the target architecture (nothing to pass with -D).
TARGET_DERIVED = {
    "JA_X86_STREAMING": "entropy.cpp: x86-64 host compile -> streaming stores of the coefficient planes",
    "JA_X86_SSE2": "entropy_encode.cpp: x86-64 host compile -> SSE2 scan of a block",
}


def _sources():
    files = glob.glob(os.path.join(ROOT, "jpeg_amd", "csrc", "*")) + glob.glob(os.path.join(ROOT, "include", "*"))
    files = [f for f in files if os.path.isfile(f) and not f.endswith(".o")]   # (objects of an in-tree build)
    assert len(files) >= 25, files
    return {f: open(f, encoding="utf-8", errors="replace").read() for f in sorted(files)}


def test_no_experiment_switch_in_the_product_sources():
    hits = [os.path.relpath(f, ROOT) for f, text in _sources().items() if "JA_X_" in text]
    assert not hits, hits


def test_every_conditional_macro_is_a_listed_one():
    found = {}
    for f, text in _sources().items():
        text = text.replace("\\\n", " ")
        for line in text.splitlines():
            m = re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b(.*)", line)
            if m:
                for name in re.findall(r"\bJA_\w+", m.group(2).split("//")[0]):
                    found.setdefault(name, set()).add(os.path.basename(f))
    unlisted = {n: sorted(fs) for n, fs in found.items() if n not in SWITCHES and n not in TARGET_DERIVED}
    assert not unlisted, unlisted
    # the lists hold nothing the sources no longer use
    assert set(found) == set(SWITCHES) | set(TARGET_DERIVED)
    # a target-derived macro is #defined, on both arms, by the one file that tests it
    for name in TARGET_DERIVED:
        (fname,) = found[name]
        text = open(os.path.join(ROOT, "jpeg_amd", "csrc", fname)).read()
        assert len(re.findall(r"^#define %s [01]$" % name, text, flags=re.M)) == 2, name
