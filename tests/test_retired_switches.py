"""The build-time A/B switches of the trajectory kernels that were retired ("Retired build-time switches": each fixed at
its measured value, the other arm deleted) stay retired: none of their names occurs in the engine's sources, in the scripts or in the
switch table of DESIGN.md §11.  A `-DAHMC_X=0` handed to scripts/build_variant.py for a name the sources no longer read would be
accepted and silently build the shipped code — a name that comes back must come back on purpose, with this list edited.

No build, no device: text only."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RETIRED = [
    # ahmc_nuts.hpp
    "AHMC_SCALAR_ANY", "AHMC_ADAPT_REREAD", "AHMC_RUNNING_STATS", "AHMC_HIER_PRE", "AHMC_CKPT_G64", "AHMC_CKPT_MIN_JW", "AHMC_TRANS_SCALAR",
    "AHMC_SLOTS_ADDRSPACE", "AHMC_DRAWS_PER_LANE", "AHMC_DRAW_SCALAR_WORD", "AHMC_LEAF_PAIR",
    # ahmc_kernels.hpp
    "AHMC_TAIL_NORMALS", "AHMC_CKPT",
    # ahmc_device.hpp
    "AHMC_LEAF_EXP", "AHMC_LEAF_EXP_NARROW_TABLE", "AHMC_LEAF_MICRO", "AHMC_UTURN_ANY", "AHMC_PAIR_LANE_STATS",
    # ahmc_dense.hpp
    "AHMC_EPOCH_NT",
]
# The two layout-mismatch messages of ahmc_api.hip keep their wording — callers and logs may match on it — and that wording names
# AHMC_CKPT.  The phrase is taken out before the search, and only there; the messages themselves are counted below.
LAYOUT_PHRASE = "(AHMC_CKPT / NUTS_* constants)"


def _names_in(text):
    return sorted(n for n in RETIRED if re.search(r"(?<![A-Za-z0-9_])" + re.escape(n) + r"(?![A-Za-z0-9_])", text))


def _design_section_11():
    text = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    m = re.search(r"^## 11\. .*?(?=^## 12\. )", text, flags=re.M | re.S)
    assert m, "DESIGN.md has no §11 followed by §12"
    return m.group(0)


def test_retired_switch_names_are_gone():
    assert len(RETIRED) == len(set(RETIRED)) == 19
    found = {}
    csrc = sorted(glob.glob(os.path.join(ROOT, "advancedhmc.jl_amd", "csrc", "*")))
    scripts = sorted(glob.glob(os.path.join(ROOT, "scripts", "*.py")))
    assert len([f for f in csrc if f.endswith((".hpp", ".hip"))]) >= 30 and len(scripts) >= 30, "the search did not find the sources"
    n_phrase = 0
    for f in csrc + scripts:
        if not os.path.isfile(f) or f.endswith((".so", ".digest", ".kdigest", ".kdigests")):
            continue
        text = open(f, encoding="utf-8", errors="replace").read()
        if os.path.basename(f) == "ahmc_api.hip":
            n_phrase = text.count(LAYOUT_PHRASE)
            text = text.replace(LAYOUT_PHRASE, "")
        names = _names_in(text)
        if names:
            found[os.path.relpath(f, ROOT)] = names
    names = _names_in(_design_section_11())
    if names:
        found["DESIGN.md §11"] = names
    assert not found, found
    assert n_phrase == 2, n_phrase   # the two messages are still there, in their wording
    # the switches that stay are still switches (a retirement that took one of them along would break the probes / the measurement scripts)
    device = open(os.path.join(ROOT, "advancedhmc.jl_amd", "csrc", "ahmc_device.hpp"), encoding="utf-8").read()
    nuts = open(os.path.join(ROOT, "advancedhmc.jl_amd", "csrc", "ahmc_nuts.hpp"), encoding="utf-8").read()
    for name, text in (("AHMC_MFMA_REDUCE", device), ("AHMC_DS_REDUCE", device), ("AHMC_LEAF_PROF", nuts), ("AHMC_WAVE_TIMELINE", nuts)):
        assert re.search(r"^#ifndef " + name + r"$", text, flags=re.M), name
