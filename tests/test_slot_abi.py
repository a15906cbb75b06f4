"""_lib.SlotBatch against fx_slot_batch in include/fantoch_amd.h, as gcc lays
it out (size and every field's offset), and the slot executor's constants
against the header's macros.  CPU only, no library call."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import pytest

from fantoch_amd import _lib
from fantoch_amd import slot as fslot

import slot_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CONSTANTS = ["FX_ERR_SLOT", "FX_SLOT_TIER_LANE", "FX_SLOT_TIER_SCAN", "FX_SLOT_LANE_WINDOW"]


def _run_c():
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "fantoch_amd.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(fx_slot_batch));']
    for name, _ in _lib.SlotBatch._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(fx_slot_batch, %s));' % (name, name))
    for c in CONSTANTS + ["FX_ERR_CAPACITY", "FX_RELEASE_NONE", "FX_ORDER_SCC_START"]:
        lines.append('  printf("%s %%lu\\n", (unsigned long)%s);' % (c, c))
    lines += ["  return 0;", "}"]
    d = tempfile.mkdtemp()
    try:
        src, exe = os.path.join(d, "abi.c"), os.path.join(d, "abi")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", exe, src], check=True,
                       capture_output=True, text=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    finally:
        shutil.rmtree(d, ignore_errors=True)
    return {ln.split()[0]: int(ln.split()[1]) for ln in out.split("\n") if ln}


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_slot_batch_matches_the_header():
    c = _run_c()
    assert ctypes.sizeof(_lib.SlotBatch) == c["size"]
    for name, _ in _lib.SlotBatch._fields_:
        assert getattr(_lib.SlotBatch, name).offset == c[name], name
    for name in CONSTANTS:
        assert getattr(_lib, name) == c[name], name
    # the restatement's and the Python mirror's copies
    assert (slot_ref.SLOT, slot_ref.CAPACITY, slot_ref.NONE, slot_ref.SCC_START) == \
        (c["FX_ERR_SLOT"], c["FX_ERR_CAPACITY"], c["FX_RELEASE_NONE"], c["FX_ORDER_SCC_START"])
    assert (fslot.LANE, fslot.SCAN, fslot.LANE_WINDOW) == \
        (c["FX_SLOT_TIER_LANE"], c["FX_SLOT_TIER_SCAN"], c["FX_SLOT_LANE_WINDOW"])
