"""_lib.TableBatch against fx_table_batch in include/fantoch_amd.h, as gcc
lays it out (size and every field's offset), and the table executor's
constants against the header's macros.  CPU only, no library call."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import pytest

from fantoch_amd import _lib
from fantoch_amd import table as ft

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CONSTANTS = ["FX_ERR_VOTE_RANGE", "FX_TABLE_ATTACHED", "FX_TABLE_DETACHED", "FX_TABLE_MAX_VOTES", "FX_TABLE_MAX_KEYS",
             "FX_TABLE_TIER_ONCHIP", "FX_TABLE_TIER_HBM", "FX_TABLE_ONCHIP_PENDING", "FX_TABLE_ONCHIP_KEYS",
             "FX_TABLE_ONCHIP_WINDOW", "FX_TABLE_HBM_PENDING", "FX_TABLE_HBM_WINDOW", "FX_PROFILE_SLOT_TABLE"]
HDRS = [(0, 0, 0), (1, 3, 7), (0, 64, (1 << 24) - 1), (1, 127, 12345)]


def _run_c():
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "fantoch_amd.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(fx_table_batch));']
    for name, _ in _lib.TableBatch._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(fx_table_batch, %s));' % (name, name))
    for c in CONSTANTS:
        lines.append('  printf("%s %%lu\\n", (unsigned long)%s);' % (c, c))
    for i, (kind, nv, key) in enumerate(HDRS):
        lines.append('  printf("hdr%d %%lu\\n", (unsigned long)FX_TABLE_HDR(%du, %du, %du));' % (i, kind, nv, key))
        for acc in ("KIND", "NVOTES", "KEY"):
            lines.append('  printf("%s%d %%lu\\n", (unsigned long)FX_TABLE_HDR_%s(FX_TABLE_HDR(%du, %du, %du)));'
                         % (acc, i, acc, kind, nv, key))
    lines.append('  printf("slots %lu\\n", (unsigned long)FX_PROFILE_SLOTS);')
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
def test_table_batch_matches_the_header():
    c = _run_c()
    assert ctypes.sizeof(_lib.TableBatch) == c["size"]
    for name, _ in _lib.TableBatch._fields_:
        assert getattr(_lib.TableBatch, name).offset == c[name], name
    for name in CONSTANTS:
        assert getattr(_lib, name) == c[name], name
    for i, (kind, nv, key) in enumerate(HDRS):
        assert ft.table_hdr(kind, nv, key) == c["hdr%d" % i]
        assert (c["KIND%d" % i], c["NVOTES%d" % i], c["KEY%d" % i]) == (kind, nv, key)
    # the table executor's profile slots lie inside the slot array
    assert _lib.FX_PROFILE_SLOT_TABLE + _lib.FX_TABLE_TIER_HBM < c["slots"]
