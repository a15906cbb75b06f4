"""_lib.TableBatchMk against fx_table_batch_mk in include/fantoch_amd.h, as
gcc lays it out, the multi-key constants against the header's macros, and the
argument checks of fx_table_execute_mk / fx_table_run_mk (they come before
the device is looked at).  CPU only."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import pytest

from fantoch_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CONSTANTS = ["FX_TABLE_MAX_CMD_KEYS", "FX_TABLE_MK_ONCHIP_LIVE", "FX_TABLE_MK_HBM_LIVE", "FX_TABLE_MK_ONCHIP_STACK",
             "FX_TABLE_MK_HBM_STACK", "FX_TABLE_MK_BUFFERED"]


def _run_c():
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "fantoch_amd.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(fx_table_batch_mk));',
             '  printf("base_size %zu\\n", sizeof(fx_table_batch));']
    for name, _ in _lib.TableBatchMk._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(fx_table_batch_mk, %s));' % (name, name))
    for name, _ in _lib.TableBatch._fields_:
        lines.append('  printf("base.%s %%zu\\n", offsetof(fx_table_batch_mk, base.%s));' % (name, name))
    for c in CONSTANTS:
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
def test_table_batch_mk_matches_the_header():
    c = _run_c()
    assert ctypes.sizeof(_lib.TableBatchMk) == c["size"]
    assert ctypes.sizeof(_lib.TableBatch) == c["base_size"]
    for name, _ in _lib.TableBatchMk._fields_:
        assert getattr(_lib.TableBatchMk, name).offset == c[name], name
    assert _lib.TableBatchMk.base.offset == 0
    for name, _ in _lib.TableBatch._fields_:
        assert getattr(_lib.TableBatch, name).offset == c["base." + name], name
    for name in CONSTANTS:
        assert getattr(_lib, name) == c[name], name
    # the kernel keeps one live op, one message and one buffered pair per lane and register row
    assert _lib.FX_TABLE_MK_ONCHIP_LIVE == _lib.FX_TABLE_ONCHIP_PENDING == _lib.FX_TABLE_MK_ONCHIP_STACK
    assert _lib.FX_TABLE_MK_HBM_LIVE == _lib.FX_TABLE_HBM_PENDING == _lib.FX_TABLE_MK_HBM_STACK


def _batch(nkeys=1, **over):
    """A batch whose pointers are never followed: the checks under test fail first."""
    f = dict(hdr=8, dot=8, clock=8, votes=8, lengths=None, num_streams=1, steps=4, n=3, keys=2, vmax=1,
             stability_threshold=2)
    f.update(over)
    base = _lib.TableBatch(*[f[name] for name, _ in _lib.TableBatch._fields_])
    return _lib.TableBatchMk(base, 8 if nkeys else None), _lib.OrderBatch(8, 8, 8, 8)


@pytest.mark.parametrize("over", [dict(nkeys=0), dict(hdr=None), dict(n=0), dict(n=17), dict(stability_threshold=4),
                                  dict(vmax=0), dict(vmax=65), dict(keys=0), dict(steps=1 << 26)])
def test_bad_arguments(lib, over):
    inb, outb = _batch(**over)
    ex = lambda i, o, tier=0, state=None, flags=0: lib.fx_table_execute_mk(i, o, None, None, 1, tier, state, flags, None)
    assert ex(ctypes.byref(inb), ctypes.byref(outb)) == _lib.FX_ERR_INVALID_ARG
    assert lib.fx_table_run_mk(ctypes.byref(inb), ctypes.byref(outb), None, 0, None, None) == _lib.FX_ERR_INVALID_ARG


def test_bad_calls(lib):
    inb, outb = _batch()
    i, o = ctypes.byref(inb), ctypes.byref(outb)
    ex = lambda i, o, lanes=1, tier=0, state=None, flags=0: lib.fx_table_execute_mk(i, o, None, None, lanes, tier, state,
                                                                                   flags, None)
    rr = ctypes.c_uint32(7)
    assert ex(None, o) == ex(i, None) == _lib.FX_ERR_INVALID_ARG
    assert lib.fx_table_run_mk(None, o, None, 0, None, ctypes.byref(rr)) == _lib.FX_ERR_INVALID_ARG and rr.value == 0
    assert lib.fx_table_run_mk(i, None, None, 0, None, None) == _lib.FX_ERR_INVALID_ARG
    assert ex(i, o, lanes=2) == _lib.FX_ERR_INVALID_ARG  # more lanes than streams without a map
    assert ex(i, o, tier=2) == _lib.FX_ERR_INVALID_ARG
    assert ex(i, o, tier=_lib.FX_TABLE_TIER_HBM) == _lib.FX_ERR_INVALID_ARG  # HBM without state
    assert ex(i, o, state=8) == _lib.FX_ERR_INVALID_ARG  # ONCHIP with state
    assert ex(i, o, flags=_lib.FX_FLAG_INIT) == _lib.FX_ERR_INVALID_ARG
    no_out = _lib.OrderBatch(8, 8, None, 8)
    assert ex(i, ctypes.byref(no_out)) == _lib.FX_ERR_INVALID_ARG
