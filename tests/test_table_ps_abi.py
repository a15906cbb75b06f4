"""The constants and macros of the table executor over several shards against
include/fantoch_amd.h as gcc compiles it, and the argument checks of
fx_table_execute_ps / fx_table_run_ps (they come before the device is looked
at).  CPU only."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import pytest

from fantoch_amd import _lib
from fantoch_amd import table as ft

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CONSTANTS = ["FX_TABLE_MAX_CMD_SHARDS", "FX_TABLE_PS_ONCHIP_BUFFERED", "FX_TABLE_PS_HBM_BUFFERED",
             "FX_TABLE_MK_BUFFERED", "FX_TABLE_MK_HBM_LIVE", "FX_TABLE_MAX_CMD_KEYS", "FX_TABLE_MAX_VOTES"]
EXPRESSIONS = {
    "word_2_3": "FX_TABLE_PS_WORD(2, 3)", "word_8_8": "FX_TABLE_PS_WORD(8, 8)", "word_1_1": "FX_TABLE_PS_WORD(1, 1)",
    "word_nkeys": "FX_TABLE_PS_WORD_NKEYS(FX_TABLE_PS_WORD(5, 7))",
    "word_shards": "FX_TABLE_PS_WORD_SHARDS(FX_TABLE_PS_WORD(5, 7))",
    "stable_5": "FX_TABLE_HDR_STABLE(5)", "stable_kind": "FX_TABLE_HDR_KIND(FX_TABLE_HDR_STABLE(5))",
    "stable_nvotes": "FX_TABLE_HDR_NVOTES(FX_TABLE_HDR_STABLE(5))", "stable_key": "FX_TABLE_HDR_KEY(FX_TABLE_HDR_STABLE(5))",
    "stable_max_key": "FX_TABLE_HDR_KEY(FX_TABLE_HDR_STABLE(FX_TABLE_MAX_KEYS - 1))",
}


def _run_c():
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "fantoch_amd.h"', "int main(void) {"]
    for c in CONSTANTS:
        lines.append('  printf("%s %%lu\\n", (unsigned long)%s);' % (c, c))
    for name, expr in EXPRESSIONS.items():
        lines.append('  printf("%s %%lu\\n", (unsigned long)(%s));' % (name, expr))
    lines += ["  return 0;", "}",
              # the new entry points are declared with stable_sent where the issue puts it (unevaluated: no link)
              "_Static_assert(_Generic(&fx_table_execute_ps, int (*)(const fx_table_batch_mk*, const fx_order_batch*,"
              " uint32_t*, uint32_t*, const uint32_t*, uint32_t, uint32_t, void*, uint32_t, void*): 1, default: 0),"
              ' "fx_table_execute_ps");',
              "_Static_assert(_Generic(&fx_table_run_ps, int (*)(const fx_table_batch_mk*, const fx_order_batch*,"
              ' uint32_t*, uint32_t*, uint32_t, void*, uint32_t*): 1, default: 0), "fx_table_run_ps");',
              "_Static_assert(_Generic(&fx_table_state_bytes_ps, size_t (*)(uint32_t, uint32_t, uint32_t): 1,"
              ' default: 0), "fx_table_state_bytes_ps");']
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
def test_constants_and_macros_match_the_header():
    c = _run_c()
    for name in CONSTANTS:
        assert getattr(_lib, name) == c[name], name
    assert c["FX_TABLE_MAX_CMD_SHARDS"] == 8 and c["FX_TABLE_PS_ONCHIP_BUFFERED"] == 64
    assert c["FX_TABLE_PS_HBM_BUFFERED"] >= c["FX_TABLE_MK_HBM_LIVE"]
    assert c["FX_TABLE_PS_ONCHIP_BUFFERED"] == c["FX_TABLE_MK_BUFFERED"]  # one per lane, as before
    assert (c["word_2_3"], c["word_8_8"], c["word_1_1"]) == (2 | 3 << 8, 8 | 8 << 8, 0x101)
    assert (c["word_nkeys"], c["word_shards"]) == (5, 7)
    assert c["word_2_3"] == ft.table_ps_word(2, 3)
    assert c["stable_5"] == ft.table_hdr_stable(5) == (1 << 31) | (127 << 24) | 5
    assert (c["stable_kind"], c["stable_nvotes"], c["stable_key"]) == (_lib.FX_TABLE_DETACHED, 127, 5)
    assert c["stable_max_key"] == _lib.FX_TABLE_MAX_KEYS - 1
    assert c["stable_nvotes"] == ft.STABLE_NVOTES > c["FX_TABLE_MAX_VOTES"]  # the old entry points refuse the event


def test_state_bytes(lib):
    """The HBM tier keeps its buffered pairs in `state`: three words each
    behind the votes tables; fx_table_state_bytes is what it was."""
    for keys, lanes in ((1, 1), (16, 3), (33, 70)):
        base = lib.fx_table_state_bytes(5, keys, lanes)
        assert base == keys * 16 * (1 + _lib.FX_TABLE_HBM_WINDOW // 32) * 4 * lanes
        assert lib.fx_table_state_bytes_ps(5, keys, lanes) == base + 3 * 4 * _lib.FX_TABLE_PS_HBM_BUFFERED * lanes


def _batch(nkeys=1, **over):
    """A batch whose pointers are never followed: the checks under test fail first."""
    f = dict(hdr=8, dot=8, clock=8, votes=8, lengths=None, num_streams=1, steps=4, n=3, keys=2, vmax=1,
             stability_threshold=2)
    f.update(over)
    base = _lib.TableBatch(*[f[name] for name, _ in _lib.TableBatch._fields_])
    return _lib.TableBatchMk(base, 8 if nkeys else None), _lib.OrderBatch(8, 8, 8, 8)


@pytest.mark.parametrize("sent", [None, 8])
@pytest.mark.parametrize("over", [dict(nkeys=0), dict(hdr=None), dict(dot=None), dict(n=0), dict(n=17),
                                  dict(stability_threshold=4), dict(vmax=0), dict(vmax=65), dict(keys=0),
                                  dict(steps=1 << 26)])
def test_bad_arguments(lib, over, sent):
    inb, outb = _batch(**over)
    i, o = ctypes.byref(inb), ctypes.byref(outb)
    assert lib.fx_table_execute_ps(i, o, None, sent, None, 1, 0, None, 0, None) == _lib.FX_ERR_INVALID_ARG
    assert lib.fx_table_run_ps(i, o, None, sent, 0, None, None) == _lib.FX_ERR_INVALID_ARG


def test_bad_calls(lib):
    inb, outb = _batch()
    i, o = ctypes.byref(inb), ctypes.byref(outb)
    ex = lambda i, o, lanes=1, tier=0, state=None, flags=0: lib.fx_table_execute_ps(i, o, None, None, None, lanes, tier,
                                                                                   state, flags, None)
    rr = ctypes.c_uint32(7)
    assert ex(None, o) == ex(i, None) == _lib.FX_ERR_INVALID_ARG
    assert lib.fx_table_run_ps(None, o, None, None, 0, None, ctypes.byref(rr)) == _lib.FX_ERR_INVALID_ARG
    assert rr.value == 0
    assert lib.fx_table_run_ps(i, None, None, None, 0, None, None) == _lib.FX_ERR_INVALID_ARG
    assert ex(i, o, lanes=2) == _lib.FX_ERR_INVALID_ARG  # more lanes than streams without a map
    assert ex(i, o, tier=2) == _lib.FX_ERR_INVALID_ARG
    assert ex(i, o, tier=_lib.FX_TABLE_TIER_HBM) == _lib.FX_ERR_INVALID_ARG  # HBM without state
    assert ex(i, o, state=8) == _lib.FX_ERR_INVALID_ARG  # ONCHIP with state
    assert ex(i, o, flags=_lib.FX_FLAG_INIT) == _lib.FX_ERR_INVALID_ARG
    no_out = _lib.OrderBatch(8, 8, None, 8)
    assert ex(i, ctypes.byref(no_out)) == _lib.FX_ERR_INVALID_ARG
