"""The state layout of fx_table_advance (fantoch_amd/csrc/table_state.h, the
index arithmetic its kernels use) compiled for the host under AddressSanitizer
and UBSan and driven as a stand-alone program (tests/table_state_main.cpp):
for every kind and 1, 32 and 999 keys every index is distinct and inside the
stream's stride, and the stride is what fx_table_session_bytes reports.  CPU only."""
import os
import shutil
import subprocess
import tempfile

import pytest

from fantoch_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX") or "g++"


@pytest.fixture(scope="module")
def program():
    if shutil.which(CXX) is None:
        pytest.skip("needs a host C++ compiler (%s)" % CXX)
    d = tempfile.mkdtemp()
    try:
        probe = os.path.join(d, "probe.cpp")
        open(probe, "w").write("int main() { return 0; }\n")
        san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
        ok = subprocess.run([CXX] + san + ["-o", os.path.join(d, "probe"), probe], capture_output=True)
        if ok.returncode != 0 or subprocess.run([os.path.join(d, "probe")], capture_output=True).returncode != 0:
            pytest.skip("%s has no AddressSanitizer / UBSan runtime" % CXX)
        exe = os.path.join(d, "table_state_main")
        subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + san +
                       ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "fantoch_amd", "csrc"),
                        "-o", exe, os.path.join(ROOT, "tests", "table_state_main.cpp")],
                       check=True, capture_output=True, text=True)
        yield exe
    finally:
        shutil.rmtree(d, ignore_errors=True)


@pytest.mark.parametrize("keys", [1, 32, 999])
@pytest.mark.parametrize("kind", [_lib.FX_TABLE_KIND_SINGLE, _lib.FX_TABLE_KIND_MK, _lib.FX_TABLE_KIND_PS])
def test_indices_are_distinct_and_inside_the_session_bytes(program, lib, kind, keys):
    run = subprocess.run([program, str(kind), str(keys)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    stride, image_at, marked = (int(x) for x in run.stdout.split())
    assert marked == stride > image_at
    for streams in (1, 7):
        assert lib.fx_table_session_bytes(kind, 3, keys, streams) == stride * 4 * streams
    tables = lib.fx_table_state_bytes_ps if kind == _lib.FX_TABLE_KIND_PS else lib.fx_table_state_bytes
    assert image_at * 4 == tables(3, keys, 1)
    assert (stride - image_at) * 4 <= 17 * 1024  # about 16 KB of registers per stream
