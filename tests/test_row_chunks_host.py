"""Host check of the arithmetic part of csrc/row_chunks.h (no GPU): pad128, the chunk size under a byte cap and the
plan of row chunks that post_var_dev, row_forms_dev, the acquisition gradients and the unfused extremum walk.  For
pp in {128, 256, 4096, 16384, 65536} at the 1 GiB and 8 GiB caps and for chunk sizes 128 and 256 given outright,
n in {1, 127, 128, 129, 300, cmax - 1, cmax, cmax + 1, 3 cmax + 44}: the chunks tile [0, n) in ascending order
without gap or overlap, all but the last have cmax rows, npad = pad128(nr) >= nr, `whole` holds exactly for the one
chunk that is the call, and a block of pp x npad doubles stays within the cap whenever cmax > 128; chunk_rows_for
returns 1 048 576 at (128, 1 GiB), 32 768 at (4096, 1 GiB), 2048 at (65536, 1 GiB), 65 536 at (16384, 8 GiB) and 128
where the quotient falls below 128.  tests/row_chunks_check.cpp is compiled with g++ under the address and
undefined-behaviour sanitizers and run as a program of its own."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "outerbase_amd", "csrc", "row_chunks.h")


@pytest.fixture(scope="module")
def result(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("row_chunks") / "row_chunks_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "row_chunks_check.cpp"), "-o", exe],
                   check=True)
    return subprocess.run([exe], capture_output=True, text=True)


def test_row_chunk_arithmetic(result):
    assert result.stderr == "", result.stderr
    assert result.returncode == 0, result.stdout
    last = result.stdout.splitlines()[-1].split()
    assert last[0] == "ok" and int(last[1]) > 1000, result.stdout


def test_arithmetic_part_is_plain_cpp():
    """nothing from HIP and no header of the library before the frame, which only the HIP compiler sees: the check
    above includes the header alone; and the family's host files read no environment variable through it"""
    with open(HEADER) as f:
        src = f.read()
    plain, frame = src.split("#if defined(__HIPCC__)")
    assert [ln.split()[1] for ln in plain.splitlines() if ln.startswith("#include")] == ["<algorithm>", "<cstdint>"]
    assert [ln.split()[1] for ln in frame.splitlines() if ln.startswith("#include")] == ['"obhip_internal.h"']
    assert "getenv" not in src
