"""Host check of csrc/sens_plan.h (no GPU): the index arithmetic that the kernels of the sensitivity family and
their host code must agree on.  For d = 1 .. 60 at T = 5 pass_of maps every output (di <= dj) to a pass whose decode
returns (di / T, dj / T), every pass 0 .. nb + nb (nb - 1) / 2 - 1 is hit and the largest index of the partials that
the pair kernel writes is pair_part_doubles - 1; tile_pair and tile_pair_lower enumerate each pair once in the
documented order for 1 .. 40 tiles; the two packed-triangle decodes of the reduce kernel are bijections.
tests/sens_plan_check.cpp is compiled with g++ under the address and undefined-behaviour sanitizers and run as a
program of its own."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def result(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("sens_plan") / "sens_plan_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "sens_plan_check.cpp"), "-o", exe],
                   check=True)
    return subprocess.run([exe], capture_output=True, text=True)


def test_sens_plan_index_arithmetic(result):
    assert result.stderr == "", result.stderr
    assert result.returncode == 0, result.stdout
    last = result.stdout.splitlines()[-1].split()
    assert last[0] == "ok" and int(last[1]) > 100000, result.stdout


def test_header_is_plain_cpp():
    """nothing from HIP and no other header of the library: the check above includes it alone"""
    with open(os.path.join(ROOT, "outerbase_amd", "csrc", "sens_plan.h")) as f:
        includes = [line.split()[1] for line in f if line.startswith("#include")]
    assert includes == ["<cstdint>"]
