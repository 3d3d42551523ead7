"""CPU test of the index arithmetic of the gradient pass's set-up (csrc/rnnt_lin.h lin_grad_indices).  The set-up fetches the
cell, both neighbours of the next diagonal, four frames and the label unconditionally, so every index must lie inside its array
for EVERY cell -- also where the neighbour does not exist: row n + 1 of the last utterance when N = T + U - 1 is a multiple of 16
(no row Nr), column u + 1 at u = Up - 1, the label at u = U - 1, and U = 1 (no label array).

tests/cell_prologue_host_main.hip is a stand-alone program with its own main(): it walks every (b, t, u) of the shapes below, for
blocks of four and of eight diagonals, against the extents of csrc/rnnt_common.h make_layout, and reads a byte of a host array of
that extent at every index.  It is built twice, plain and with the host sanitizers (address + undefined behaviour), and both
binaries are run directly; nothing of it is loaded into Python."""
import os
import shutil
import subprocess

import pytest

import rnnt_speech_recognition_amd as pkg

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cell_prologue_host_main.hip")
CSRC = os.path.join(os.path.dirname(os.path.abspath(pkg.__file__)), "csrc")
# the shapes of tests/test_cell_prologue_gpu.py, then: u + 1 = Up at the last column (U = 64, K = 1), three and four lattice
# columns per sweep lane (U = 150, 250), N a multiple of 16 with K = 3, and a shape of the headline's row stride
SHAPES = ["3,17,33", "1,1,1", "2,12,5", "2,10,7", "2,9,20", "1,3,64", "2,7,150", "1,11,150", "1,7,250", "2,600,150"]


@pytest.fixture(scope="module")
def hipcc():
    path = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(path), "hipcc not found (the library itself cannot be built without it)"
    return path


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_every_index_of_the_gradient_setup_is_inside_its_array(hipcc, tmp_path, sanitize):
    exe = str(tmp_path / "cell_prologue_host")
    cmd = [hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-I", CSRC, SRC, "-o", exe]
    if sanitize:
        cmd += ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    run = subprocess.run([exe] + SHAPES, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert ", 0 failed" in run.stdout.splitlines()[-1], run.stdout[-2000:]
    assert len([line for line in run.stdout.splitlines() if "checksum" in line]) == len(SHAPES)


def test_the_program_reports_a_bad_shape(hipcc, tmp_path):
    """(the checker sees what it is for) an argument that is no shape ends with status 2, not 0."""
    exe = str(tmp_path / "cell_prologue_host")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-I", CSRC, SRC, "-o", exe], check=True, capture_output=True)
    assert subprocess.run([exe, "0,1,1"], capture_output=True).returncode == 2
